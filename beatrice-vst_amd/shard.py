"""Multi-process plumbing for the data-parallel path: one process per GPU,
streams sharded by rank, model bytes broadcast once from rank 0 (RCCL over xGMI when the backend is
nccl; gloo on CPU in the tests), no collective inside a hop."""
import os

MODEL_FILES = ("phone_extractor.bin", "pitch_estimator.bin", "waveform_generator.bin",
               "embedding_setter.bin", "speaker_embeddings.bin")


def stream_range(rank, world, total_streams):
    """Contiguous shard [lo, hi) of `total_streams` for `rank`; the remainder goes to the first ranks."""
    base, rem = divmod(total_streams, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def broadcast_bytes(data, rank, world, dist, torch, device):
    """rank 0's `data` (bytes) -> every rank, as ONE broadcast of a uint8 tensor on `device`."""
    if world == 1:
        return data
    n = torch.tensor([len(data) if rank == 0 else 0], dtype=torch.int64, device=device)
    dist.broadcast(n, 0)
    if rank == 0:
        buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(device)
    else:
        buf = torch.empty(int(n.item()), dtype=torch.uint8, device=device)
    dist.broadcast(buf, 0)
    return buf.cpu().numpy().tobytes()


def broadcast_model(model_dir, rank, world, dist, torch, device):
    """Returns {file name: bytes} on every rank; only rank 0 needs `model_dir` populated."""
    blobs = {}
    for f in MODEL_FILES:
        data = open(os.path.join(model_dir, f), "rb").read() if rank == 0 else b""
        blobs[f] = broadcast_bytes(data, rank, world, dist, torch, device)
    return blobs


class _DeviceView:
    """Foreign device memory (a pointer handed out by the C-ABI) as something torch can alias without copying."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(ptr), False),
                                         "strides": None, "version": 2}


def device_bytes(torch, ptr, nbytes, device="cuda"):
    """uint8 tensor ALIASING [ptr, ptr + nbytes) of device memory owned by the library."""
    return torch.as_tensor(_DeviceView(ptr, nbytes), device=device)


def broadcast_inplace(buf, world, dist, src=0):
    """One broadcast of `buf` (a tensor every rank holds with the same size): rank `src`'s contents land in the
    other ranks' `buf`, device to device when the tensors are device memory (RCCL over xGMI)."""
    if world > 1:
        dist.broadcast(buf, src)
    return buf


KINDS = (("phone", 1, "ReadPhoneExtractorParameters", "phone_extractor.bin"),
         ("pitch", 2, "ReadPitchEstimatorParameters", "pitch_estimator.bin"),
         ("wave", 3, "ReadWaveformGeneratorParameters", "waveform_generator.bin"),
         ("embed", 4, "ReadEmbeddingSetterParameters", "embedding_setter.bin"))


def all_ranks_ok(ok, world, dist, torch, device):
    """True only if `ok` is true on every rank (MIN all-reduce): ranks must take the same branch before a collective."""
    if world == 1:
        return bool(ok)
    t = torch.tensor([1 if ok else 0], dtype=torch.int32, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    return bool(int(t.item()))


LOADERS = {"phone": "BeatriceHip_LoadPhoneExtractorFromMemory", "pitch": "BeatriceHip_LoadPitchEstimatorFromMemory",
           "wave": "BeatriceHip_LoadWaveformGeneratorFromMemory", "embed": "BeatriceHip_LoadEmbeddingSetterFromMemory"}


def load_models_from_rank0(product, objs, model_dir, rank, world, dist, torch, device="cuda"):
    """The four model objects of this rank (objs: name -> handle, freshly created).  Rank 0 reads and packs the files
    (Read*Parameters); every other rank gets an empty device blob of the same size (BeatriceHip_ModelBlob) that
    receives rank 0's PACKED blob by one broadcast each, device to device -- no file, no host copy, no repacking --
    and is then marked ready.  If any rank cannot expose its blobs to torch, ALL ranks agree (all_ranks_ok) to ship
    the file bytes instead (broadcast_bytes + BeatriceHip_Load*FromMemory).  Returns (bytes broadcast, path taken)."""
    import ctypes as C
    views, ok = {}, True
    for name, kind, reader, fname in KINDS:
        if rank == 0:
            err = getattr(product, reader)(objs[name], os.path.join(model_dir, fname).encode())
            if err:
                raise RuntimeError("%s: Beatrice_ErrorCode %d" % (fname, err))
        if world == 1:
            continue
        try:
            ptr, nbytes = C.c_void_p(), C.c_size_t()
            rc = product.BeatriceHip_ModelBlob(kind, objs[name], 0 if rank == 0 else 1, C.byref(ptr), C.byref(nbytes))
            if rc:
                raise RuntimeError("BeatriceHip_ModelBlob(%s): %d" % (name, rc))
            views[name] = device_bytes(torch, ptr.value, nbytes.value, device)
        except Exception as e:  # noqa: BLE001 -- any failure means "take the other path", decided collectively below
            print("shard: rank %d cannot share the %s blob in place (%s)" % (rank, name, e))
            ok = False
    if world == 1:
        return 0, "file"
    if all_ranks_ok(ok, world, dist, torch, device):
        moved = 0
        for name, kind, _, _ in KINDS:
            broadcast_inplace(views[name], world, dist)
            moved += views[name].numel()
            if rank != 0:
                torch.cuda.synchronize()
                rc = product.BeatriceHip_ModelBlobReady(kind, objs[name])
                if rc:
                    raise RuntimeError("BeatriceHip_ModelBlobReady(%s): %d" % (name, rc))
        return moved, "device blobs, in place"
    moved = 0
    for name, kind, _, fname in KINDS:
        data = open(os.path.join(model_dir, fname), "rb").read() if rank == 0 else b""
        data = broadcast_bytes(data, rank, world, dist, torch, device)
        moved += len(data)
        if rank != 0:
            fn = getattr(product.lib, LOADERS[name])
            fn.restype = C.c_int
            fn.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
            err = fn(objs[name], data, len(data))
            if err:
                raise RuntimeError("%s: Beatrice_ErrorCode %d" % (LOADERS[name], err))
    return moved, "file bytes, repacked per rank"


def share_speaker_tables(product, batch_handle, n_speakers, rank, world, dist, torch, device="cuda", host_tables=None):
    """Rank 0 has uploaded its tables (BeatriceBatch_SetSpeakerTables); the raw device tables go to the other ranks
    by four broadcasts and are projected there (BeatriceBatch_ProjectSpeakerTables).  Fallback, agreed by all ranks:
    rank 0's host arrays (host_tables: the SpeakerTables object, rank 0 only) are broadcast and every other rank calls
    BeatriceBatch_SetSpeakerTables itself.  Returns (bytes broadcast, path taken)."""
    import ctypes as C
    import numpy as np
    if world == 1:
        return 0, "file"
    views, ok = [], True
    try:
        ptrs, sizes = (C.c_void_p * 4)(), (C.c_size_t * 4)()
        rc = product.BeatriceBatch_SpeakerTablesDevice(batch_handle, ptrs, sizes)
        if rc:
            raise RuntimeError("BeatriceBatch_SpeakerTablesDevice: %d" % rc)
        views = [device_bytes(torch, ptrs[i], sizes[i], device) for i in range(4)]
    except Exception as e:  # noqa: BLE001
        print("shard: rank %d cannot share its speaker tables in place (%s)" % (rank, e))
        ok = False
    if all_ranks_ok(ok, world, dist, torch, device):
        for v in views:
            broadcast_inplace(v, world, dist)
        if rank != 0:
            torch.cuda.synchronize()
            rc = product.BeatriceBatch_ProjectSpeakerTables(batch_handle, n_speakers)
            if rc:
                raise RuntimeError("BeatriceBatch_ProjectSpeakerTables: %d" % rc)
        return int(sum(v.numel() for v in views)), "device tables, in place"
    shapes = ((n_speakers, 512, 128), (n_speakers, 256), (9, 256), (n_speakers, 384, 128))  # codebooks, additive, formant, kv
    arrays, moved = [], 0
    for i, shape in enumerate(shapes):
        src = (host_tables.codebooks, host_tables.additive, host_tables.formant, host_tables.kv)[i] if rank == 0 else None
        t = torch.from_numpy(np.ascontiguousarray(src, dtype=np.float32)).to(device) if rank == 0 else \
            torch.empty(shape, dtype=torch.float32, device=device)
        dist.broadcast(t, 0)
        arrays.append(np.ascontiguousarray(t.cpu().numpy()))
        moved += t.numel() * 4
    if rank != 0:
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        rc = product.BeatriceBatch_SetSpeakerTables(batch_handle, n_speakers, fp(arrays[0]), fp(arrays[1]), fp(arrays[2]), fp(arrays[3]))
        if rc:
            raise RuntimeError("BeatriceBatch_SetSpeakerTables: %d" % rc)
    return moved, "host tables, projected per rank"


def affine_speaker(rank, world, local_stream, n_speakers):
    """Speaker-affine placement: rank r starts its streams on the speakers congruent to r
    modulo the world size, so a GPU keeps 1/world of the codebooks and K/V tables hot.  With fewer speakers than
    ranks every rank cycles through all of them."""
    if n_speakers < world:
        return local_stream % n_speakers
    # the speakers congruent to `rank`: rank, rank + world, ... below n_speakers -- ceil((n_speakers - rank) / world) of
    # them, so that the ranks' sets PARTITION the table for any n_speakers (64 over 3 ranks: 22 + 21 + 21)
    mine = (n_speakers - rank + world - 1) // world
    return rank + world * (local_stream % mine)


def _around_48k(batch):
    """True when the batch converts resident 48 kHz blocks (BeatriceBatch_BindResidentIO48k): the one mode in which
    BeatriceBatch_Stream48kQuiescent answers at all."""
    ask = getattr(batch.a, "BeatriceBatch_Stream48kQuiescent", None)
    return ask is not None and ask(batch.h, 0) >= 0


def _move_streams_in_flight(src_batch, src_streams, dst_batch, dst_streams, entry_map, reset_source):
    """move_streams(in_flight=True): both batches are in plain tick mode, or both convert resident 48 kHz blocks, and go on ticking;
    the streams named are quiescent (Batch.stream_quiescent / Batch.stream48k_quiescent).  On one device the rings go from batch to
    batch on the device and nothing is returned; across devices the in-flight blob pair carries them and the blobs are returned.
    One batch in each of the two modes: the plain calls are asked and refuse."""
    a = src_batch.a
    k48 = _around_48k(src_batch) and _around_48k(dst_batch)
    if a.BeatriceBatch_Device(src_batch.h) == dst_batch.a.BeatriceBatch_Device(dst_batch.h):
        (src_batch.move_streams48k_in_flight if k48 else src_batch.move_streams_in_flight)(dst_batch, src_streams, dst_streams, entry_map)
        blobs = None
    else:
        blobs = (src_batch.export_streams48k_in_flight if k48 else src_batch.export_streams_in_flight)(src_streams)
        (dst_batch.import_streams48k_in_flight if k48 else dst_batch.import_streams_in_flight)(dst_streams, blobs, entry_map)
    if reset_source:
        for s in src_streams:
            src_batch._check(a.BeatriceBatch_ResetStreamInFlight(src_batch.h, int(s)))
    return blobs


def move_streams(src_batch, src_streams, dst_batch, dst_streams, entry_map=None, reset_source=False, with_wrapper=False, in_flight=False):
    """Stream src_streams[i] of src_batch goes on as stream dst_streams[i] of dst_batch, with its state and settings
    (Batch.export_streams / Batch.import_streams): its next step there is bit for bit the step it would have run in
    src_batch.  Both batches drain.  The two are batches of ONE process (any two GPUs of it: each call runs on its batch's
    device); they must come from the same library build and have the same hops per step.  entry_map[i] = the table entry of
    dst_batch that holds what entry i of src_batch holds (None: the same entries) -- that the tables, and an active morph's
    weights, are equal there is the caller's promise.  reset_source: BeatriceBatch_ResetStream on the source streams
    afterwards, so that the slots start from silence for their next users.  Returns the blobs.

    with_wrapper: both batches run clocks per stream (BeatriceBatch_ConfigureWrapperRates / ProcessBlocksRagged) and the stream
    takes its host side along as well -- its rate, resampler histories and clocks, FIFO and gain ramps (Batch.export_stream_wrappers /
    Batch.import_stream_wrappers) -- so that its next BLOCK there is the block it would have got in src_batch; reset_source then
    also restarts the source slots' wrappers.  Returns (blobs, wrapper_blobs).

    Between ranks the blob is plain bytes: export_streams on the rank that has the stream, broadcast_bytes (or a
    point-to-point send of a uint8 tensor) to the rank that takes it, import_streams there.

    in_flight: neither batch drains (both in plain tick mode, or both bound to resident 48 kHz blocks -- then the 48 kHz wrapper's
    state travels too; the streams quiescent): the device-to-device call when both batches live on one device (returns None), the
    in-flight blob pair otherwise (returns the blobs); reset_source then marks the source slots with
    BeatriceBatch_ResetStreamInFlight, which drains in neither mode.  The any-rate wrapper's state does not travel this way:
    with_wrapper is refused."""
    if len(src_streams) != len(dst_streams):
        raise ValueError("move_streams: %d source streams, %d destination streams" % (len(src_streams), len(dst_streams)))
    if in_flight:
        if with_wrapper:
            raise ValueError("move_streams: in_flight=True moves no wrapper state (with_wrapper=True needs the drained path)")
        return _move_streams_in_flight(src_batch, src_streams, dst_batch, dst_streams, entry_map, reset_source)
    blobs = src_batch.export_streams(src_streams)
    wrapper_blobs = src_batch.export_stream_wrappers(src_streams) if with_wrapper else None
    dst_batch.import_streams(dst_streams, blobs, entry_map)
    if with_wrapper:
        dst_batch.import_stream_wrappers(dst_streams, wrapper_blobs)
    if reset_source:
        for s in src_streams:
            src_batch._check(src_batch.a.BeatriceBatch_ResetStream(src_batch.h, int(s)))
            if with_wrapper:
                src_batch.restart_stream_wrapper(s)
    return (blobs, wrapper_blobs) if with_wrapper else blobs


def move_bound_streams(src, streams, dst, dst_streams, entry_map=None, turn_over_source=False):
    """Stream streams[i] of `src` goes on as stream dst_streams[i] of `dst` while BOTH batches stay bound with clocks per stream
    (BeatriceBatch_BindResidentBlocksRagged) and neither drains: the streams named are at rest (Batch.bound_stream_quiescent), and the
    stream's next block in `dst` is the block it would have got in `src` -- model state, settings, rate, resampler and FIFO state, gain
    ramps.  On one device the state goes from batch to batch on the device and None is returned; across devices the in-flight blob pair
    carries it and (blobs, wrapper_blobs) is returned.  turn_over_source: the source slots are turned over to new callers
    (BeatriceBatch_RestartStreamInFlight(s, 0.0, 1)).  move_streams is the drained way, and the way of every other mode."""
    if len(streams) != len(dst_streams):
        raise ValueError("move_bound_streams: %d source streams, %d destination streams" % (len(streams), len(dst_streams)))
    if src.a.BeatriceBatch_Device(src.h) == dst.a.BeatriceBatch_Device(dst.h):
        src.move_bound_streams_in_flight(dst, streams, dst_streams, entry_map)
        out = None
    else:
        out = src.export_bound_streams_in_flight(streams)
        dst.import_bound_streams_in_flight(dst_streams, out[0], out[1], entry_map)
    if turn_over_source:
        for s in streams:
            src._check(src.a.BeatriceBatch_RestartStreamInFlight(src.h, int(s), 0.0, 1))
    return out


def max_over_ranks(value, world, dist, torch, device):
    if world == 1:
        return value
    t = torch.tensor([value], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def gather_over_ranks(value, world, dist, torch, device):
    """every rank's value, in rank order (all ranks receive the list)"""
    if world == 1:
        return [value]
    t = torch.tensor([value], dtype=torch.float64, device=device)
    out = [torch.zeros_like(t) for _ in range(world)]
    dist.all_gather(out, t)
    return [float(x.item()) for x in out]
