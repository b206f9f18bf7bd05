/*
 * beatrice_batch.h -- batched extension of the beatrice C-ABI (this project's addition).
 *
 * The reference library is one-stream-per-context: one plugin instance = one stream = one thread
 * (reference src/vst/processor.h:56-57, factory.cc:21 kManyInstances); its per-hop entry points
 * carry the suffix "1" (ExtractPhone1 / EstimatePitch1 / GenerateWaveform1,
 * reference lib/beatricelib/beatrice.h:243-247, 266-271, 301-307).  A GPU wants many streams per
 * launch, so this header adds an N-stream object that runs the SAME three modules, in the same
 * order, for B independent streams per call, and keeps the reference host's per-stream settings
 * and call protocol (reference src/common/processor_core_2.cc):
 *
 *   reference ProcessorCore2 member            ->  batched entry point (per stream)
 *   SetTargetSpeaker        (:431-466)             BeatriceBatch_SetTargetSpeaker
 *     + one K/V block per hop (:179-181, .h:161)   (applied inside BeatriceBatch_ConvertFrames)
 *   SetFormantShift         (:468-481)             BeatriceBatch_SetFormantShift
 *   SetPitchShift / SetAverageSourcePitch /
 *   SetIntonationIntensity / SetPitchCorrection /
 *   SetPitchCorrectionType  (:483-559)             BeatriceBatch_SetPitch*   (math of :190-252 on device)
 *   SetMinSourcePitch / SetMaxSourcePitch (:561-583) BeatriceBatch_SetMin/MaxSourcePitch
 *   SetVQNumNeighbors       (:585-590)             BeatriceBatch_SetVQNumNeighbors
 *   ResetContext            (:258-291)             BeatriceBatch_ResetStream
 *   Process1                (:50-256)              BeatriceBatch_ConvertFrames (one hop, all streams)
 *
 * All functions return 0 on success and a negative value on error (bad argument -1, HIP failure -2);
 * they never throw.  `stream` = -1 addresses every stream.  Plain C types only.
 */
#ifndef BEATRICE_BATCH_H_
#define BEATRICE_BATCH_H_

#include <stddef.h>
#include <stdint.h>

#include "beatrice_abi.h"

BEATRICE_ABI_BEGIN

typedef struct BeatriceBatch BeatriceBatch;

/* Parameter blobs that arrive over the wire (e.g. broadcast with RCCL from rank 0) instead of from
 * a file: same validation and error codes as the Read*Parameters functions. */
Beatrice_ErrorCode BeatriceHip_LoadPhoneExtractorFromMemory(Beatrice20rc0_PhoneExtractor* m, const void* bytes, size_t size);
Beatrice_ErrorCode BeatriceHip_LoadPitchEstimatorFromMemory(Beatrice20rc0_PitchEstimator* m, const void* bytes, size_t size);
Beatrice_ErrorCode BeatriceHip_LoadWaveformGeneratorFromMemory(Beatrice20rc0_WaveformGenerator* m, const void* bytes, size_t size);
Beatrice_ErrorCode BeatriceHip_LoadEmbeddingSetterFromMemory(Beatrice20rc0_EmbeddingSetter* m, const void* bytes, size_t size);

/* Beatrice20rc0_SetCodebook (beatrice.h:318-322) is called per hop on the audio thread in morph mode and therefore recognises
 * a caller-owned table by address + a 96-word sample of its contents.  After rewriting a table IN PLACE (the same address)
 * call this, off the audio thread, so that the next SetCodebook of it uploads the new contents; NULL forgets every table. */
void BeatriceHip_InvalidateCodebook(Beatrice20rc0_PhoneContext1* ctx, const float* codebook);
/* Test hook for the recovery path of the 1-stream team launches (a launch whose workgroups could not all become resident gives its
 * waits up after ~0.3 s instead of hanging the GPU): the context's next GenerateWaveform1 returns zeros, its state restarts from
 * silence, and from then on the context runs one launch per layer.  -1: the context has no team launch. */
int BeatriceHip_InjectTeamTimeout(Beatrice20rc0_WaveformContext1* ctx);
/* ... and for the content encoder's and the pitch estimator's contexts (the next ExtractPhone1 / EstimatePitch1 returns zeros, the context restarts from
 * silence like a new one and runs one launch per layer from then on), and for a ONE-STREAM batch, whose in-order chain uses the same team launches (the
 * steps since the last BeatriceBatch_Synchronize are void: it returns -2 once, the stream restarts from silence, the batch stays usable).  -1: no team launch. */
int BeatriceHip_InjectTeamTimeoutPhone(Beatrice20rc0_PhoneContext1* ctx);
int BeatriceHip_InjectTeamTimeoutPitch(Beatrice20rc0_PitchContext1* ctx);
/* Test hook: the hop counter of a 1-stream context (the same counter, the same wrap at BEATRICE_HIP_STEP_WRAP, below: it addresses the
 * context's rings and travels to the device with every hop's input).  kind: 1 phone, 2 pitch, 3 waveform context; ctx a context of the
 * 2.0.0-rc.0 generation (BeatriceHip_SetHopCount) or of a legacy generation, Beatrice20a2_* / Beatrice20b1_* (BeatriceHip_SetHopCountLegacy).
 * FRESH contexts only -- before the context's first hop, when all its rings are zeros and a context started at counter c computes what one
 * started at 0 computes.  The three contexts of a stream count independently: set all three.  0; -1 and no change for an unknown kind, a
 * bad context, a counter outside [0, BEATRICE_HIP_STEP_WRAP) or a context that has run a hop.  BeatriceHip_HopCount[Legacy] reads the
 * counter of the context's NEXT hop (-1: unknown kind, bad context). */
int BeatriceHip_SetHopCount(int kind, void* ctx, int counter);
int BeatriceHip_SetHopCountLegacy(int kind, void* ctx, int counter);
int BeatriceHip_HopCount(int kind, const void* ctx);
int BeatriceHip_HopCountLegacy(int kind, const void* ctx);
/* The pitch call beside the phone call.  The reference's hop calls ExtractPhone1 and EstimatePitch1 one after the other on the SAME 160 samples
 * (src/common/processor_core_2.cc:184,188); the two modules are independent.  Once a pitch context has been called right after a phone context with
 * the same samples (same thread), that phone context's calls also start the pitch context's hop for their input on the pitch context's own stream;
 * EstimatePitch1 claims that hop when it arrives with the same samples, bin range, estimator and parameters, and otherwise drops it and runs as it
 * always did -- results and state are the same to the bit either way (csrc/abi.hip, tests/test_gpu_pitch_beside_phone.py).  This entry reads the
 * counters: hops claimed / dropped so far (either pointer may be NULL); returns 1 while the context has a partner and gets such hops, 0 if not, -1 on
 * a bad context.  BEATRICE_HIP_NO_SPECULATION=1 in the environment turns the mechanism off. */
int BeatriceHip_PitchSpeculation(Beatrice20rc0_PitchContext1* ctx, long long* claimed, long long* dropped);

/* Several GPUs in one process (a C++ host with one thread per GPU, examples/node_convert.cc; the reference runs many plugin
 * instances per process, src/vst/factory.cc:21).  Every object of this library -- model objects, contexts, batches --
 * lives on ONE device, fixed when it is created: the calling thread's target device, BeatriceHip_SetDevice(ordinal)
 * (thread-local; -1 = follow the thread's current HIP device, the default), and every entry point makes its object's
 * device current for its own duration and restores the caller's, so a thread may own objects on several GPUs and a host
 * framework's own device selection is left alone.  Objects of different devices cannot be combined (a context with a
 * model object of another GPU emits zeros; BeatriceBatch_Create returns an unhealthy batch).  0, or -1 for an ordinal the
 * runtime does not have. */
int BeatriceHip_SetDevice(int ordinal);
int BeatriceHip_GetDevice(void);
int BeatriceBatch_Device(const BeatriceBatch* b);

/* Test support: the packed (two results per instruction) forms of MODEL_SPEC's scalar functions that the kernels use
 * (csrc/spec_math.hip.h) against their scalar definitions, on the device, for ALL 2^32 float32 bit patterns (NaN excluded).
 * which: 0 exp, 1 tanh, 2 gelu, 3 sigmoid.  Returns the number of inputs whose results differ in any bit (0 = identical),
 * *first_bad_bits = the lowest such input (0xffffffff when none); -1 on a HIP failure or an unknown `which`. */
long long BeatriceHip_MathSelfTest(int which, unsigned* first_bad_bits);

/* Test support: one of MODEL_SPEC 2.1's functions, as the device computes it, at n caller-chosen points.  `bits` and `out_bits` are
 * host arrays of n float32 bit patterns.  which: 0 exp, 1 tanh, 2 gelu, 3 sigmoid, 4 log (positive normal arguments), 5 lrelu -- the
 * scalar device functions; 6 exp, 7 tanh, 8 gelu, 9 sigmoid in their packed forms, the points taken in pairs (2p, 2p + 1; an odd
 * count pairs the last point with itself).  Returns 0; -1 on a HIP failure, an unknown `which` or a null array with n > 0. */
int BeatriceHip_MathEval(int which, const uint32_t* bits, size_t n, uint32_t* out_bits);

/* Device-resident parameter blobs, for loading a model on several GPUs from ONE file read.
 * kind: 1 phone extractor, 2 pitch estimator, 3 waveform generator, 4 embedding setter; `model` the matching object.
 * BeatriceHip_ModelBlob returns the object's parameter blob as it sits on the device (already in the kernels' packed
 * layout); with allocate != 0 an object that has not been loaded gets an empty blob of the right size.  The caller
 * moves bytes device to device (e.g. a RCCL broadcast from the rank that called Read*Parameters) and then calls
 * BeatriceHip_ModelBlobReady on the receiving objects.  0 on success, -1 bad argument / nothing to share, -2 HIP failure. */
int BeatriceHip_ModelBlob(int kind, void* model, int allocate, void** d_ptr, size_t* n_bytes);
int BeatriceHip_ModelBlobReady(int kind, void* model);

/* ---------------------------------------------------------------------------------------------------------------------------------------
 * MODES.  A batch is in exactly one of the modes below; the table says which entry point works in which (ok), which is refused with -1
 * (-), and at which hops per step H (BeatriceBatch_CreateBlock) the mode exists.  A refused call changes NOTHING: no drain, no clock, no
 * flag -- tests/test_gpu_mode_matrix.py asks every "-" cell of this table between steps and compares the batch, bit for bit, with one that
 * never asked.  The "ok" cells are the -m gpu parity tests against the oracle.  Settings (BeatriceBatch_Set*, ResetStream, Morph*,
 * SetInputGain / SetOutputGain once a wrapper is configured) work in every mode and apply to the step / call that follows them.
 * The library decides on this table as code: beatrice-vst_amd/csrc/batch_modes.h, held against the test's matrix by tests/test_cpu_mode_table.py.
 *
 *   mode (how it is entered)                                        H           its entry point per step / call
 *   A  in order            (a new batch)                            1 2 4 8     ConvertFrames, ConvertFramesDevice
 *   B  stage pipelining    (EnablePipelining(2..4))                 1 2 4 8     ConvertFrames, ConvertFramesDevice
 *   C  resident I/O        (BindResidentIO)                         1 2 4 8     ConvertFramesDevice(NULL, NULL)
 *   D  tick mode           (C + EnableTickPipeline(1))              1 2 4       ConvertFramesDevice(NULL, NULL)
 *   E  host streaming      (EnableHostStreaming(1))                 1 2 4       StreamFrames / StreamFlush
 *   F  48 kHz blocks around the ticks (BindResidentIO48k)           1 2 4       ConvertBlocks48kDevice(NULL, NULL)
 *   G  resident blocks around the ticks, one set of clocks
 *                          (ConfigureWrapper + BindResidentBlocks)  1 2 4       ProcessBlocksDevice(NULL, NULL, channels, n)
 *   P  ... with clocks per stream
 *                          (ConfigureWrapperRates + BindResidentBlocksRagged)  1   ProcessBlocksRaggedDevice
 *   S  A with the silent-block rule (EnableSilentBlockRule(1))      1           ConvertBlocks48k[Device]
 *
 *   entry point                          A        B     C     D        E     F        G     P     S
 *   ConvertFrames (host buffers)         ok       ok    -     -        -     -        -     -     ok
 *   ConvertFramesDevice(d_in, d_out)     ok       ok    -     -        -     -        -     -     ok
 *   ConvertFramesDevice(NULL, NULL)      ok       ok    ok    ok       -     -        -     -     ok
 *   ConvertBlocks48k, ..Device(ptrs)     ok, H=1  -     -     -        -     -        -     -     ok
 *   ConvertBlocks48kDevice(NULL, NULL)   -        -     -     -        -     ok       -     -     -
 *   ProcessBlocks, ..Device(ptrs)        ok (1)   -     -     -        -     -        -     -     - (1)
 *   ProcessBlocksDevice(NULL, NULL)      -        -     -     -        -     -        ok    -     -
 *   FlushResidentBlocks                  -        -     -     -        -     -        ok    ok    -
 *   ProcessBlocksRagged                  ok (2)   -     -     -        -     -        -     -     - (2)
 *   ProcessBlocksRaggedDevice            -        -     -     -        -     -        -     ok    -
 *   StreamFrames / StreamFlush           -        -     -     -        ok    -        -     -     -
 *   EnableSilentBlockRule(1)             ok, H=1  -     - (7) ok (6)   -     ok (6)   -     -     ok
 *   EnableSilentBlockRule(0)             ok       ok    ok    ok       ok    ok       -     -     ok
 *   SetSilentStreams                     - (3)    -     -     - (3)    -     - (3)    -     -     ok
 *   EnablePipelining(n)                  ok       ok    ok(7) -        -     -        -     -     - (n >= 1)
 *   EnableTickPipeline(1)                -        -     ok(4,7) ok(7)  -     -        -     -     -
 *   EnableTickPipeline(0)                ok       ok    ok    ok       -     -        -     -     ok
 *   EnableHostStreaming(1)               ok (8)   -     -     -        ok    -        -     -     -
 *   BindResidentIO (bind)                ok       ok    ok(7) -        -     -        -     -     -
 *   BindResidentIO (NULL, NULL)          ok       ok    ok    -        -     -        -     -     ok
 *   BindResidentIO48k (bind)             ok (8)   -     -     -        -     ok (5)   -     -     -
 *   BindResidentBlocks (bind)            ok (1)   -     -     -        -     -        ok(5) ok(5) -
 *   BindResidentBlocksRagged (bind)      ok (2)   -     -     -        -     -        ok(5) ok(5) -
 *   Bind...(NULL, NULL) of F / G / P     ok       ok    ok    ok       ok    leaves F leaves G / P      ok
 *   ConfigureWrapper (8)                 ok       ok    ok    ok       ok    ok       -     -     ok
 *   ConfigureWrapperRates                ok, H=1  -     -     -        -     -        -     -     ok
 *   ProfileKernels                       ok       ok    ok    -        -     -        -     -     ok
 *   TimeSteps                            ok       ok    ok    ok       -     -        -     -     ok
 *   TimeTickLaunch                       -        -     -     ok       -     -        -     -     -
 *
 *   (1) once BeatriceBatch_ConfigureWrapper has been called (-1 before); one hop per step for the in-order calls, H = 1 / 2 / 4 for the binding.
 *   (2) once BeatriceBatch_ConfigureWrapperRates has been called (-1 before); one hop per step.
 *   (3) ok once the rule is enabled in that mode (D, F: any H; the flagged streams sit the NEXT step out).
 *   (4) with more resident slots than BeatriceBatch_TickStages() and at most 4096 of them, B <= 4096, H = 1 / 2 / 4.
 *   (6) at H = 2 / 4 a flagged stream sits a WHOLE step (its H hops / its H 48 kHz blocks) out: the caller flags a stream whose blocks of the step are ALL silent.  One
 *       silent block among sounding ones of the same step cannot be skipped there (it is converted as the sounding ones are) -- the shell's per-block rule needs one hop per step.
 *   (5) a bind call on a batch that is already in F / G / P first LEAVES that mode exactly as that mode's unbind call does, then binds anew: by the A column, as on
 *       any batch.  G / P: drained, the any-rate wrapper restarted (BeatriceBatch_BindResidentBlocks).  F: drained, and NOTHING restarted -- the 48 kHz wrapper's
 *       state carries over (BeatriceBatch_BindResidentIO48k).  tests/test_gpu_wrapper_walk.py walks one batch across these transitions against the oracle.
 *   (7) a rule enabled in D / F stays on when the batch leaves tick mode after BeatriceBatch_ConfigureWrapperRates (which keeps the rule's buffers): while it is on,
 *       these calls are refused in C (and a second EnableTickPipeline(1) in D), and EnableSilentBlockRule(1) returns 0.  EnableSilentBlockRule(0) clears it.
 *   (8) H = 1 / 2 / 4: -1 on a batch of eight hops per step.
 *   (9) not rows of this table, because they are settings: BeatriceBatch_SetStreamRate, RestartStreamWrapper, StreamRate, WrapperBlobBytes,
 *       ExportStreamWrappers and ImportStreamWrappers work exactly where the row "ProcessBlocksRagged" says ok -- A and S, one hop per step,
 *       once BeatriceBatch_ConfigureWrapperRates has been called, nothing bound -- and are refused (-1, 0.0 or 0; nothing changes) everywhere else.
 *   (10) not rows of this table either: BeatriceBatch_ScanSilentBlocksBegin, ScanSilentBlocksEnd and ScanSilentBlocks are questions about the CALLER's
 *       device memory and work in every mode; BeatriceBatch_ScanBoundBlocks48k works exactly where the row "ConvertBlocks48kDevice(NULL, NULL)" says ok -- F --
 *       and is refused (-1) everywhere else.  No scan call drains anything, moves a clock, or changes a flag or setting of the batch.
 *   (11) not rows of this table either, because they are settings: BeatriceBatch_SetStreamRateInFlight, RestartStreamInFlight and BoundStreamRate work
 *       exactly where the row "ProcessBlocksRaggedDevice" says ok -- P -- and are refused (-1, the getter 0.0; nothing changes) everywhere else.  The six
 *       calls of (9), BeatriceBatch_ResetStream and BeatriceBatch_ResetStreamInFlight behave in P as before: the six are refused, the two drain.
 *   (12) not rows of this table either, because they are settings: BeatriceBatch_StreamQuiescent, ExportStreamsInFlight, ImportStreamsInFlight and
 *       MoveStreamsInFlight work in plain tick mode -- D, H = 1 / 2 / 4, with or without the silent-block rule -- and are refused (-1; nothing changes)
 *       in A, B, C, E, F, G, P and S, where BeatriceBatch_ExportStreams / ImportStreams remain the way.  F and P keep wrapper state whose output halves
 *       run a tick or `delay` calls later: a stream at rest in the ticks is not yet at rest there.  P is served by the calls of (13), which hold that second
 *       quiescence rule; F is served by the calls of (14), which hold its own.
 *   (13) not rows of this table either, because they are settings: BeatriceBatch_BoundStreamQuiescent, MoveBoundStreamsInFlight, ExportBoundStreamsInFlight,
 *       ImportBoundStreamsInFlight and BoundWrapperBlobBytes work exactly where the row "ProcessBlocksRaggedDevice" says ok -- P -- and are refused (-1, the
 *       size 0; nothing changes) everywhere else, D included: there the calls of (12) are the way.
 *   (14) not rows of this table either, because they are settings: BeatriceBatch_Stream48kQuiescent, ExportStreams48kInFlight, ImportStreams48kInFlight and
 *       MoveStreams48kInFlight work exactly where the row "ConvertBlocks48kDevice(NULL, NULL)" says ok -- F, H = 1 / 2 / 4, with or without the silent-block
 *       rule -- and are refused (-1; nothing changes) in A, B, C, D, E, G, P and S; a move between a D batch and an F batch is refused by both families.
 *       Their quiescence rule is that of (12) plus ONE LAUNCH: the wrapper's output half of a step runs in the wrapper launch of the call after the
 *       step's last tick (or in the flush of a drain), and only behind it is the stream's 48 kHz wrapper state at rest.
 *
 * Environment variables the library reads: BEATRICE_HIP_DEBUG (print HIP errors to stderr), BEATRICE_HIP_CUMASK ("lo-hi;lo-hi;..": CU masks
 * of the stage-pipelining streams), BEATRICE_HIP_HOP_GRAPH (the 1-stream calls replayed as hipGraphs), BEATRICE_HIP_NO_SPECULATION (no pitch hop beside
 * the phone call, BeatriceHip_PitchSpeculation above).  Nothing else: the A/B switches of
 * profiles/r0*_notes.md exist in measurement builds only (tools/debug/build_variant.sh <name> -DBEATRICE_HIP_MEASUREMENT_BUILD).
 * --------------------------------------------------------------------------------------------------------------------------------------- */
/* n_streams concurrent streams; speaker tables may hold up to max_speakers entries
 * (n_speakers + 1 when the caller keeps the reference's extra "morph" slot). */
BeatriceBatch* BeatriceBatch_Create(const Beatrice20rc0_PhoneExtractor* phone, const Beatrice20rc0_PitchEstimator* pitch,
                                    const Beatrice20rc0_WaveformGenerator* wave, const Beatrice20rc0_EmbeddingSetter* embed,
                                    int n_streams, int max_speakers);
/* Block mode for offline / utterance conversion: every step converts `hops_per_step` (1, 2, 4 or 8)
 * consecutive hops of every stream, so the per-launch cost of the kernel chain is shared by H hops.
 * Results are bit-identical to H single-hop steps (the recurrent layers still advance hop by hop
 * inside the step; a pending speaker switch still installs one K/V block per hop).  Buffers become
 * in [B][H*160], out [B][H*240].  hops_per_step = 1 is BeatriceBatch_Create (10 ms real-time steps). */
BeatriceBatch* BeatriceBatch_CreateBlock(const Beatrice20rc0_PhoneExtractor* phone, const Beatrice20rc0_PitchEstimator* pitch,
                                         const Beatrice20rc0_WaveformGenerator* wave, const Beatrice20rc0_EmbeddingSetter* embed,
                                         int n_streams, int max_speakers, int hops_per_step);
void BeatriceBatch_Destroy(BeatriceBatch* b);
int BeatriceBatch_IsHealthy(const BeatriceBatch* b);
int BeatriceBatch_InjectTeamTimeout(BeatriceBatch* b);   /* test hook, see BeatriceHip_InjectTeamTimeout */
/* Test hook: where the step counter starts.  Every activation ring is addressed by (step counter mod its slot count); the counter -- on the
 * device and in the host's mirror -- wraps to 0 after BEATRICE_HIP_STEP_WRAP - 1 (lcm(1..17): every slot count divides it; 34 hours of 10 ms
 * steps), and a test cannot feed twelve million steps to get there.  BeatriceBatch_SetStepCounter sets the host mirror and the device's
 * copy on a FRESH batch only: one that has not taken a step yet, has no binding (resident I/O, 48 kHz or any-rate blocks, host streaming)
 * and is outside tick mode.  The rings of a fresh batch are all zeros, so a batch started at counter c computes exactly what one started
 * at 0 computes -- only the slots its history lands in differ (tests/test_gpu_counter_wrap.py).  -1 and no change: a counter outside
 * [0, BEATRICE_HIP_STEP_WRAP), a batch that has taken a step, a binding, tick mode.  It adds nothing to any step and is not a mode entry
 * point (no row in the MODES table).  BeatriceBatch_StepCounter returns the host mirror: the counter of the NEXT step (-1: no batch). */
#define BEATRICE_HIP_STEP_WRAP 12252240
int BeatriceBatch_SetStepCounter(BeatriceBatch* b, int counter);
int BeatriceBatch_StepCounter(const BeatriceBatch* b);
int BeatriceBatch_NumStreams(const BeatriceBatch* b);
int BeatriceBatch_HopsPerStep(const BeatriceBatch* b);
/* bytes of per-stream activation history (all rings of all three modules) held for the n_streams streams */
size_t BeatriceBatch_StateBytes(const BeatriceBatch* b);

/* Upload the four caller-owned tables exactly as Beatrice20rc0_ReadSpeakerEmbeddings fills them
 * ([n][512][128], [n][256], [9][256], [n][384][128]); projects additive/formant vectors and the
 * K/V of every (speaker, block) once, so that later speaker switches are index changes. */
int BeatriceBatch_SetSpeakerTables(BeatriceBatch* b, int n_speakers, const float* codebooks, const float* additive,
                                   const float* formant, const float* key_value);
/* The same tables filled device to device: d_ptrs[4] / n_bytes[4] receive the raw device tables (codebooks, additive,
 * formant, key_value; sized for max_speakers entries); after writing n entries into them (e.g. by a broadcast),
 * BeatriceBatch_ProjectSpeakerTables(b, n) runs the projections that BeatriceBatch_SetSpeakerTables runs after its upload. */
int BeatriceBatch_SpeakerTablesDevice(BeatriceBatch* b, void** d_ptrs, size_t* n_bytes);
int BeatriceBatch_ProjectSpeakerTables(BeatriceBatch* b, int n_speakers);
/* Replace one table entry (e.g. the morph slot after a spherical average on the host). */
int BeatriceBatch_UpdateSpeaker(BeatriceBatch* b, int speaker, const float* codebook, const float* additive,
                                const float* key_value);

/* Speaker morphing on the device (reference processor_core_2.cc:51-177, 498-532; spherical_average.h):
 * table entry `slot` (n_weights <= slot < max_speakers, e.g. the reference's extra entry n_speakers)
 * becomes the morph of the real speakers 0..n_weights-1 under `weights`: weights below 0.01 are dropped and
 * the eight largest kept (as the reference prepares them), the additive embedding and the 384 key/value
 * embeddings are weighted spherical means (one wavefront each, one launch), projections are refreshed.
 * Streams whose target speaker is `slot` then (a) re-install the entry's key/value blocks one per hop and
 * (b) use, at every step, the codebook of ONE real speaker drawn with the weights as odds from a
 * std::mt19937 seeded with `seed` the first time (the reference seeds once, from std::random_device).  Unlike the reference
 * host, which spreads the means over five hops to bound its CPU time, the new embeddings are complete
 * when the call returns.  Agreement with the host computation: float rounding (<= 1e-5), not bit-exact. */
int BeatriceBatch_MorphSpeaker(BeatriceBatch* b, int slot, const float* weights, int n_weights, unsigned seed);
/* The lottery engine is per stream, as the reference's is per plugin instance (processor_core_2.h:48,145), and like the
 * reference's it is seeded ONCE: the first BeatriceBatch_MorphSpeaker of a batch's life seeds stream s with
 * std::mt19937(seed + s); later calls (weights moving, other entries) leave every engine running, so a caller that moves
 * morph weights every step still gets a per-hop lottery and a morph on one entry does not restart the draws of streams on
 * another.  BeatriceBatch_SeedLottery re-seeds one stream (or all, -1) with std::mt19937(seed) at any time -- e.g. from the
 * stream's global identity when streams are sharded over batches or GPUs, so that a stream's draws do not depend on where it
 * runs -- and a later BeatriceBatch_MorphSpeaker keeps those engines.  One draw per hop, also in block mode.
 * The entry's key/value projections are replaced in place by BeatriceBatch_MorphSpeaker: streams already on the entry
 * see all four blocks change at that step (the reference, which computes the means over four hops on the audio
 * thread, installs them one block per hop). */
int BeatriceBatch_SeedLottery(BeatriceBatch* b, int stream, unsigned seed);
/* The reference's own timeline of a weight change for streams that are already morphing (processor_core_2.cc:51-177,
 * 144-172): on the next hop h0 the new additive embedding and the new lottery odds are in force, the OLD key/value blocks keep
 * playing over h0 .. h0+3 (the reference computes a quarter of the key/value means per hop), the new ones are installed one
 * block per hop over h0+4 .. h0+7.  The new morph is computed into ANOTHER table entry `slot` (same rules as
 * BeatriceBatch_MorphSpeaker) and every stream whose target speaker is `from_slot` moves to it on that timeline.  -3: some
 * stream still has key/value blocks of `slot` installed (rotate over three entries when the weights move faster than every
 * eight hops; as in the reference, new blocks are then never installed while the weights keep moving: each call restarts the
 * four-hop wait). */
int BeatriceBatch_MorphSpeakerStaged(BeatriceBatch* b, int slot, int from_slot, const float* weights, int n_weights, unsigned seed);
/* The same for n table entries in ONE call, and without the drain where the pipeline allows it.  For every i < n:
 *   from_slots[i] >= 0:  exactly BeatriceBatch_MorphSpeakerStaged(b, slots[i], from_slots[i], weights + i * n_weights, n_weights, seed);
 *   from_slots[i] == -1: exactly BeatriceBatch_MorphSpeaker on an entry no stream is on -- the entry is computed, no stream moves.
 * Same weight preparation, same lottery rule (seeded once per batch life, seed + stream), same timeline for the streams that move
 * (additive embedding and odds on the next hop, a four-hop wait, then one key/value block per hop).  All n * 385 spherical means run in
 * one launch and all projections in a second one (results bit-identical to the single-entry calls; a morph entry's codebook is not
 * touched).  In plain tick mode (D: H = 1, 2, 4, with or without the silent-block rule), in host streaming (E) and in the wrapper modes
 * around the ticks (F: BindResidentIO48k, G: BindResidentBlocks, P: BindResidentBlocksRagged) nothing drains and nothing synchronises:
 * the two launches go onto the batch's stream in front of the next tick and the call returns -- no tick and no wrapper launch is made,
 * BeatriceBatch_TicksLaunched, BeatriceBatch_ResidentBlocksOwed and the binding's call counter stand; in every other mode it drains as
 * the single-entry calls do.  It is a setting, not a mode entry point (no row in the MODES table).
 * In F, G and P "the next hop" of the timeline is the first hop fired by the call that follows: at H = 2 or 4 in F the first block of the
 * next step; in G the first hop of the next step FED -- a hop that has already fired into a step still filling belongs to that step, and
 * the step takes the settings in force when its last hop fires and it is fed, which is what BeatriceBatch_SetTargetSpeaker does there.
 * CONTRACT CHANGE in F, G and P: until now the call drained there, so an entry busy only by rule (b) of BeatriceBatch_SpeakerEntryBusy
 * was free by the time the call looked; now it is refused with -3 and nothing changes, as in D and E.  The single-entry calls
 * (BeatriceBatch_MorphSpeaker, MorphSpeakerStaged, UpdateSpeaker) keep draining in every mode.
 * All or nothing.  -1 and no change (no launch, no drain, no seeding): n < 1 or n > max_speakers; the n_weights rules of
 * BeatriceBatch_MorphSpeaker; a slot outside [n_weights, max_speakers); a slot twice; a from_slot twice; a from_slot out of range,
 * equal to its own slot or to another pair's slot.  -3 and no change: some slot is busy (BeatriceBatch_SpeakerEntryBusy).
 * What rotation costs: an entry stays busy until the streams that left it have installed their new key/value blocks (eight hops
 * after the call that moved them, later if the weights move again first) AND, in D, E, F, G and P, until the last step that named it has
 * left the pipeline, BeatriceBatch_TickStages() ticks on.  A stream whose weights move every step therefore needs about TickStages() + 2
 * entries to rotate over, at about 3.1 MB of projected tables per entry (four blocks, K and V, in two layouts).  Rewriting an entry
 * that streams are on is not offered; a caller's own tables go into free entries without a drain through
 * BeatriceBatch_InstallSpeakersInFlight. */
int BeatriceBatch_MorphSpeakersInFlight(BeatriceBatch* b, int n, const int* slots, const int* from_slots,
                                        const float* weights /* [n][n_weights] */, int n_weights, unsigned seed);
/* 1: table entry `entry` is busy, 0: free to be a slot of BeatriceBatch_MorphSpeakersInFlight or an entry of
 * BeatriceBatch_InstallSpeakersInFlight, -1: bad argument.  Busy means (a) some
 * stream's current settings name it -- as target, additive or codebook speaker, or as an installed or pending key/value entry -- or
 * (b) in D, E, F, G and P, a step that named it may still be inside the pipeline: that step's later stages read the entry's additive row
 * and key/value tables (csrc/speaker_entry_plan.h holds the rule).  CONTRACT CHANGE: in F, G and P the answer used to be 0 here, because
 * the two in-flight calls drained in those modes; they no longer do, and refuse such an entry with -3.  The ticks count as they are
 * launched: in P a call launches one tick per FIFO piece in which some stream fires (one idle tick if none), in G at H = 2 or 4 only
 * when a step is full -- and there an entry whose last name goes while a step is filling (a hop has fired into it, it has not been fed)
 * stays busy until that step has been fed and has left the pipeline, across BeatriceBatch_Synchronize too; it is released when
 * BeatriceBatch_FlushResidentBlocks or an unbind drops the filling step.  The bookkeeping is one stamp per entry and errs on the safe
 * side: when the entry's last naming setting goes, it stays busy until BeatriceBatch_TickStages() ticks have been launched counting from
 * the last step the BATCH had been fed at that moment (when it was a key/value install at several hops per step that took the last name
 * away: from the step that installs, whose early hops still run on the blocks installed before -- also when that step's codebook draw,
 * made behind the install, is what takes the last name: in D and E at H = 2 and 4 this is one tick later than the stamp used to say,
 * which counted from the step before), or until the pipeline is drained.  For a stream that takes part in every step that is the
 * last step that named the entry; for a stream that changes its settings while it sits out (BeatriceBatch_SetSilentStreams), or that
 * is imported over, it is later than that -- by the steps the batch was fed without it -- or (c) an active morph entry that is
 * itself busy by (a) or (b) lists it with positive odds (with any odds when all of the morph's weights were dropped: the lottery then
 * draws from all of its speakers): a step of a stream on that morph may have drawn the entry's codebook.  Host bookkeeping; launches
 * nothing. */
int BeatriceBatch_SpeakerEntryBusy(const BeatriceBatch* b, int entry);
/* New voices into a running batch: for every i < n the effect on every later step is exactly that of
 * BeatriceBatch_UpdateSpeaker(b, entries[i], codebooks + i * 512 * 128, additive + i * 256, key_value + i * 384 * 128) with all three
 * tables given -- the raw tables, the transposed codebook with its norms, the additive projection and the key/value projections of all
 * four blocks hold the same bits, the table grows to cover the entry, an active morph on the entry ends.  No stream moves: point streams
 * at the new entries afterwards with BeatriceBatch_SetTargetSpeaker(s).  All three tables are required (NULL: -1), unlike
 * BeatriceBatch_UpdateSpeaker's optional ones.
 * Two launches per call whatever n is (all tables from staging, all projections).  In plain tick mode (D: H = 1, 2, 4, with or without
 * the silent-block rule), in host streaming (E) and in the wrapper modes around the ticks (F, G, P) nothing drains and nothing
 * synchronises: the launches go onto the batch's stream in front of the next tick and the call returns -- no tick and no wrapper launch
 * is made, BeatriceBatch_TicksLaunched, BeatriceBatch_ResidentBlocksOwed and the binding's call counter stand; in every other mode it
 * drains first and waits for its launches, as the single-entry call does.  It is a setting, not a mode entry point (no row in the MODES
 * table).  CONTRACT CHANGE in F, G and P: the call used to drain there and so succeeded on an entry busy only by rule (b) of
 * BeatriceBatch_SpeakerEntryBusy; now it returns -3 and changes nothing, as in D and E.
 * The caller's arrays may be reused as soon as the call returns: the call copies them into pinned staging on the calling thread, about
 * 449 KB per entry (tens of microseconds each).  The staging is a ring of 4 calls x BeatriceBatch_MaxInstallEntries() entries, allocated
 * by the first call (29 MB of pinned memory at the cap of 16); a fifth call waits only if the device has not yet run the first one's
 * launches.
 * All or nothing.  -1 and no change (no launch, no drain, nothing staged): n < 1 or n > BeatriceBatch_MaxInstallEntries(b); a NULL
 * pointer; an entry outside [0, max_speakers); an entry twice.  -3 and no change: some entry is busy (BeatriceBatch_SpeakerEntryBusy).
 * -2: HIP or allocation failure. */
int BeatriceBatch_InstallSpeakersInFlight(BeatriceBatch* b, int n, const int* entries, const float* codebooks /* [n][512][128] */,
                                          const float* additive /* [n][256] */, const float* key_value /* [n][384][128] */);
/* The most entries one BeatriceBatch_InstallSpeakersInFlight call takes: min(16, max_speakers). */
int BeatriceBatch_MaxInstallEntries(const BeatriceBatch* b);
/* Raw embeddings of a table entry as currently held on the device: additive [256], key_value [384][128]. */
int BeatriceBatch_GetSpeakerEmbeddings(BeatriceBatch* b, int speaker, float* additive, float* key_value);

int BeatriceBatch_SetTargetSpeaker(BeatriceBatch* b, int stream, int speaker);
/* n (stream, speaker) pairs at once (the same effect as n calls of BeatriceBatch_SetTargetSpeaker, processor_core_2.cc:431-466 per
 * stream; all or nothing: -1 and no change when any pair is out of range). */
int BeatriceBatch_SetTargetSpeakers(BeatriceBatch* b, int n, const int* streams, const int* speakers);
int BeatriceBatch_FlushSpeaker(BeatriceBatch* b, int stream); /* install all pending K/V blocks now */
int BeatriceBatch_SetFormantShift(BeatriceBatch* b, int stream, double formant_shift);
int BeatriceBatch_SetVQNumNeighbors(BeatriceBatch* b, int stream, int k);
int BeatriceBatch_SetMinSourcePitch(BeatriceBatch* b, int stream, double midi_note);
int BeatriceBatch_SetMaxSourcePitch(BeatriceBatch* b, int stream, double midi_note);
int BeatriceBatch_SetPitchShift(BeatriceBatch* b, int stream, double semitones);
int BeatriceBatch_SetAverageSourcePitch(BeatriceBatch* b, int stream, double midi_note);
int BeatriceBatch_SetIntonationIntensity(BeatriceBatch* b, int stream, double v);
int BeatriceBatch_SetPitchCorrection(BeatriceBatch* b, int stream, double v);
int BeatriceBatch_SetPitchCorrectionType(BeatriceBatch* b, int stream, int type);
int BeatriceBatch_ResetStream(BeatriceBatch* b, int stream);
/* The same reset as a per-stream SETTING (stream = -1: every stream): the next step fed that the stream takes part in is the first step
 * of a new stream.  The effect on that step and all later ones is exactly that of BeatriceBatch_ResetStream followed by that step: all
 * activation history reads as zeros, the pitch head's previous bin is 0, all four key/value blocks of the target speaker are installed
 * at that step (BeatriceBatch_FlushSpeaker; the target of THAT step: a BeatriceBatch_SetTargetSpeaker made between the call and the step
 * does not install one block per hop behind the reset), every other per-stream setting is kept, the codebook lottery's engine is untouched.  Steps of
 * the stream already inside the pipeline finish on the old state and land in their slots unchanged.  It is not a mode entry point (no row
 * in the MODES table) and works in every mode: in plain tick mode (D: H = 1, 2, 4, with or without the silent-block rule), in host
 * streaming (E) and around the resident 48 kHz blocks (F: H = 1, 2, 4, with or without the rule) nothing drains and nothing synchronises
 * -- the call launches nothing, it is host bookkeeping that applies "to the step that follows" like every other setting, and a stream that
 * sits the next step(s) out is reset at its next present step; in every other mode (A, B, C, S, G, P) it IS BeatriceBatch_ResetStream,
 * with whatever drain that does there.  In F the 48 kHz wrapper's state of the stream starts over with the model's: the blocks of the
 * steps already inside come out behind the old wrapper state, unchanged, and the block of that step is the first block of a new stream
 * behind a new wrapper (at H = 2 / 4 the first block of that step).  Range checks and return codes as for BeatriceBatch_ResetStream.
 * BeatriceBatch_Synchronize, BeatriceBatch_EnableTickPipeline(b, 0), BeatriceBatch_StreamFlush, BeatriceBatch_BindResidentIO48k(NULL,
 * NULL) and a re-bind may be called while a reset is still travelling: the drain ticks, and in F the flush of the last 48 kHz block,
 * carry it to the end. */
int BeatriceBatch_ResetStreamInFlight(BeatriceBatch* b, int stream);
/* Tick launches since tick mode was entered (fill and drain ticks included); 0 outside tick mode. */
long long BeatriceBatch_TicksLaunched(const BeatriceBatch* b);

/* A stream moves from one batch into another WITH its state (a larger batch when load rises, the batch on the GPU that holds its voice,
 * the last live streams of a nearly idle batch): after BeatriceBatch_ExportStreams(X, s) and BeatriceBatch_ImportStreams(Y, t), the next
 * step of stream t of Y is bit for bit the step stream s of X would have run next on the same input, and so is every step after it.  X
 * is not changed by the export; no other stream of Y is changed by the import.
 * A blob holds exactly what BeatriceBatch_ResetStream clears, plus the stream's settings.  State: the stream's part of every activation
 * ring of the three modules, the pitch head's previous bin, the 48 kHz wrapper's history (BeatriceBatch_ConvertBlocks48k*,
 * BeatriceBatch_BindResidentIO48k).  Settings: target, additive and codebook speaker, the installed key/value entries and how many of a
 * pending switch are still to come (they go on installing one per hop in the destination), formant shift, VQ neighbours, pitch range and
 * pitch parameters, and the stream's codebook-lottery engine, which continues its sequence.  A header names the hops per step, the source
 * batch's step counter and the layout of every ring.  NOT in a blob, because it belongs to the slot and BeatriceBatch_ResetStream does
 * not restart it either: the any-rate wrapper's per-stream state (BeatriceBatch_ProcessBlocks*, BeatriceBatch_BindResidentBlocks*: the
 * resampler histories, the 480-sample FIFO, the gain clocks, the per-stream rate clocks).  For a batch with clocks per stream that state
 * travels as a second token of its own: BeatriceBatch_ExportStreamWrappers / BeatriceBatch_ImportStreamWrappers, below.
 * A blob is a short-lived token between two batches of the SAME library build with the same hops per step, not a storage format:
 * BeatriceBatch_ImportStreams refuses whatever it does not recognise and attempts no compatibility.  Between processes it is plain bytes.
 * Both calls work in every mode and are settings, not mode entry points (no row in the MODES table).  Both drain as
 * BeatriceBatch_ResetStream does, after which every stream stands at the batch's one step counter.  Export then gathers the n streams in
 * one launch per 16 streams and waits.  Import validates EVERY blob first, then uploads and scatters in one launch per 16 streams: every
 * ring with more than one step slot is turned by (destination counter - source counter) mod its slot count on the way in.  It replaces
 * the destination streams' settings and lottery engines -- the next step takes them to the device like any other changed setting -- and
 * cancels a BeatriceBatch_ResetStreamInFlight still waiting on a destination stream.
 * entry_map: every speaker-table index of a blob goes through it (index i becomes entry_map[i]), so the destination may hold the same
 * voices at other entries; NULL, 0 keeps the indices.  That the entries named hold the same tables as in the source -- for a morph entry
 * the same active morph with the same weights -- is the caller's promise; nothing checks it.
 * All or nothing.  -1 and no change (no drain, no launch, nothing staged): n < 1 or n > the batch's streams; a NULL pointer (entry_map
 * NULL with n_map != 0 included); a stream out of range or named twice; on import a blob with a bad magic word, version or size, other
 * hops per step than the batch's, a ring layout that does not match, settings out of their ranges, an index outside entry_map (without
 * a map: outside the table's capacity), or a mapped index outside [0, n_speakers) of the destination.  -3 and no change: export of a
 * stream with a BeatriceBatch_ResetStreamInFlight pending that no step has taken yet.  -2: HIP or allocation failure. */
size_t BeatriceBatch_StreamBlobBytes(const BeatriceBatch* b);   /* bytes of ONE stream's blob; the same for every stream of b */
int BeatriceBatch_ExportStreams(BeatriceBatch* b, int n, const int* streams, void* blobs /* host, n * StreamBlobBytes(b) */);
int BeatriceBatch_ImportStreams(BeatriceBatch* b, int n, const int* streams, const void* blobs /* host, n blobs */,
                                const int* entry_map, int n_map /* NULL, 0: speaker-table indices are kept as they are */);

/* The same move between batches that BOTH GO ON TICKING: nothing drains, no tick is launched, no other stream of either batch is
 * disturbed.  MODES footnote (12): plain tick mode (D), H = 1, 2 or 4, with or without the silent-block rule; refused with -1 everywhere
 * else, where the drained calls above remain the way.
 * What makes it possible is that the stream is AT REST.  BeatriceBatch_StreamQuiescent(b, s) is 1 when no step stream s took part in is
 * inside the pipeline: either it has taken part in no step since the last drained point (BeatriceBatch_Synchronize, entering tick
 * mode), or at least BeatriceBatch_TickStages(b) ticks have been launched since, and counting, the tick that fed its last present step
 * -- the stream sat out (BeatriceBatch_SetSilentStreams), or nothing was fed, for TickStages - 1 further ticks.  0 otherwise; -1 for a
 * stream out of range or outside D.  Without the silent-block rule every stream takes part in every step, and streams are at rest only
 * while the pipeline is empty.  A stream at rest stands at its OWN step counter, which lags the batch's by the steps it sat out.
 * BeatriceBatch_ExportStreamsInFlight writes the SAME blobs as BeatriceBatch_ExportStreams (format, version word and
 * BeatriceBatch_StreamBlobBytes unchanged; a blob of either export is taken by either import); the counter in a blob's header is the
 * stream's own.  The gather and the copy to the host are enqueued on the batch's stream behind the ticks already enqueued, and the call
 * waits for its own copy alone, on an event recorded behind it.  It therefore WAITS FOR THE TICKS IN FRONT OF IT: it is a scheduler's
 * call, not one for an audio thread.  BeatriceBatch_TicksLaunched, every stream's counter and BeatriceBatch_ResidentBlocksOwed read the
 * same before and after, and the source is unchanged: fed again, the stream goes on as if nothing had been asked.
 * BeatriceBatch_ImportStreamsInFlight validates every blob exactly as BeatriceBatch_ImportStreams does, then enqueues the upload from
 * pinned staging and the scatter in front of the next tick and returns WITHOUT waiting.  Staging is a ring of two calls: a third call
 * waits only if the device has not yet run the first one's scatter.  Every ring with more than one slot is turned by (the DESTINATION
 * STREAM's own counter - the blob's counter) mod its slot count; the destination stream's counter does not change.  Settings and lottery
 * engine are replaced on the host and reach the device with the next step fed, like any setting changed between two ticks (a stream that
 * brings the first or takes away the last use of the k-NN stage drains there, as BeatriceBatch_SetVQNumNeighbors does).  A
 * BeatriceBatch_ResetStreamInFlight still waiting on the slot is cancelled.
 * BeatriceBatch_MoveStreamsInFlight is both at once for two batches ON ONE DEVICE with the same hops per step and ring layout: one
 * launch per 16 streams copies ring to ring, turned on the way; no staging buffer, no trip over the host link, no host wait.  The
 * settings move host to host with the checks of the blob path.  If the batches run on different HIP streams the launch, on the
 * destination's, waits for an event on the source's, and the source's stream waits for an event behind the launch, so that a later
 * reset, import or present step of the source slot cannot overtake the read; with one shared stream (BeatriceBatch_SetStream) no event
 * is needed.  The source is unchanged: BeatriceBatch_ResetStreamInFlight turns the slot over afterwards.
 * All or nothing, and a refused call changes nothing (no launch, no staging, no clock, no flag), in this order.  -1: n < 1 or n > the
 * batch's streams; a NULL pointer (entry_map NULL with n_map != 0 and the reverse); a stream out of range or named twice; a mode other
 * than D; on import everything BeatriceBatch_ImportStreams refuses; for a move also src == dst, a NULL batch, different devices, hops
 * per step or layouts.  -3: a stream named, source or destination, is not quiescent; on export and move also a source stream with a
 * BeatriceBatch_ResetStreamInFlight pending that no step has taken yet.  -2: HIP or allocation failure. */
int BeatriceBatch_StreamQuiescent(const BeatriceBatch* b, int stream);
int BeatriceBatch_ExportStreamsInFlight(BeatriceBatch* b, int n, const int* streams, void* blobs /* host, n * StreamBlobBytes(b) */);
int BeatriceBatch_ImportStreamsInFlight(BeatriceBatch* b, int n, const int* streams, const void* blobs /* host, n blobs */,
                                        const int* entry_map, int n_map);
int BeatriceBatch_MoveStreamsInFlight(BeatriceBatch* src, BeatriceBatch* dst, int n, const int* src_streams, const int* dst_streams,
                                      const int* entry_map, int n_map);

/* The same four calls for batches that BOTH GO ON CONVERTING RESIDENT 48 kHz BLOCKS (BeatriceBatch_BindResidentIO48k, mode F).  MODES
 * footnote (14): F, H = 1, 2 or 4, with or without the silent-block rule; refused with -1 everywhere else, D included -- and the four
 * calls above go on refusing F, so a move between a D batch and an F batch is refused by both families.
 * The contract is that of the calls above, word for word -- the same blobs (which already hold the 48 kHz wrapper's state of the
 * stream), the blob's counter the stream's own, every ring turned by the destination stream's own counter minus the blob's, staging a
 * ring of two import calls, the export waiting for its own copy alone, the move one launch per 16 streams on the destination's stream
 * fenced by events against the source's, settings and lottery engine host to host with the entry_map checks, a pending
 * BeatriceBatch_ResetStreamInFlight refusing a source with -3 and cancelled on a destination, the same order of refusals,
 * BeatriceBatch_TicksLaunched and every counter unchanged -- with ONE difference: when a stream is at rest.
 * Around the ticks of F stands the 48 kHz wrapper, and the output half of a step runs ONE LAUNCH LATE: the 48 kHz block of the step fed
 * by call T is produced by the wrapper launch of call T + BeatriceBatch_TickStages(b), or by the flush of a drain that gets there first,
 * and that launch reads and writes the stream's wrapper state.  BeatriceBatch_Stream48kQuiescent(b, s) is 1 when stream s has taken part
 * in no step since the last drained point, or when that launch has been enqueued for its last present step: TickStages + 1 calls have
 * been made since, and counting, the call that fed it -- the stream sat out for TickStages further calls, one more than in D.  From then
 * on no launch reads or writes the stream's rings, its previous bin or its wrapper state until it is fed again: the input half of an
 * absent stream returns early, its output half copies its own down-mix.  A BeatriceBatch_ResetStreamInFlight that is still travelling
 * implies that the stream is not at rest.  0 otherwise; -1 for a stream out of range or outside F.
 * The wrapper state is mono: the two bindings' channel counts and slot counts need not agree; hops per step and ring layout must, as in
 * D.  After a move the stream's next block, written by the caller into the destination binding's next slot, comes out as the block the
 * source would have produced -- the first one included, whose 48 kHz samples are the model output that travelled in the wrapper's FIFO. */
int BeatriceBatch_Stream48kQuiescent(const BeatriceBatch* b, int stream);
int BeatriceBatch_ExportStreams48kInFlight(BeatriceBatch* b, int n, const int* streams, void* blobs /* host, n * StreamBlobBytes(b) */);
int BeatriceBatch_ImportStreams48kInFlight(BeatriceBatch* b, int n, const int* streams, const void* blobs /* host, n blobs */,
                                           const int* entry_map, int n_map);
int BeatriceBatch_MoveStreams48kInFlight(BeatriceBatch* src, BeatriceBatch* dst, int n, const int* src_streams, const int* dst_streams,
                                         const int* entry_map, int n_map);

/* One step (H hops, H = 1 unless created with BeatriceBatch_CreateBlock) for every stream.
 * Host variant: in [B][H*160] @16 kHz, out [B][H*240] @24 kHz, synchronous.
 * Device variant: pointers are device memory, work is enqueued on the batch's HIP stream and the
 * call returns without waiting (BeatriceBatch_Synchronize to wait). */
int BeatriceBatch_ConvertFrames(BeatriceBatch* b, const float* in, float* out);
int BeatriceBatch_ConvertFramesDevice(BeatriceBatch* b, const float* d_in, float* d_out);
int BeatriceBatch_Synchronize(BeatriceBatch* b);

/* Resident I/O (utterances or stream buffers that already live on the device): bind
 *   d_in [n_slots][B][H*160] and d_out [n_slots][B][H*240];
 * afterwards every BeatriceBatch_ConvertFramesDevice(b, NULL, NULL) converts the next slot (k mod n_slots) in
 * place -- no per-step copy, same results.  While bound, the host-buffer and 48 kHz entry points return -1.
 * NULL, NULL unbinds.  Re-binding restarts at slot 0. */
int BeatriceBatch_BindResidentIO(BeatriceBatch* b, const float* d_in, float* d_out, int n_slots);

/* 48 kHz host-rate blocks with the reference's wrapper ON THE DEVICE (BASELINE.json configs[4]):
 * per call one 10 ms block of every stream, planar float, `channels` = 1 or 2:
 *   in [B][channels][480] @48 kHz -> out [B][channels][480] @48 kHz.
 * Performs, per stream, what the reference host does around the model for a 48 kHz host at 0 dB gains:
 * stereo downmix (L+R)*0.5 (reference src/vst/processor.cc:183-192), 31-tap low-pass + keep every 3rd
 * sample (src/common/resample.h:130-159, 384-386), the 480-sample FIFO (:343-363, i.e. +10 ms), the
 * model hop, zero-stuffing x2 (:390-393), 32-tap low-pass (:168-206), copy to every output channel
 * (processor.cc:221-225).  Bit-identical to the host chain.  Other host rates and non-zero gains: use
 * the C++ host layer (beatrice-vst_amd/host).  Per 10 ms block only: returns -1 on a block-mode batch (H > 1). */
int BeatriceBatch_ConvertBlocks48k(BeatriceBatch* b, const float* in, float* out, int channels);
int BeatriceBatch_ConvertBlocks48kDevice(BeatriceBatch* b, const float* d_in, float* d_out, int channels);
/* Throughput form: n_slots (> BeatriceBatch_TickStages()) resident 48 kHz blocks per direction, [n_slots][B][channels][480], with
 * the tick pipeline between them (the batch allocates its own 16 / 24 kHz slots).  While bound, block k --
 * BeatriceBatch_ConvertBlocks48kDevice(b, NULL, NULL, channels) -- is taken from slot k mod n_slots, and its converted block
 * appears in the same slot of d_out48 BeatriceBatch_TickStages() - 1 calls later or after BeatriceBatch_Synchronize: the
 * samples of the in-order call, later.  NULL, NULL unbinds (and leaves tick mode).
 * Binding, binding again (another slot count, other buffers: footnote 5 of MODES) and unbinding drain the pipeline and restart NOTHING of a
 * stream: its 48 kHz wrapper state (the latched model output, the down-sampler's and the up-sampler's histories) and its model state carry
 * over, so blocks fed in order, then bound, then in order again are, block for block, the samples of ONE in-order run.  The next call
 * after a bind reads slot 0.
 * On a batch with H = 2 or 4 hops per step (BeatriceBatch_CreateBlock(..., H)) a slot holds H consecutive blocks per stream,
 * [n_slots][B][H][channels][480], and every call converts them all (the samples of H in-order calls). */
int BeatriceBatch_BindResidentIO48k(BeatriceBatch* b, const float* d_in48, float* d_out48, int channels, int n_slots);
/* The shell's rule "a block whose down-mix is all zeros is not converted: the core is not called, its state and its 10 ms FIFO
 * stand still, the output is that down-mix" (reference src/vst/processor.cc:204-214), PER STREAM, for the in-order 48 kHz blocks
 * (one hop per step, no pipelining).  Enabled, BeatriceBatch_ConvertBlocks48k finds the silent streams of every call itself with
 * the shell's own test; for BeatriceBatch_ConvertBlocks48kDevice the caller flags them (flags[B], non-zero = silent) before the
 * call, once per block.  A silent stream's model state, wrapper state, pending key/value installs and codebook lottery stand
 * still as if the block had never existed (the batch runs the step for every stream and puts the silent ones back: rings rotated,
 * in-place state restored).
 * In TICK MODE (BeatriceBatch_EnableTickPipeline, or the 48 kHz blocks around the ticks, BeatriceBatch_BindResidentIO48k; one hop
 * per step): enable the rule after entering the mode; the streams flagged with BeatriceBatch_SetSilentStreams sit the NEXT step out --
 * the step carries each stream's own step counter through the pipeline, a second instance of the launch runs from then on.  At
 * every drained point (BeatriceBatch_Synchronize, leaving the mode) the streams are brought back to the batch's one counter
 * (their rings rotated by the steps they missed), so the common launch runs again and BeatriceBatch_EnableTickPipeline(b, 0) /
 * BeatriceBatch_BindResidentIO48k(b, NULL, NULL, ..) succeed as on any batch.  A batch of several hops per step takes the rule in tick mode
 * as well (round 6; plain or with the 48 kHz blocks around the ticks): a flagged stream then sits a WHOLE step -- its H hops, its H 48 kHz blocks, which come back as
 * their own down-mix -- out; a single silent block among sounding ones of a step is converted like them (the shell's per-block rule: one hop per step).
 * Returns -1 under host streaming or resident wrapper blocks, and (in order) with resident I/O, stage pipelining or several hops per step. */
int BeatriceBatch_EnableSilentBlockRule(BeatriceBatch* b, int enable);
int BeatriceBatch_SetSilentStreams(BeatriceBatch* b, const unsigned char* flags);
/* The shell's test on blocks that live on the DEVICE: the flags that BeatriceBatch_SetSilentStreams, BeatriceBatch_ConvertBlocks48kDevice and
 * BeatriceBatch_ProcessBlocksRaggedDevice expect from a caller whose audio never was on the host.  Input: n_cells cells, cell c at float
 * c * cell_stride of d_blocks; a cell holds blocks_per_cell planar blocks [channels][n_samples] back to back, channels 1 or 2.  With
 * cell_samples (host, [n_cells]; needs blocks_per_cell = 1) cell c holds ONE block [channels][cell_samples[c]] at its start.  Output: one
 * byte per block, [n_cells][blocks_per_cell], 1 when every sample of the block's down-mix -- x[i], or (x0[i] + x1[i]) * 0.5f -- equals 0.0f
 * in float32, exactly the test BeatriceBatch_ConvertBlocks48k makes on host buffers: -0.0 and L = -R are silent, NaN and Inf are not,
 * subnormals count as the CPU counts them, a block of no samples is silent.  Nothing outside [block, block + channels * length) is read.
 *   The layouts of the resident modes: D's [n_slots][B][H*160] -- cells n_slots * B, blocks_per_cell H, n_samples 160, mono; G's
 *   [n_slots][B][channels][n] -- blocks_per_cell 1; P's [n_slots][B][channels * max_samples] with cell_samples = the lengths of the calls
 *   to come.  In P a block found silent is handed to BeatriceBatch_ProcessBlocksRaggedDevice as n_samples = 0; its output cell is then not
 *   written and is the caller's to zero.  F's slots: BeatriceBatch_ScanBoundBlocks48k below.
 * hip_stream: NULL = a non-blocking stream the batch keeps for scans (made by the first such call), so a scan never queues behind the
 * ticks in flight; or a stream of the caller's, which orders the scan behind whatever produced the blocks.  Either way it is the
 * CALLER'S PROMISE that the blocks have been written and are visible to that stream when the scan runs, and stay untouched until End.
 * Begin enqueues the scan and returns a ticket (>= 0); End waits for THAT ticket's scan only and copies its flags out; tickets end in any
 * order.  Up to four tickets may be outstanding: a fifth Begin returns -3 and changes nothing.  End of an unknown ticket, or of one that
 * has ended, returns -1.  BeatriceBatch_ScanSilentBlocks is Begin + End.  Begin allocates or grows the staging of its ticket (device and
 * pinned memory, by the size of the call): it is not a call for an audio thread.
 * Refused with -1, nothing enqueued: a NULL pointer (d_blocks, flags); n_cells < 1; blocks_per_cell < 1; channels other than 1 or 2;
 * n_samples < 1 (or > 2^30); cell_stride < blocks_per_cell * channels * n_samples (or > 2^40); cell_samples with blocks_per_cell != 1 or with an entry
 * outside [0, n_samples]; more than 2^20 blocks in one call.  -2: an unhealthy batch, or a HIP failure.
 * No scan call drains anything, moves a clock, or changes a flag or setting of the batch (footnote 10 of MODES). */
int BeatriceBatch_ScanSilentBlocksBegin(BeatriceBatch* b, const float* d_blocks, int n_cells, int blocks_per_cell, int channels, int n_samples,
                                        long long cell_stride, const int* cell_samples /* host [n_cells] or NULL */, void* hip_stream);
int BeatriceBatch_ScanSilentBlocksEnd(BeatriceBatch* b, int ticket, unsigned char* flags /* host [n_cells][blocks_per_cell] */);
int BeatriceBatch_ScanSilentBlocks(BeatriceBatch* b, const float* d_blocks, int n_cells, int blocks_per_cell, int channels, int n_samples,
                                   long long cell_stride, const int* cell_samples, void* hip_stream, unsigned char* flags);
/* Mode F (BeatriceBatch_BindResidentIO48k) only, -1 everywhere else: scans the resident input slots that the NEXT n_calls calls of
 * BeatriceBatch_ConvertBlocks48kDevice(b, NULL, NULL, channels) will read (1 <= n_calls <= n_slots, at most 2^20 blocks), in the binding's
 * layout [B][H][channels][480], and waits for the answer.  step_flags[k][s] (host, [n_calls][B]) = 1 when ALL H blocks of stream s in the
 * k-th of those calls are silent: what BeatriceBatch_SetSilentStreams wants before that call at any H (footnote 6).  block_flags (host,
 * [n_calls][B][H], or NULL) gets every block's own flag.  The rule need not be enabled to scan.  Takes one or two of the four tickets
 * while it runs (-3 if they are out).  hip_stream and the caller's promise: as above. */
int BeatriceBatch_ScanBoundBlocks48k(BeatriceBatch* b, int n_calls, unsigned char* step_flags /* [n_calls][B] */,
                                     unsigned char* block_flags /* [n_calls][B][H] or NULL */, void* hip_stream);

/* The same wrapper at ANY host rate and block size, with the dB-ramped gains (the whole of the reference's
 * ProcessorCore2::Process, src/common/processor_core_2.cc:24-48, per stream on the device): input gain (gain.h:41-71,
 * 2 dB/ms towards the target) -> host rate to 48 kHz (resample.h:130-237: Stern-Brocot ratio, Hann-windowed sinc tables) ->
 * exact-480 FIFO -> every third sample -> model hop -> zero-stuffing -> 48 kHz to host rate -> output gain -> every channel.
 * BeatriceBatch_ConfigureWrapper sets the host rate for the batch and restarts every stream's wrapper as the reference's SetSampleRate
 * (processor_core_2.cc:421-429) restarts it at a NEW rate: both resampler histories and the 480-sample FIFO become zeros, the two clocks and
 * the FIFO fill start over; both gains keep their target and their present value and ramp on, at the new rate, from the next block; model
 * state and settings are untouched.  Unlike SetSampleRate it does so at the PRESENT rate too (the reference: SetSampleRate(another rate),
 * SetSampleRate(the rate)) -- in mid-life, and after BeatriceBatch_ConfigureWrapperRates, which it replaces.
 * ACCEPTED RATES: the ratio between the host rate and 48 kHz is replaced by the fraction hi/lo >= 1 of smallest denominator that the
 * reference's search finds with both parts below 1000 (resample.h:25-46; 44.1 kHz: 160/147, 47 952 Hz: 999/998, 48 048 Hz: 1/1), and the
 * filter history of the high-rate side, 32 hi / lo + 1 samples, must fit the per-stream state block of 257 (the division is the
 * integer one, so what counts is hi/lo after the search: at most 8 and the sliver above it that rounds away) -- 6 kHz to 384 kHz.  A rate outside that range (5 900 Hz, 390 kHz), not finite or <= 0 is refused with -1 and NOTHING changes: the rate
 * configured before, every stream's clocks, histories, FIFO and gains stand, and the next block goes on as if nobody had asked.  The same
 * range holds for BeatriceBatch_ConfigureWrapperRates, BeatriceBatch_SetStreamRate and BeatriceBatch_SetStreamRateInFlight;
 * BeatriceBatch_ProcessBlocks[Device] converts one block of n samples per stream, [B][channels][n] planar, channels 1 or 2
 * (stereo is down-mixed (L+R)*0.5 as src/vst/processor.cc:183-192 does; the shell's skip of an all-zero block, :204-214,
 * is NOT applied per stream -- the streams of a batch advance together, a silent stream is converted like any other; the
 * one-stream form of that rule is ProcessorProxy::ProcessChannels, beatrice_host.h); n may change from call to call, up to
 * BeatriceBatch_MaxWrapperBlock(b) (4088 samples at the higher of the two rates).  A model hop runs whenever 480 samples
 * at 48 kHz have accumulated (0, 1 or several times per call).  Bit-identical to the host chain.  One 10 ms hop per step
 * batches only, pipelining off (a batch of several hops per step takes BeatriceBatch_ConfigureWrapper for
 * BeatriceBatch_BindResidentBlocks, below; the in-order calls return -1 on it). */
int BeatriceBatch_ConfigureWrapper(BeatriceBatch* b, double host_sample_rate);
int BeatriceBatch_SetInputGain(BeatriceBatch* b, int stream, double gain_db);
int BeatriceBatch_SetOutputGain(BeatriceBatch* b, int stream, double gain_db);
int BeatriceBatch_ProcessBlocks(BeatriceBatch* b, const float* in, float* out, int channels, int n_samples);
int BeatriceBatch_ProcessBlocksDevice(BeatriceBatch* b, const float* d_in, float* d_out, int channels, int n_samples);
int BeatriceBatch_MaxWrapperBlock(const BeatriceBatch* b);
/* The same wrapper with clocks PER STREAM -- what the reference gives every plugin instance (src/common/resample.h:401-438,
 * processor_core_2.h:28): a batch whose streams come from hosts at different rates and block sizes.
 * BeatriceBatch_ConfigureWrapperRates: rates[B], the host rate of each stream (restarts every stream's resampler pair and FIFO;
 * gains keep their state; the uniform entry points above are off until BeatriceBatch_ConfigureWrapper is called again).
 * BeatriceBatch_ProcessBlocksRagged: for every stream s one block of n_samples[s] samples at its rate (0: the stream sits the
 * call out); in / out (host): the streams' planar blocks [channels][n_samples[s]] one after the other.  A stream fires a model
 * hop whenever ITS 480-sample FIFO fills; a model step runs for the streams that fire in it, the others stand still.
 * apply_silent_rule != 0: the shell's rule per stream (src/vst/processor.cc:204-214): a block whose down-mix is all zeros is
 * not converted -- gains, resampler clocks, FIFO, model state, key/value installs and codebook lottery of that stream do not
 * move, its output block is zeros.  In-order mode.  Bit-identical to one reference wrapper per stream. */
int BeatriceBatch_ConfigureWrapperRates(BeatriceBatch* b, const double* rates);
int BeatriceBatch_ProcessBlocksRagged(BeatriceBatch* b, const float* in, float* out, int channels, const int* n_samples, int apply_silent_rule);
/* ONE stream's host side of such a batch, without touching the others: a caller changes its sample rate, a slot goes to a new caller, a
 * stream moves to another batch with its resampler histories, FIFO, clocks and gain ramps.  All six calls below work where
 * BeatriceBatch_ProcessBlocksRagged works (MODES, footnote 9: in order or with the in-order silent rule, one hop per step, after
 * BeatriceBatch_ConfigureWrapperRates, no binding) and are refused with -1 (the getters: 0.0 / 0) everywhere else, changing nothing: before
 * BeatriceBatch_ConfigureWrapperRates, under the uniform BeatriceBatch_ConfigureWrapper alone, in modes B - G and P.  They are settings,
 * not mode entry points (no row in the MODES table); a call that is not refused first waits for what the batch has enqueued.
 * BeatriceBatch_SetStreamRate is the reference's SetSampleRate (processor_core_2.cc:421-429) for that one stream: an equal rate returns 0
 * and does nothing; otherwise the stream's two resampler histories and its FIFO become zeros, its two clocks and its FIFO fill start
 * over, and its gains keep their target and present value and ramp at the new rate from the next block on.  The stream's model state and
 * settings are untouched, and no bit of any other stream changes -- device state, clocks, gains.  BeatriceBatch_RestartStreamWrapper is
 * the same restart at the stream's present rate (the reference: SetSampleRate(another rate), SetSampleRate(the rate)); together with
 * BeatriceBatch_ResetStream it turns a slot over to a new caller.  BeatriceBatch_StreamRate: the stream's rate (0.0: none / bad argument).
 * Streams of equal rate share their tap tables (a rate class).  A rate no stream has had becomes a new class; the tables are rebuilt
 * whenever the set of rates in use changes, without the classes no stream uses any more, so a batch never holds more classes than
 * streams; every other stream goes on reading the same taps.
 * -1 and no change: a stream out of range; a rate that is not finite, <= 0, or whose filter history exceeds the state block (above
 * 384 kHz).  -2: HIP or allocation failure -- the new tables are built before anything is committed, so host and device state of every
 * stream still agree. */
int BeatriceBatch_SetStreamRate(BeatriceBatch* b, int stream, double host_sample_rate);
int BeatriceBatch_RestartStreamWrapper(BeatriceBatch* b, int stream);
double BeatriceBatch_StreamRate(const BeatriceBatch* b, int stream);
/* The wrapper's per-stream state as a token of its own, beside the stream blob of BeatriceBatch_ExportStreams: the stream's rate, its
 * two resampler clocks and FIFO fill, both gain clocks (target and present gain in dB), its four filter histories and the 480-sample
 * FIFO.  After BeatriceBatch_ExportStreamWrappers(X, s) and BeatriceBatch_ImportStreamWrappers(Y, t) -- and the stream blob's pair, in
 * either order: the two tokens are independent -- the next block of stream t through BeatriceBatch_ProcessBlocksRagged on Y is bit for
 * bit the block stream s would have got from X, whatever the block lengths that follow.  Export changes nothing in X; import changes no
 * other stream of Y and adds the rate's class if Y lacks it (as BeatriceBatch_SetStreamRate does).  One launch per 16 streams each way.
 * Like the stream blob it is a short-lived token between two batches of the SAME library build, not a storage format
 * (beatrice-vst_amd/csrc/wrapper_blob.h: what is refused, and why every blob that is taken keeps the kernels inside their buffers).
 * BeatriceBatch_WrapperBlobBytes: bytes of ONE stream's wrapper blob; 0 where the two calls are refused.
 * All or nothing, every blob validated before anything is staged.  -1 and no change (no drain, no launch): n < 1 or n > the batch's
 * streams; a NULL pointer; a stream out of range or named twice; on import a blob with a bad magic word, version, size or check word, a
 * rate BeatriceBatch_SetStreamRate would refuse, a resampler clock outside [0, hi) of its rate's ratio hi / lo, a FIFO fill outside
 * [0, 480), a gain that is not finite.  A clock pair in range that no run of calls could have produced may make a later
 * BeatriceBatch_ProcessBlocksRagged return -2 (its plan's check); it never reads or writes out of bounds.  -2: HIP or allocation failure. */
size_t BeatriceBatch_WrapperBlobBytes(const BeatriceBatch* b);
int BeatriceBatch_ExportStreamWrappers(BeatriceBatch* b, int n, const int* streams, void* blobs /* host, n * WrapperBlobBytes(b) */);
int BeatriceBatch_ImportStreamWrappers(BeatriceBatch* b, int n, const int* streams, const void* blobs /* host, n blobs */);
/* Throughput form of the any-rate wrapper: the TICK pipeline between resident host-rate blocks (as BeatriceBatch_BindResidentIO48k
 * is for 48 kHz / 0 dB).  d_in / d_out: [n_slots][B][channels][n_samples] planar, at the rate of BeatriceBatch_ConfigureWrapper.
 * Call k = BeatriceBatch_ProcessBlocksDevice(b, NULL, NULL, channels, n_samples) reads slot k mod n_slots; its output block is in
 * the same slot of d_out BeatriceBatch_ResidentBlocksDelay() (= TickStages() - 1) calls later, or after BeatriceBatch_Synchronize.
 * Gains (BeatriceBatch_SetInputGain / SetOutputGain) and every per-stream setting apply to the call that follows them, as in
 * order.  Same samples as BeatriceBatch_ProcessBlocksDevice in order.  n_slots >= TickStages() + 1.  NULL pointers unbind.
 * Binding, binding again without unbinding (another block length, slot count: footnote 5 of MODES) and unbinding each restart the wrapper
 * (resampler histories, clocks, FIFO) as BeatriceBatch_ConfigureWrapper does; gains keep target and present value, ramps in progress go on;
 * the streams' model state carries on.  The next call after a bind is call 0 and reads slot 0.  An unbind whose restart fails returns -2:
 * the binding is gone and the in-order entry points are refused until BeatriceBatch_ConfigureWrapper succeeds.
 * On a batch with H = 2 or 4 hops per step (BeatriceBatch_CreateBlock(..., H); BeatriceBatch_ConfigureWrapper accepts it for this
 * entry point only): the model hops the FIFOs fire are collected H at a time -- hop k of the batch is hop k mod H of step k / H --
 * and a step enters the pipeline when it is full, so every tick launch carries H hops per stream as in plain tick mode; ticks run
 * only then (no idle tick per call).  A call's block is out once the step of its newest hop has filled and TickStages() - 1 further
 * steps have gone in behind it: BeatriceBatch_ResidentBlocksDelay() = the calls that bring ((H - 1) + (TickStages() - 1) x H) x 480
 * inner samples, + 1 (the output half rides in the next call's launch: one launch per call beside the tick launches) (ask BeatriceBatch_ResidentBlocksDelayFor(b, n_samples) before binding: n_slots >= that + 2; -1 for blocks shorter
 * than two inner samples).  BeatriceBatch_Synchronize drains the ticks and completes the calls whose hops' steps are full; the last
 * calls, which end on a step still filling, stay owed (BeatriceBatch_ResidentBlocksOwed, 0 at one hop per step) until later calls
 * fill it -- an offline caller ends a file with BeatriceBatch_FlushResidentBlocks (or with that many blocks of silence).  Same samples as one
 * hop per step.  Unbinding or binding again WITHOUT a flush gives the owed calls up: their blocks are never written, and the hops of the step
 * that was still filling never reach the model (the streams' model state is that of the full steps). */
int BeatriceBatch_BindResidentBlocks(BeatriceBatch* b, const float* d_in, float* d_out, int channels, int n_samples, int n_slots);
int BeatriceBatch_ResidentBlocksDelay(const BeatriceBatch* b);
int BeatriceBatch_ResidentBlocksDelayFor(const BeatriceBatch* b, int n_samples);
int BeatriceBatch_ResidentBlocksOwed(const BeatriceBatch* b);
/* End of the material (reference src/common/resample.h:331-364: the FIFO hands a block's samples out one block later -- whatever follows):
 * every call made so far gets its output block, as if blocks of silence had followed -- the library makes up calls of its own, each one block
 * of zeros of the binding's length through the running wrapper (no caller slot is read or written for them, they are not counted as calls),
 * until the newest hop that a call of the caller's needs lies in a full step; it drains the pipeline and runs the output halves still owed --,
 * then the binding STARTS OVER as a new one does: resampler pair and FIFO restarted, the next call is call 0 and reads slot 0.
 * BeatriceBatch_ResidentBlocksOwed() is 0 afterwards.
 *   Which hops reach the model: a made-up call fires whatever hops its block brings, not just those the open step lacks.  Every FULL step goes
 *   through the model, a further full step of the last made-up call included -- what a host that went on with that much silence would have
 *   run.  A hop fired beyond the last full step is DROPPED when the binding starts over: the model never sees it (the reference host would
 *   have run it; the streams then stand at most H - 1 hops of silence short of it).  The streams' model state carries on from the last full step.
 *   The gains: their clocks advance through every made-up block as through a caller's block of that length, so a ramp in progress goes on
 *   (or ends) during the flush; target and present value are kept across the restart, as at BeatriceBatch_ConfigureWrapper.
 * With nothing owed (always so at one hop per step and with clocks per stream; at several hops per step when the newest hop needed already
 * lies in a full step) it is BeatriceBatch_Synchronize and the binding is left AS IT IS: nothing restarts, the next call is not call 0 and
 * reads slot k mod n_slots.  -1 without a binding. */
int BeatriceBatch_FlushResidentBlocks(BeatriceBatch* b);
/* The throughput form with clocks PER STREAM (reference src/common/resample.h:401-438: every plugin instance owns its resampler
 * pair; here a batch whose streams come from hosts at 44.1, 48, 96 kHz ... with block sizes of their own, around ONE tick pipeline).
 * After BeatriceBatch_ConfigureWrapperRates: d_in / d_out = [n_slots][B][channels * max_samples]; stream s's block of a call, planar
 * [channels][n_samples[s]], sits at the start of its cell.  Call k = BeatriceBatch_ProcessBlocksRaggedDevice(b, n_samples) reads slot
 * k mod n_slots: n_samples[B], 0 <= n_samples[s] <= max_samples (and the per-rate limit of BeatriceBatch_ProcessBlocksRagged),
 * 0 = the stream sits the call out (nothing of it moves, no output).  A stream fires a model hop when ITS 480-sample FIFO fills; the
 * step that enters the ticks carries the streams that fired, the others sit it out with step counters of their own (the tick launch's
 * ragged steps).  The output blocks of call k are in the same slot of d_out BeatriceBatch_ResidentBlocksDelay() (= TickStages() - 1)
 * calls later, or after BeatriceBatch_Synchronize.  Gains and per-stream settings apply to the call that follows them.  Same samples
 * as BeatriceBatch_ProcessBlocksRagged in order = one reference wrapper per stream.  One hop per step, n_slots >= TickStages() + 1.
 * NULL pointers unbind (either bind call unbinds either form); binding and unbinding restart every stream's resampler pair and FIFO
 * (gains keep target and present value).  An unbind whose restart fails returns -2: the binding is gone and the in-order entry points are
 * refused until BeatriceBatch_ConfigureWrapperRates succeeds. */
int BeatriceBatch_BindResidentBlocksRagged(BeatriceBatch* b, const float* d_in, float* d_out, int channels, int max_samples, int n_slots);
int BeatriceBatch_ProcessBlocksRaggedDevice(BeatriceBatch* b, const int* n_samples);
/* ONE stream's life cycle INSIDE that binding, without touching the others and without leaving the throughput mode: a caller's host changes
 * its sample rate, a caller hangs up and another takes the slot.  The three calls work exactly where BeatriceBatch_ProcessBlocksRaggedDevice
 * works (MODES, footnote 11: mode P) and are refused with -1 (the getter: 0.0) everywhere else, changing nothing.  They are settings, not
 * mode entry points.  A call applies at the boundary in front of the next BeatriceBatch_ProcessBlocksRaggedDevice.
 * BeatriceBatch_SetStreamRateInFlight is the reference's SetSampleRate (processor_core_2.cc:421-429) for that one stream: an equal rate
 * returns 0 and does nothing; otherwise both resampler histories of the stream and its FIFO read as zeros from that call on, its two
 * clocks, its FIFO fill and its 48 kHz sample count start over, both gains keep target and present value and ramp at the new rate; model
 * state and settings are untouched.  BeatriceBatch_RestartStreamInFlight is the same restart, also at the present rate
 * (host_sample_rate = 0.0; the reference: SetSampleRate(another rate), SetSampleRate(the rate)); with reset_model != 0 it also does what
 * BeatriceBatch_ResetStreamInFlight does in plain tick mode -- the stream's next present step is the first step of a new stream, all four
 * key/value blocks of its target speaker are installed at that step (set the new caller's voice first), steps already in the pipeline
 * finish on the old state: the slot is turned over to a new caller.  A stream that then hands in n_samples = 0 starts over at the first
 * step it takes part in.  BeatriceBatch_BoundStreamRate: the stream's rate in P (0.0: refused / bad argument); after the unbind
 * BeatriceBatch_StreamRate reports it.
 * NOTHING DRAINS: no call of the three synchronises, launches a tick or runs an output half -- BeatriceBatch_TicksLaunched and
 * BeatriceBatch_ResidentBlocksOwed read the same before and after.  The blocks of earlier calls that are still owed come out
 * BeatriceBatch_ResidentBlocksDelay() calls after their own call, with the old rate, the old taps and the old output histories, as if
 * nothing had been asked; the restarted stream's first 480 inner samples behind the restart come back as zeros (the reference's zeroed
 * FIFO), the hops it still has in the pipeline are never read; no bit of any other stream changes.  BeatriceBatch_Synchronize,
 * BeatriceBatch_FlushResidentBlocks and the unbind work while a restart or a reset is waiting for the stream's next block.
 * All or nothing.  -1 and no change: a stream out of range; a rate BeatriceBatch_SetStreamRate would refuse; a rate at which a block of
 * min(max_samples, the rate's longest block) samples could fire more model hops per call than the binding's slot ring and slot map were
 * sized for when it was made -- that size comes from the lowest rate among the streams at bind time, so BIND WHILE A STREAM OF THE LOWEST
 * RATE YOU EXPECT IS CONFIGURED (and set its real rate with BeatriceBatch_SetStreamRateInFlight before the first call).  -2: HIP or
 * allocation failure; nothing is committed.
 * A rate no stream of the binding has had ALLOCATES (the rate's tap tables on the host, their place in the tap buffer, possibly a longer
 * buffer; beatrice-vst_amd/csrc/wrapper_turnover_plan.h) and computes the tables: like BeatriceBatch_ScanSilentBlocksBegin it is not for an
 * audio thread.  A rate the binding still holds -- a stream is on it, or was within the last ResidentBlocksDelay() + 1 calls -- costs a
 * few stores. */
int BeatriceBatch_SetStreamRateInFlight(BeatriceBatch* b, int stream, double host_sample_rate);
int BeatriceBatch_RestartStreamInFlight(BeatriceBatch* b, int stream, double host_sample_rate /* 0.0: the present rate */, int reset_model);
double BeatriceBatch_BoundStreamRate(const BeatriceBatch* b, int stream);
/* A stream MOVES between two such bindings with everything it owns, and neither batch drains: what BeatriceBatch_MoveStreamsInFlight /
 * ExportStreamsInFlight / ImportStreamsInFlight are to plain tick mode, for mode P (MODES, footnote 13; refused with -1, the size 0,
 * everywhere else, D included).  Settings, not mode entry points.  The rules: beatrice-vst_amd/csrc/bound_move_plan.h.
 * AT REST.  A bound stream owns more than its model state: its resampler histories and FIFO, and the output of its last fired model hop,
 * which the output half of its NEXT block still reads.  It is at rest when (a) no step of it is inside the ticks and (b) the output half of
 * every call it handed a block in has been launched -- which is the case once BeatriceBatch_ResidentBlocksDelay() calls have been made in
 * which it sat out (n_samples[s] = 0), or behind BeatriceBatch_Synchronize.  BeatriceBatch_BoundStreamQuiescent: 1 / 0; -1 out of range
 * or outside P.
 * NOTHING DRAINS: no call of the five launches a tick, runs an output half or synchronises the batch; BeatriceBatch_TicksLaunched,
 * BeatriceBatch_ResidentBlocksOwed, every other stream's clocks and BeatriceBatch_BoundStreamRate of every other stream read the same
 * before and after.  The export waits for its own copies only, on an event.
 * THE SOURCE IS UNCHANGED: fed again, the stream goes on as if nothing had been asked; turn the slot over with
 * BeatriceBatch_RestartStreamInFlight(s, 0.0, 1).  THE DESTINATION SLOT CONTINUES THE STREAM: the next block handed in for destination
 * stream t is, bit for bit, the block source stream s would have got next, whatever block lengths follow -- one reference wrapper per
 * stream (reference src/common/resample.h:401-438).  What travels: the model rings, each turned at the stream's own counter; settings and
 * the lottery engine, through entry_map as in BeatriceBatch_ImportStreams; the wrapper's filter histories and FIFO, the last hop's
 * output, the rate, both resampler clocks and the FIFO fill; both gain clocks (target and present dB: a ramp in progress goes on); the
 * 48 kHz sample count.  The destination's own hop numbering goes on.  A reset or restart still pending on a DESTINATION stream is
 * cancelled.  The destination acquires the rate's class exactly as BeatriceBatch_SetStreamRateInFlight does: a rate it does not hold
 * ALLOCATES -- not for an audio thread.
 * The blobs are interchangeable tokens: stream blobs are those of BeatriceBatch_ExportStreams, wrapper blobs those of
 * BeatriceBatch_ExportStreamWrappers (same format, same version, BoundWrapperBlobBytes == WrapperBlobBytes of an in-order batch); a blob
 * of either export is taken by either import, bound or in order.  (A wrapper blob holds the FIFO fill, not the 48 kHz sample count: an
 * imported stream counts from 480 + fill, which reads the same samples.)
 * All or nothing, in this order.  -1 and no change: arguments (a NULL pointer, n < 1, a stream out of range or named twice, entry_map /
 * n_map not paired); a batch outside P; a blob BeatriceBatch_ImportStreams or ImportStreamWrappers would refuse; for the move src == dst,
 * two devices, another hops per step or ring layout; a rate the destination would refuse in BeatriceBatch_SetStreamRateInFlight (its
 * blocks could fire more hops per call than the binding was sized for).  -3 and no change: a named stream, source or destination, is not
 * at rest by both rules, or a SOURCE stream has a BeatriceBatch_ResetStreamInFlight or a restart pending that no block has taken.  Only
 * then is anything allocated, staged or launched; -2: HIP or allocation failure.
 * Two batches on two HIP streams are fenced by events as in BeatriceBatch_MoveStreamsInFlight; on one shared stream
 * (BeatriceBatch_SetStream) no event is needed. */
int BeatriceBatch_BoundStreamQuiescent(const BeatriceBatch* b, int stream);
int BeatriceBatch_MoveBoundStreamsInFlight(BeatriceBatch* src, BeatriceBatch* dst, int n, const int* src_streams, const int* dst_streams,
                                           const int* entry_map, int n_map);
int BeatriceBatch_ExportBoundStreamsInFlight(BeatriceBatch* b, int n, const int* streams, void* stream_blobs /* n * StreamBlobBytes */,
                                             void* wrapper_blobs /* n * BoundWrapperBlobBytes */);
int BeatriceBatch_ImportBoundStreamsInFlight(BeatriceBatch* b, int n, const int* streams, const void* stream_blobs, const void* wrapper_blobs,
                                             const int* entry_map, int n_map);
size_t BeatriceBatch_BoundWrapperBlobBytes(const BeatriceBatch* b);

/* Execution control: use an externally owned hipStream_t (e.g. the framework's current stream);
 * replay the per-hop kernel chain from a captured hipGraph (default on). */
int BeatriceBatch_SetStream(BeatriceBatch* b, void* hip_stream);
void* BeatriceBatch_GetStream(const BeatriceBatch* b);
int BeatriceBatch_EnableGraph(BeatriceBatch* b, int enable);
/* Throughput mode for callers that enqueue steps ahead of their completion (BeatriceBatch_ConvertFramesDevice
 * without waiting, resident I/O).  The per-hop chain is ~40 dependent, latency-bound launches that leave most of
 * the chip idle; with a pipeline depth n = 2..4 it is cut into n stages (front end = content encoder + pitch
 * estimator; the waveform generator in 1..3 parts) on n HIP streams, and stage s of step t+1 overlaps stage s+1 of
 * step t.  Same samples (bit for bit).  enable: 0 = off (default: everything in order on the batch's stream),
 * 1 = depth 2, 2..4 = that depth.  A step's output is complete after BeatriceBatch_Synchronize, or in stream order
 * on BeatriceBatch_GetWaveStream.  The 48 kHz entry points need it off.  Depth 4 needs more hardware queues than ROCm
 * hands a process by default (environment GPU_MAX_HW_QUEUES=8, set before the HIP runtime starts): streams that
 * share a queue do not overlap, and depth 4 then runs slower than depth 3. */
int BeatriceBatch_EnablePipelining(BeatriceBatch* b, int enable);
void* BeatriceBatch_GetWaveStream(const BeatriceBatch* b);
/* Tick pipelining: the deepest form of the same idea, on ONE stream.  Every layer of the chain is its own pipeline
 * stage (the conditioned blocks: two stages each, as row-local chains); each BeatriceBatch_ConvertFramesDevice(b, NULL, NULL)
 * is one "tick" -- a single launch of 512-thread workgroups in which stage s works on the step fed s ticks ago, so ~26
 * steps are in flight and their ~1900 independent workgroups (at 256 streams) fill the chip two per CU, with the kernel boundary between
 * ticks as the only synchronisation.  Same samples, bit for bit; a step's output lands
 * in its resident-I/O slot BeatriceBatch_TickStages() - 1 ticks after its input was fed, and BeatriceBatch_Synchronize
 * drains the pipeline (that many ticks without new input).  Settings changed between steps apply to exactly the step
 * they precede.  Requirements (-1 otherwise): one, two or four hops per step, at most 4096 streams (tested to 4096), resident I/O bound with more slots
 * than stages and at most 4096 of them, and the caller must leave a step's INPUT slot untouched for BeatriceBatch_TickStages() further steps.
 * The host-buffer, 48 kHz and profiling entry points return -1 while it is on.
 * H = 2 or 4 hops per step (a batch from BeatriceBatch_CreateBlock(..., H); slots of [B][H * 160] in, [B][H * 240] out): every stage
 * works on all hops of its step in one launch -- the fixed cost of a launch is paid once per H hops, and a short run has fewer
 * partly filled launches per hop (256 streams, 20 steps + drain: 2.72 / 3.44 / 3.9 M frames/s at 1 / 2 / 4 hops per step; steady
 * 3.8 / 4.35 / 4.38 M; 64 speakers on 256 streams: 2.30 / 3.01 / 3.45 M), same samples as one hop per step, settings still apply
 * per step and key/value installs per hop.  The 48 kHz wrapper around the ticks takes such a batch too
 * (BeatriceBatch_BindResidentIO48k: a slot then holds H consecutive blocks per stream, [B][H][channels][480], and a call converts
 * them all: 64 stereo streams 1.41 / 2.32 / 2.9 M frames/s), and so does host streaming (BeatriceBatch_StreamFrames then takes
 * [B][H * 160] and returns [B][H * 240]) and the any-rate wrapper around the ticks (BeatriceBatch_BindResidentBlocks: a step enters the
 * pipeline when the FIFOs have fired H hops); the silent-block rule needs one hop per step. */
int BeatriceBatch_EnableTickPipeline(BeatriceBatch* b, int enable);
int BeatriceBatch_TickStages(const BeatriceBatch* b);
/* Host streaming: tick pipelining for callers whose audio lives in HOST memory (offline conversion of files, a network
 * front end).  BeatriceBatch_EnableHostStreaming(b, 1) gives the batch its own resident slots + pinned mirrors and turns
 * tick mode on (requirements as above, nothing else bound); every BeatriceBatch_StreamFrames(b, in, out) then takes one
 * hop of every stream ([B][160] in) and -- once the pipeline is full -- returns 1 with `out` ([B][240]) holding the samples
 * of the step fed BeatriceBatch_HostStreamDelay() calls earlier (0 while filling: `out` untouched).  The resident slots ARE
 * the pinned host mirrors: the first stages read their hop and the last stage writes its samples over PCIe themselves, so
 * there is no copy command and no second stream, and the transfers hide among the tick's workgroups.  After the last
 * input, BeatriceBatch_StreamFlush(b, out) returns the remaining steps one per call (1, then 0 when none is left).
 * Same samples as BeatriceBatch_ConvertFrames, bit for bit.  This is the host-buffer form of what src/common's
 * ProcessorCore2::Process does per stream (processor_core_2.cc:24-48: in -> model hop -> out), for a whole batch. */
int BeatriceBatch_EnableHostStreaming(BeatriceBatch* b, int enable);
int BeatriceBatch_HostStreamDelay(const BeatriceBatch* b);
int BeatriceBatch_StreamFrames(BeatriceBatch* b, const float* in, float* out);
int BeatriceBatch_StreamFlush(BeatriceBatch* b, float* out);
/* Measurement hook (tick mode on, pipeline full): `ticks` (<= 64) more ticks back to back between one pair of HIP events
 * on the batch's stream: mean microseconds per launch (boundary to the next launch included) + the launch's algorithmic
 * FLOPs and bytes. */
int BeatriceBatch_TimeTickLaunch(BeatriceBatch* b, int ticks, float* us_per_launch, double* flops, double* bytes);
/* Optional: capture the hipGraphs of the current mode now (settings, I/O binding, pipelining as they stand; nothing
 * runs), so that the first steps do not spend milliseconds on it.  Otherwise it happens inside the first step. */
int BeatriceBatch_Prepare(BeatriceBatch* b);

/* Resident buffers of the batch ([B][H*160] in, [B][H*240] out) for callers that produce / consume
 * audio on the device. */
float* BeatriceBatch_DeviceInput(BeatriceBatch* b);
float* BeatriceBatch_DeviceOutput(BeatriceBatch* b);

/* Test hook: copies the last step's intermediate results (any pointer may be NULL):
 * phone [B][H][128], raw bins [B][H], transformed bins [B][H], features [B][H][4]. */
int BeatriceBatch_GetIntermediates(BeatriceBatch* b, float* phone, int* q_raw, int* q, float* feat);

/* Measurement hook: runs `steps` steps (H hops each) on the resident input buffer, timed with HIP events recorded
 * on the batch's own stream; returns total milliseconds in *ms. */
int BeatriceBatch_TimeSteps(BeatriceBatch* b, int steps, float* ms);

/* Per-kernel measurement hook: runs ONE hop eagerly (no graph) with every launch of the chain
 * bracketed by HIP events on the batch's stream; each launch is issued `repeats` times back to back
 * inside its bracket and the bracket time is divided by `repeats` (launches that update state in place -- the GRUs,
 * the pitch head, the upsampler tail -- are issued once, so the profiled hop is an ordinary hop of the stream).  Launches with the same name are accumulated.  Fills up to max_entries rows:
 * names (64 bytes each, NUL terminated), launches per hop, mean microseconds per launch, and the
 * algorithmic FLOPs and bytes of one launch.  Returns the number of rows. */
int BeatriceBatch_ProfileKernels(BeatriceBatch* b, int repeats, int max_entries, char* names, int* launches,
                                 double* mean_us, double* flops, double* bytes);

BEATRICE_ABI_END

#endif /* BEATRICE_BATCH_H_ */
