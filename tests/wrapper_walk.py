"""One batch walked through the wrapper modes with its state carried over, and the yardstick walked through the same script.

Test plumbing (no pytest): tests/test_cpu_wrapper_walk.py runs the yardstick alone (witnesses, negative controls), tests/test_gpu_wrapper_walk.py
runs the product beside it and compares every output block that include/beatrice_batch.h says is produced, bit for bit.

A case is a list of ops:
  ("cfg", rate)                 BeatriceBatch_ConfigureWrapper
  ("io", n, block, channels)    n in-order BeatriceBatch_ProcessBlocks calls
  ("bind", block, channels, k)  BeatriceBatch_BindResidentBlocks (on a bound batch: footnote 5 of MODES, no unbind first); k picks the slot count
  ("g", n)                      n calls BeatriceBatch_ProcessBlocksDevice(NULL, NULL)
  ("flush",)                    BeatriceBatch_FlushResidentBlocks
  ("unbind",)                   BeatriceBatch_BindResidentBlocks(NULL, NULL)
  ("cfgr", rates)               BeatriceBatch_ConfigureWrapperRates
  ("rag", n, blocks, channels[, rule])  n in-order BeatriceBatch_ProcessBlocksRagged calls, blocks[s] samples for stream s; rule: apply_silent_rule
  ("bindr", blocks, channels, k)  BeatriceBatch_BindResidentBlocksRagged, cells of max(blocks) samples
  ("p", n)                      n calls BeatriceBatch_ProcessBlocksRaggedDevice
  ("unbindr",)                  BeatriceBatch_BindResidentBlocksRagged(NULL, NULL)
  ("io48", n, channels)         n in-order BeatriceBatch_ConvertBlocks48k calls
  ("bind48", channels, k)       BeatriceBatch_BindResidentIO48k (on a bound batch: footnote 5, no unbind first)
  ("f", n)                      n calls BeatriceBatch_ConvertBlocks48kDevice(NULL, NULL): H blocks per stream each
  ("unbind48",)                 BeatriceBatch_BindResidentIO48k(NULL, NULL)
  ("unbind", "cross") / ("unbindr", "cross")  the same unbinding through the OTHER form's call ("either bind call unbinds either form"):
                                BeatriceBatch_BindResidentBlocksRagged(NULL, NULL) leaves G, BeatriceBatch_BindResidentBlocks(NULL, NULL) leaves P
  ("rule", on)                  BeatriceBatch_EnableSilentBlockRule: S in order (the library finds the silent blocks itself); in F the caller
                                flags them with BeatriceBatch_SetSilentStreams before the call
Events ride in front of a call: ("gin" / "gout" / "spk", stream, value) and ("reset", stream): BeatriceBatch_ResetStream.
A TRANSITION is a maximal run of ops without a call between them, in mid-life (not the ops before the first call).  plant() puts in front of
every transition what it has to be about: both gains of every stream set 70 dB and more away one call before (2 dB/ms: 35 ms, longer than
any block used here), speaker switches one to three calls before (their key/value blocks install one per model hop), k-NN on for two
streams of three.  With clocks per stream (holes=True) also blocks that are absent (n_samples = 0) or silent (the shell's rule: all zeros in
order, n_samples = 0 in P) in the two calls on each side; stream 3 sits out the very call before the transition.  In the 48 kHz
family holes=True flags streams silent in the two calls on each side (a 48 kHz stream cannot be absent); resets=True resets stream 1 in
the call before every transition, stream 2 in the call behind it and stream 3 one call later.

THE YARDSTICK: per stream one wrapper oracle (oracle/wrapper_oracle.c, pinned to the reference's resample.h / gain.h) whose hop callback
runs one Stream1 of the CPU oracle -- nothing shared between streams.  ALL THREE families use this one yardstick: the per-stream family
at each stream's own rate instead of one continuing ProcessorProxy per stream, and the 48 kHz family at 48 000 Hz instead of the continued
chain of test_gpu_wrapper48k.py's oracle_leg_48k (which is this same oracle wrapper at 48 kHz under a bound of 1e-4; here the bound is
equality).  Only the callback form can say which fired hops reach the model, and it is pinned to the reference as the proxy is.
What the header's paragraphs say, as the yardstick does it:
  cfg, bind, re-bind, unbind, cfgr     the chain restarts -- SetSampleRate(rate); at the present rate SetSampleRate(another), SetSampleRate(rate)
                                       -- and both gains keep target and present value.
  flush, something owed (H > 1)        the host goes on with blocks of silence (the gains ramp through them) until the newest hop that a call
                                       made so far needs lies in a full step; then the chain restarts as above.  Of the hops fired since the
                                       binding started, those of FULL steps reach the model -- extra full steps of a made-up call included --
                                       and the hops of the step left part filled are dropped: the model never sees them.
  flush, nothing owed                  nothing: no restart, the next call is not call 0.
  unbind / re-bind at H > 1            the hops of the step left part filled are dropped in the same way; the calls that needed them
                                       (BeatriceBatch_ResidentBlocksOwed) never get their block and are not compared.
  bindr, unbindr                       as bind / unbind, per stream at its own rate; a flush in P never has anything owed.
  an absent or silent block            nothing of the stream moves: gains, clocks, FIFO, model state, key/value installs.
  bind48, re-bind48, unbind48          nothing restarts: the 48 kHz wrapper's latch and filter histories carry over (the chain goes on).
  rule                                 nothing of a stream moves when the rule goes on or off.
  reset                                the stream's model starts anew with all key/value blocks of its target speaker installed, every other
                                       setting kept; its 48 kHz wrapper restarts (latch and both histories zero).
A setting applies to the STEP that follows it: the H hops that enter the ticks together, so a speaker switch made before call c reaches the
model with hop H * (hops fired before c) // H of the binding -- known from a dry run of the clocks, as are the hops that get dropped.

NEGATIVE CONTROLS: the same script with the opposite contract at ONE transition -- "carried" where the yardstick restarts, "restarted" where
it carries over, "fresh" (gains restarted too) where the rate changes, "all_hops" (the dropped hops reach the model) at a flush that drops
some.  A control must differ from the yardstick within the first two calls after the transition, or the case tests nothing."""
import ctypes as C
import math

import numpy as np

import wrapperlib

OTHER_RATE = 8000.0      # SetSampleRate(another rate) of a restart at the present rate
MIN_HOPS = 22            # model hops on each side of every transition (the deepest model ring has 17 step slots)
MAX_STAGES = 30          # phase lengths are laid out for a tick pipeline of at most this many stages (28 today; asserted at run time)
N_KV = 4                 # key/value blocks of a speaker switch, one per hop
CALLS = ("io", "g", "rag", "io48", "f", "p")


def hops_per_call(rate, block):
    return block * 48000.0 / (rate * 480.0)


def calls_for(rate, block, H=1, bound=False):
    """Calls of a phase: at least MIN_HOPS model hops, and in a bound mode more than the binding's delay (rb_delay's bound, at MAX_STAGES)."""
    n = int(math.ceil((MIN_HOPS + H) / hops_per_call(rate, block))) + 1
    if bound:
        if H == 1:
            n = max(n, MAX_STAGES + 3)
        else:
            m_lo = math.floor(block * 48000.0 / rate) - 1
            n = max(n, int(math.ceil(((H - 1) + (MAX_STAGES - 1) * H) * 480.0 / m_lo)) + 5)
    return n


class Case:
    def __init__(self, name, B, H, ops, seed=0, want_flush=None, holes=False, resets=False):
        self.name, self.B, self.H, self.ops, self.seed, self.holes, self.resets = name, B, H, list(ops), seed, holes, resets
        self.absent, self.silent = set(), set()     # (global call index, stream): no block at all / a block the shell's rule skips
        self.want_flush = want_flush      # per flush op: the sub-case a dry run must find there ("noop", "exact", "over_leftover", "over_full")
        self.events = []                  # (global call index, kind, stream, value), applied before that call
        self.calls = []                   # per global call index: (mode, blocks[B], channels)
        self.transitions = []             # (index of the first op, index past the last op, global call index)
        self._layout()

    def _layout(self):
        c, i, ops = 0, 0, self.ops
        rate, block, ch = None, None, None
        started = False
        while i < len(ops):
            op = ops[i]
            if op[0] in CALLS:
                started = True
                if op[0] == "io":
                    block, ch = [op[2]] * self.B, op[3]
                elif op[0] == "rag":
                    block, ch = list(op[2]), op[3]
                elif op[0] == "io48":
                    block, ch = [480] * self.B, op[2]
                for _ in range(op[1]):
                    self.calls.append((op[0], block, ch))
                c += op[1]
                i += 1
                continue
            j = i
            while j < len(ops) and ops[j][0] not in CALLS:
                if ops[j][0] == "bindr":
                    block, ch = list(ops[j][1]), ops[j][2]
                if ops[j][0] == "bind":
                    block, ch = [ops[j][1]] * self.B, ops[j][2]
                if ops[j][0] == "bind48":
                    block, ch = [480 * self.H] * self.B, ops[j][1]
                j += 1
            if started and j < len(ops):
                self.transitions.append((i, j, c))
            i = j
        self.n_calls = c
        self.family48 = any(op[0] in ("io48", "f") for op in ops)

    def plant(self):
        """What every transition is about, in front of it (module docstring)."""
        B = self.B
        gin, gout, spk = [0.0] * B, [0.0] * B, [s % 3 for s in range(B)]
        for _i, _j, T in self.transitions:
            for s in range(B):
                if not self.family48:      # (the 48 kHz wrapper has no gains)
                    gin[s] = -70.0 - s
                    gout[s] = -71.0 - s
                    self.events.append((T - 1, "gin", s, gin[s]))
                    self.events.append((T - 1, "gout", s, gout[s]))
                    if gin[s] != 0.0:      # (down one call before the transition, up again two calls behind it: in flight across it either way)
                        self.events.append((T + 2, "gin", s, 0.0))
                        gin[s] = 0.0
                    if gout[s] != 3.0:
                        self.events.append((T + 2, "gout", s, 3.0))
                        gout[s] = 3.0
                spk[s] = (spk[s] + 1) % 3
                # (four 48 kHz blocks per step: a call is a whole step and takes all four installs, nothing can straddle -- stream 0 switches
                #  with the first call behind the transition instead)
                self.events.append((T if self.family48 and self.H == 4 and s == 0 else T - 1 - s % 3, "spk", s, spk[s]))
            if self.holes and self.family48:
                self.silent.update({(T - 1, 1), (T, 1), (T - 2, 2), (T + 1, 2)})
            elif self.holes:      # (only a call with clocks per stream can leave a stream out)
                self.absent.update(h for h in ((T - 2, 1), (T + 1, 1), (T - 1, 3), (T + 2, 3)) if self.calls[h[0]][0] in ("rag", "p"))
                self.silent.update(h for h in ((T - 1, 2), (T, 2), (T - 2, 4), (T + 1, 4)) if self.calls[h[0]][0] in ("rag", "p"))
            if self.resets:
                self.events.extend([(T - 1, "reset", 1, None), (T, "reset", 2, None), (T + 1, "reset", 3, None)])
        self.events.sort(key=lambda e: e[0])
        return self

    def hole(self, c, s):
        return (c, s) in self.absent or (c, s) in self.silent

    def vq_k(self, s):
        return (0, 1, 2)[s % 3]

    def signal(self, s):
        """[2][total samples]: stream s's two channels, consumed call after call whatever the rate (channel 1 is used by stereo calls only)."""
        total = sum(b[s] for _m, b, _c in self.calls) + 1
        return np.stack([wrapperlib.test_signal(total, 44100, seed=7000 + 97 * self.seed + 11 * s),
                         (0.6 * wrapperlib.test_signal(total, 44100, seed=7500 + 97 * self.seed + 11 * s)).astype(np.float32)])

    def mono(self, sig, pos, n, ch):
        if ch == 1:
            return np.ascontiguousarray(sig[0, pos:pos + n])
        return np.ascontiguousarray(((sig[0, pos:pos + n] + sig[1, pos:pos + n]) * np.float32(0.5)).astype(np.float32))


class Sched:
    """What a dry run of one stream's clocks knows before the models run."""

    def __init__(self):
        self.reach = []          # per fired hop, in firing order: does it reach the model
        self.eff = {}            # index into case.events (speaker switches of this stream) -> the model hop it is in force from
        self.made_up = {}        # op index of a flush -> blocks of silence the library makes up
        self.flush_kind = {}     # op index of a flush -> "noop" / "exact" / "over_leftover" / "over_full"
        self.owed = {}           # op index of a flush / unbind / re-bind -> calls of the binding whose block never comes (0 after a flush)
        self.fill = {}           # global call index of a transition -> samples waiting in the FIFO there
        self.dropped = {}        # op index -> hops dropped there


class _Walk:
    """One stream's chain through the case's ops.  model=None: the dry run (clocks only, blocks of zeros)."""

    def __init__(self, case, s, wl, model=None, sched=None, control=None, new_model=None):
        self.case, self.s, self.wl, self.model, self.control, self.new_model = case, s, wl, model, control, new_model
        self.target = s % 3      # the stream's target speaker
        self.dry = model is None
        self.sched = Sched() if self.dry else sched
        self.p, self.rate = None, None
        self.cb = wrapperlib.HOP_FN(self._hop)
        self.n_fired = self.n_model = 0
        # the segment since the last restart: H hops per step inside a binding, 1 in order
        self.seg_H, self.seg_f, self.seg_base, self.seg_calls = 1, 0, 0, []
        self.pending = []        # (model hop, speaker), the real run: every switch of the script, known from the dry run
        if not self.dry:
            self.pending = sorted((self.sched.eff[i], e[3]) for i, e in enumerate(case.events) if e[1] == "spk" and e[2] == s)
        self.err = None
        self.issued = 0          # switches whose call has come
        self.witness = {}        # global call index of a transition -> dict
        self.out = []            # per global call: this stream's mono output block

    # -- the hop callback ------------------------------------------------------------------------------------------------------------
    def _hop(self, in160, out240, _u):
        try:
            self._hop_body(in160, out240)
        except BaseException as e:      # (ctypes would print it and go on)
            self.err = self.err or e
            C.memset(out240, 0, 240 * 4)

    def _hop_body(self, in160, out240):
        i = self.n_fired
        self.n_fired += 1
        self.seg_f += 1
        if self.dry or not self.sched.reach[i]:
            C.memset(out240, 0, 240 * 4)
            return
        while self.pending and self.pending[0][0] <= self.n_model:
            self.model.set_target_speaker(self.pending.pop(0)[1])
        o = self.model.hop(np.ctypeslib.as_array(in160, (160,)).copy())
        C.memmove(out240, o.ctypes.data, 240 * 4)
        self.n_model += 1

    # -- segments --------------------------------------------------------------------------------------------------------------------
    def _close_segment(self, op_index, keep_all=False):
        full = self.seg_f if keep_all else self.seg_H * (self.seg_f // self.seg_H)
        if self.dry:
            self.sched.reach.extend([True] * full + [False] * (self.seg_f - full))
            self.sched.dropped[op_index] = self.seg_f - full
            self.sched.owed[op_index] = sum(1 for last in self.seg_calls if last >= full)
        self.seg_base += full
        self.seg_f, self.seg_calls = 0, []

    def _restart(self, rate, fresh=False):
        if self.p is None:
            self.p, self.rate = self.wl.f_create(float(rate), self.cb, None), float(rate)
            return
        if fresh:    # (a control: the gains restarted too -- a new processor that is told the targets)
            gi, _a, go, _b = self.wl.gain_state(self.p)
            self.wl.f_destroy(self.p)
            self.p = self.wl.f_create(float(rate), self.cb, None)
            self.wl.f_in_gain(self.p, gi)
            self.wl.f_out_gain(self.p, go)
        elif float(rate) == self.rate:
            self.wl.f_set_rate(self.p, OTHER_RATE)
            self.wl.f_set_rate(self.p, float(rate))
        else:
            self.wl.f_set_rate(self.p, float(rate))
        self.rate = float(rate)

    def _process(self, x):
        y = np.zeros_like(x)
        assert self.wl.f_process(self.p, x.ctypes.data_as(wrapperlib._f32p), y.ctypes.data_as(wrapperlib._f32p), len(x)) == 0
        return y

    def _last_hop(self):
        """the newest hop of the segment that the call just made needs for its block (the FIFO hands a hop's samples out one block later)"""
        return (480 * self.seg_f + self.wl.f_fifo_fill(self.p) - 1) // 480 - 1

    # -- the walk --------------------------------------------------------------------------------------------------------------------
    def run(self, stop_after_call=None):
        case, s = self.case, self.s
        sig = None if self.dry else case.signal(s)
        pos = c = 0
        ev = 0
        trans = {i: (j, T) for i, j, T in case.transitions}
        ctl_at, ctl_kind = self.control if self.control else (None, None)
        block = None
        oi = 0
        while oi < len(case.ops):
            op = case.ops[oi]
            if oi in trans:
                self._witness(trans[oi][1])
            in_ctl = ctl_at is not None and any(i <= oi < j and T == ctl_at for i, j, T in case.transitions)
            kind = op[0]
            if kind in CALLS:
                for _ in range(op[1]):
                    if stop_after_call is not None and c >= stop_after_call:
                        if self.err:
                            raise self.err
                        return self
                    _mode, blocks, ch = case.calls[c]
                    n = blocks[s]
                    if self.p is None:
                        self._restart(48000.0)     # (the 48 kHz family: no configure call)
                    while ev < len(case.events) and case.events[ev][0] <= c:
                        self._event(ev, case.events[ev])
                        ev += 1
                    if case.hole(c, s):      # (nothing of the stream moves)
                        if not self.dry:
                            self.out.append(None)
                    elif n > 0:
                        x = np.zeros(n, np.float32) if self.dry else case.mono(sig, pos, n, ch)
                        y = np.concatenate([self._process(x[k:k + 480]) for k in range(0, n, 480)]) if kind == "f" else self._process(x)
                        self.seg_calls.append(self._last_hop())
                        if not self.dry:
                            self.out.append(y)
                    elif not self.dry:
                        self.out.append(np.zeros(0, np.float32))
                    pos += n
                    c += 1
            elif kind in ("cfg", "cfgr"):
                rate = op[1] if kind == "cfg" else op[1][s]
                changes = self.rate is not None and float(rate) != self.rate
                self._close_segment(oi)
                if not (in_ctl and ctl_kind == "carried" and not changes):
                    self._restart(rate, fresh=in_ctl and ctl_kind == "fresh")
                self.seg_H = 1
            elif kind in ("bind", "unbind", "bindr", "unbindr"):
                self._close_segment(oi)
                if not (in_ctl and ctl_kind == "carried"):
                    self._restart(self.rate)
                self.seg_H = case.H if kind == "bind" else 1
                if kind == "bind":
                    block = op[1]
            elif kind in ("bind48", "unbind48"):
                if self.p is None:
                    self._restart(48000.0)
                elif in_ctl and ctl_kind == "restarted":
                    self._restart(48000.0)
            elif kind == "rule":
                pass
            elif kind == "flush":
                fed =self.seg_H * (self.seg_f // self.seg_H)
                owed = bool(self.seg_calls) and self.seg_calls[-1] >= fed
                need = (self.seg_calls[-1] // self.seg_H + 1) * self.seg_H if owed else fed
                if not owed:
                    if self.dry:
                        self.sched.made_up[oi], self.sched.flush_kind[oi], self.sched.owed[oi], self.sched.dropped[oi] = 0, "noop", 0, 0
                    if in_ctl and ctl_kind == "restarted":
                        self._close_segment(oi)
                        self._restart(self.rate)
                else:
                    made = 0
                    while self.seg_calls[-1] >= self.seg_H * (self.seg_f // self.seg_H):
                        self._process(np.zeros(block, np.float32))
                        made += 1
                        assert made < 64 * self.seg_H
                    full, left = self.seg_H * (self.seg_f // self.seg_H), self.seg_f % self.seg_H
                    if self.dry:
                        self.sched.made_up[oi] = made
                        self.sched.flush_kind[oi] = "over_leftover" if left else ("over_full" if full > need else "exact")
                    self._close_segment(oi, keep_all=in_ctl and ctl_kind == "all_hops")
                    if self.dry:
                        self.sched.owed[oi] = 0
                    if not (in_ctl and ctl_kind == "carried"):
                        self._restart(self.rate)
            else:
                raise ValueError(op)
            oi += 1
        self._close_segment(len(case.ops))
        if self.err:
            raise self.err
        return self

    def _event(self, index, e):
        _c, kind, s, value = e
        if s != self.s:
            return
        if kind == "gin":
            self.wl.f_in_gain(self.p, value)
        elif kind == "gout":
            self.wl.f_out_gain(self.p, value)
        elif kind == "spk":
            if self.dry:
                self.sched.eff[index] = self.seg_base + self.seg_H * (self.seg_f // self.seg_H)
            self.issued += 1
            self.target = value
        elif kind == "reset":
            assert self.case.family48 and self.seg_f % self.seg_H == 0
            self._restart(self.rate)
            if not self.dry:
                n_spk = sum(1 for e in self.case.events if e[1] == "spk" and e[2] == self.s)
                while n_spk - len(self.pending) < self.issued:      # (a switch whose step has not come: the reset installs its speaker whole)
                    self.pending.pop(0)
                self.model.close()
                self.model = self.new_model(self.target)

    def _witness(self, T):
        if self.dry:
            self.sched.fill[T] = self.wl.f_fifo_fill(self.p)
            return
        gi_t, gi_n, go_t, go_n = self.wl.gain_state(self.p)
        n_spk = sum(1 for e in self.case.events if e[1] == "spk" and e[2] == self.s)
        applied = n_spk - len(self.pending)
        self.witness[T] = {"fill": self.wl.f_fifo_fill(self.p), "gin": (gi_t, gi_n), "gout": (go_t, go_n),
                           "kv_pending": (N_KV - self.model.kv_count) + N_KV * (self.issued - applied), "knn": self.case.vq_k(self.s) > 0,
                           "hops_before": self.n_model}

    def close(self):
        if self.p is not None:
            self.wl.f_destroy(self.p)
            self.p = None
        if self.model is not None:
            self.model.close()
            self.model = None


def dry_run(case, s, wl=None, control=None):
    w = _Walk(case, s, wl or wrapperlib.oracle_wrapper(), control=control).run()
    w.close()
    return w.sched


def control_kind(case, s, T, sched):
    """The opposite contract at transition T for stream s, or None where the transition cannot be told from its opposite (module docstring)."""
    i, j, _T = next(t for t in case.transitions if t[2] == T)
    kinds = [op[0] for op in case.ops[i:j]]
    if "bind48" in kinds or "unbind48" in kinds:
        return "restarted"
    rate = None     # the stream's rate before the transition
    for op in case.ops[:i]:
        if op[0] == "cfg":
            rate = float(op[1])
        elif op[0] == "cfgr":
            rate = float(op[1][s])
    for op in case.ops[i:j]:
        if op[0] in ("cfg", "cfgr") and float(op[1] if op[0] == "cfg" else op[1][s]) != rate:
            return "fresh"
    if kinds == ["flush"]:
        return "restarted" if sched.flush_kind[i] == "noop" else "carried"
    return "carried"


def yardstick(bv, oracle_models, case, streams=None, control=None, stop_after_call=None, scheds=None):
    """-> {s: _Walk} after the run: .out (per call, the stream's mono block), .witness (per transition), .sched"""
    wl = wrapperlib.oracle_wrapper()
    res = {}
    for s in (range(case.B) if streams is None else streams):
        sched = scheds[s] if scheds else dry_run(case, s, wl)
        def new_model(speaker, s=s):
            return bv.Stream1(oracle_models, speaker=speaker, vq_k=case.vq_k(s))
        ctl = None
        if control is not None:
            ctl = (control[0], control[1] if control[1] else control_kind(case, s, control[0], sched))
            if ctl[1] == "all_hops":      # (other hops reach the model: the control's own dry run)
                sched = dry_run(case, s, wl, control=ctl)
        w = _Walk(case, s, wl, model=new_model(s % 3), sched=sched, control=ctl, new_model=new_model)
        try:
            w.run(stop_after_call)
        finally:
            w.close()
        res[s] = w
    return res


def hop_aligned(case, T):
    """Per stream: True where the calls in front of transition T bring whole hops (48 kHz blocks of 480; 441 samples at 44.1 kHz): the FIFO
    is then empty after every call and cannot be part filled at the transition, whatever the case plants."""
    if case.family48:
        return [True] * case.B
    rate = None
    c = 0
    for op in case.ops:
        if op[0] == "cfg":
            rate = [float(op[1])] * case.B
        elif op[0] == "cfgr":
            rate = [float(r) for r in op[1]]
        elif op[0] in ("io", "g", "rag", "p"):
            c += op[1]
        if c >= T:
            break
    _m, blocks, _ch = case.calls[T - 1]
    return [(b * 48000.0) % (480.0 * r) == 0.0 for b, r in zip(blocks, rate)]


def compared_calls(case, sched):
    """Global call indices whose block is compared: all but the calls owed at an unbind / re-bind without a flush (H > 1)."""
    skip = set()
    c = 0
    for oi, op in enumerate(case.ops):
        if op[0] in CALLS:
            c += op[1]
        elif op[0] in ("bind", "unbind"):
            skip.update(range(c - sched.owed.get(oi, 0), c))
    return [k for k in range(case.n_calls) if k not in skip], sorted(skip)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def _find_flush(make, kinds, lo, tries=40):
    """The first phase length n >= lo at which a dry run finds the flush sub-cases `kinds` (one per flush op of make(n), None = any)."""
    for n in range(lo, lo + tries):
        case = make(n)
        sched = dry_run(case, 0)
        got = [sched.flush_kind[oi] for oi, op in enumerate(case.ops) if op[0] == "flush"]
        if all(k is None or k == g for k, g in zip(kinds, got)):
            return case
    raise AssertionError("no phase length in [%d, %d) gives the flush sub-cases %s" % (lo, lo + tries, kinds))


def _find(make, pred, lo, tries=40):
    """The first phase length n >= lo whose case a dry run accepts."""
    for n in range(lo, lo + tries):
        case = make(n)
        if pred(dry_run(case, 0)):
            return case
    raise AssertionError("no phase length in [%d, %d) gives the case what it is about" % (lo, lo + tries))


def u1(rate, block, ch, B, seed):
    n_io, n_g = calls_for(rate, block), calls_for(rate, block, 1, True)
    return Case("U1-%d-%d-%dch" % (rate, block, ch), B, 1,
                [("cfg", rate), ("io", n_io, block, ch), ("bind", block, ch, 0), ("g", n_g), ("unbind",), ("io", n_io, block, ch)], seed).plant()


def u2(rate, block, ch, B, H, kinds, seed):
    lo = calls_for(rate, block, H, True)
    return _find_flush(lambda n: Case("U2-%d-%d-H%d-%s" % (rate, block, H, "-".join(k or "any" for k in kinds)), B, H,
                                      [("cfg", rate), ("bind", block, ch, 0), ("g", n), ("flush",), ("g", lo), ("flush",), ("unbind",)],
                                      seed, kinds).plant(), kinds, lo)


def u3(rate, block, block2, ch, B, H, seed):
    # (several hops per step: the re-bind finds a step part filled, so that a switch made just before it has installs still to come)
    return _find(lambda n: Case("U3-%d-%d-%d-H%d" % (rate, block, block2, H), B, H,
                                [("cfg", rate), ("bind", block, ch, 0), ("g", n), ("bind", block2, ch, 1),
                                 ("g", calls_for(rate, block2, H, True))] + ([("flush",)] if H > 1 else []) + [("unbind",)], seed).plant(),
                 lambda sched: H == 1 or sched.dropped[3] > 0, calls_for(rate, block, H, True))


def u4_in_order(B, seed):
    a = calls_for(44100, 400)      # (24 blocks of 500 samples at 48 kHz are 25 whole hops: a length that leaves the FIFO part filled)
    return _find(lambda b: Case("U4-in-order", B, 1, [("cfg", 44100), ("io", a, 400, 1), ("cfg", 48000), ("io", b, 500, 1), ("cfg", 44100),
                                                      ("io", a, 400, 1)], seed).plant(),
                 lambda sched: all(0 < f < 480 for f in sched.fill.values()), calls_for(48000, 500))


def u4_bound(B, H, seed):
    a, b = calls_for(44100, 400, H, True), calls_for(48000, 500, H, True)
    return _find(lambda n: Case("U4-bound-H%d" % H, B, H, [("cfg", 44100), ("bind", 400, 1, 0), ("g", n), ("unbind",), ("cfg", 48000),
                                                           ("bind", 500, 1, 0), ("g", b), ("flush",), ("unbind",)], seed).plant(),
                 lambda sched: sched.dropped[3] > 0, a)      # (the unbind finds a step part filled: U3)


def u5(seed):
    rates = [44100.0, 48000.0, 96000.0, 32000.0, 16000.0]
    blocks = [400, 500, 1000, 300, 333]
    n = calls_for(44100, 400)
    n_r = max(int(math.ceil((MIN_HOPS + 1) / hops_per_call(r, b))) + 1 for r, b in zip(rates, blocks))
    return Case("U5-uniform-ragged-uniform", 5, 1, [("cfg", 44100), ("io", n, 400, 2), ("cfgr", rates), ("rag", n_r, blocks, 2), ("cfg", 44100),
                                                     ("io", n, 400, 2)], seed).plant()


R_RATES = [44100.0, 48000.0, 96000.0, 32000.0, 16000.0]
R_BLOCKS = [441, 480, 1024, 512, 333]      # (tests/test_gpu_wrapper_tick_ragged.py's block lengths at these rates)


def _r_calls(bound):
    n = max(int(math.ceil((MIN_HOPS + 3) / hops_per_call(r, b))) + 1 for r, b in zip(R_RATES, R_BLOCKS)) + 2     # (+ the calls a stream sits out)
    return max(n, MAX_STAGES + 3) if bound else n


def r1(ch, seed):
    return Case("R1-%dch" % ch, 5, 1, [("cfgr", R_RATES), ("rag", _r_calls(False), R_BLOCKS, ch, 1), ("bindr", R_BLOCKS, ch, 0), ("p", _r_calls(True)),
                                       ("unbindr",), ("rag", _r_calls(False), R_BLOCKS, ch, 1)], seed, holes=True).plant()


def r2(ch, seed):
    return Case("R2-%dch" % ch, 5, 1, [("cfgr", R_RATES), ("bindr", R_BLOCKS, ch, 1), ("p", _r_calls(True)), ("flush",), ("p", _r_calls(True)),
                                       ("unbindr",)], seed, holes=True).plant()


def r3(ch, seed):
    """P -> G -> P with each binding left through the OTHER form's call, and the wrapper configured anew between them (a binding needs its
    own form's configure call: the A column of MODES)."""
    # (G at 48 000 Hz: stream 1 keeps its rate -- the control "carried" -- and stream 0, which no call leaves out, changes it -- "fresh")
    n_p, n_g = _r_calls(True), calls_for(48000, 500, 1, True)
    return Case("R3-%dch" % ch, 5, 1, [("cfgr", R_RATES), ("bindr", R_BLOCKS, ch, 0), ("p", n_p), ("unbindr", "cross"), ("cfg", 48000),
                                       ("bind", 500, ch, 0), ("g", n_g), ("unbind", "cross"), ("cfgr", R_RATES), ("bindr", R_BLOCKS, ch, 1),
                                       ("p", n_p), ("unbindr",)], seed, holes=True).plant()


def f3(ch, B, seed):
    """S -> F with the rule -> S.  MODES refuses BeatriceBatch_BindResidentIO48k in S, and in F the rule is enabled after entering the mode;
    leaving F ends a rule that was enabled there."""
    n = MIN_HOPS + 4      # (two calls of every phase's ends may be silent)
    return Case("F3-%dch" % ch, B, 1, [("rule", 1), ("io48", n, ch), ("rule", 0), ("bind48", ch, 0), ("rule", 1), ("f", MAX_STAGES + 3),
                                       ("unbind48",), ("rule", 1), ("io48", n, ch)], seed, holes=True).plant()


def f4(ch, B, H, seed):
    n = MIN_HOPS + 2
    head = [("io48", n, ch)] if H == 1 else []      # (the in-order 48 kHz blocks are one hop per step)
    return Case("F4-%dch-H%d" % (ch, H), B, H, head + [("bind48", ch, 0), ("f", MAX_STAGES + 3), ("bind48", ch, 1), ("f", MAX_STAGES + 3), ("unbind48",)] +
                ([("io48", n, ch)] if H == 1 else []), seed, resets=True).plant()


def f1(ch, B, seed):
    n = MIN_HOPS + 1
    return Case("F1-%dch" % ch, B, 1, [("io48", n, ch), ("bind48", ch, 0), ("f", MAX_STAGES + 3), ("unbind48",), ("io48", n, ch)], seed).plant()


def f2(ch, B, H, seed):
    n = max(MAX_STAGES + 3, (MIN_HOPS + H) // H + 1)
    return Case("F2-%dch-H%d" % (ch, H), B, H, [("bind48", ch, 0), ("f", n), ("bind48", ch, 1), ("f", n), ("unbind48",)], seed).plant()


def all_cases():
    # (a case's time is the yardstick's: model hops x streams on the CPU.  The cases of four hops per step, whose bound phases have to
    #  cover a delay of some 110 hops, run two streams: one with k-NN and one without, the two that the controls use)
    cases = [u1(44100, 441, 1, 3, 1), u1(48000, 480, 2, 4, 2), u1(44100, 64, 1, 2, 3), u1(32000, 1000, 2, 2, 4),
             u2(44100, 441, 1, 3, 2, ("noop", None), 5), u2(48000, 480, 2, 2, 4, ("noop", None), 6),
             u2(44100, 441, 1, 2, 4, ("exact", None), 7), u2(44100, 64, 1, 3, 2, ("exact", None), 8),
             u2(32000, 1000, 2, 3, 2, ("over_leftover", None), 9), u2(32000, 1000, 2, 3, 2, ("over_full", None), 10),
             u3(44100, 300, 441, 1, 3, 1, 11), u3(44100, 512, 441, 1, 2, 4, 12),
             u4_in_order(3, 13), u4_bound(2, 4, 14), u5(15), r1(1, 21), r1(2, 22), r2(2, 23),
             f1(1, 3, 16), f1(2, 4, 17), f2(2, 3, 1, 18), f2(1, 3, 2, 19), f2(2, 2, 4, 20),
             r3(2, 24), f3(2, 4, 25), f4(2, 4, 1, 26), f4(1, 4, 2, 27)]
    return cases


# ---- the product's side (needs a GPU) ----------------------------------------------------------------------------------------------------
SENTINEL = np.float32(-777.25)


class HipFailure(Exception):
    """an entry point returned -2 (HIP failure): whoever drives the GPU starts nothing more on it"""


def _rc(rc, want=0):
    if rc == -2:
        raise HipFailure("an entry point returned -2")
    assert rc == want, rc


def run_product(bv, models, case, scheds):
    """The batch through the case's ops.  -> got[c][s] = [channels][n] for every call c whose block the header says is produced (None for
    the calls owed at an unbind / re-bind without a flush).  Resident slots that no call of a chunk may touch are held against a sentinel."""
    from tick_driver import Hip
    hip = Hip()
    B, H = case.B, case.H
    batch = bv.Batch(models, B, hops_per_step=H)
    a, h = batch.a, batch.h
    for s in range(B):
        _rc(a.BeatriceBatch_SetTargetSpeaker(h, s, s % 3))
        _rc(a.BeatriceBatch_SetVQNumNeighbors(h, s, case.vq_k(s)))
    _rc(a.BeatriceBatch_FlushSpeaker(h, -1))
    stages = a.BeatriceBatch_TickStages(h)
    assert stages <= MAX_STAGES, "the cases' phase lengths are laid out for at most %d tick stages" % MAX_STAGES
    sigs = [case.signal(s) for s in range(B)]
    pos = [0] * B
    got = [None] * case.n_calls
    ev = 0
    c = 0
    bufs = []
    bind = None      # the present binding: dict

    def apply_events(c):
        nonlocal ev
        while ev < len(case.events) and case.events[ev][0] <= c:
            _c, kind, s, value = case.events[ev]
            if kind == "reset":
                _rc(a.BeatriceBatch_ResetStream(h, s))
            else:
                fn = {"gin": a.BeatriceBatch_SetInputGain, "gout": a.BeatriceBatch_SetOutputGain, "spk": a.BeatriceBatch_SetTargetSpeaker}[kind]
                _rc(fn(h, s, value))
            ev += 1

    def block_in(c):
        _m, blocks, ch = case.calls[c]
        out = []
        for s in range(B):
            out.append(np.ascontiguousarray(sigs[s][:ch, pos[s]:pos[s] + blocks[s]]))
            pos[s] += blocks[s]
        return out

    def collect(upto):
        """the blocks of the binding's calls [have, upto) are out: read them from their slots"""
        bd = bind
        out = np.zeros(bd["shape"], np.float32)
        hip.d2h(out, bd["d_out"])
        written = set()
        for k in range(bd["have"], upto):
            if bd.get("ragged"):
                cells = []
                for s in range(B):
                    n = bd["blocks"][s]
                    if case.hole(bd["c0"] + k, s):      # (no block: the cell is the caller's, nothing was written into it)
                        assert np.all(out[k % bd["slots"], s] == SENTINEL), "%s: call %d wrote the cell of stream %d, which sat it out" % (case.name, bd["c0"] + k, s)
                        cells.append(None)
                    else:
                        cells.append(out[k % bd["slots"], s, :bd["ch"] * n].reshape(bd["ch"], n).copy())
                        assert np.all(out[k % bd["slots"], s, bd["ch"] * n:] == SENTINEL)
                got[bd["c0"] + k] = cells
            else:
                cells = [out[k % bd["slots"], s].reshape(bd["ch"], -1).copy() if not bd["f48"] else
                         np.concatenate([out[k % bd["slots"], s, hh] for hh in range(H)], axis=1) for s in range(B)]
                for s in range(B):
                    if case.hole(bd["c0"] + k, s):      # (F with the rule: a flagged stream's blocks "come back as their own down-mix")
                        assert np.all(cells[s] == 0.0), "%s: call %d, the silent block of stream %d" % (case.name, bd["c0"] + k, s)
                        cells[s] = None
                got[bd["c0"] + k] = cells
            written.add(k % bd["slots"])
        for sl in range(bd["slots"]):     # a slot that no call of this chunk owns still holds the sentinel: nothing was written elsewhere
            if sl not in written:
                assert np.all(out[sl] == SENTINEL), "%s: output slot %d was written by no call of the chunk" % (case.name, sl)
        bd["have"] = upto
        hip.h2d(bd["d_out"], np.full(bd["shape"], SENTINEL, np.float32))     # (drained: nothing is in flight)

    def bound_calls(n):
        """n calls of the binding: chunks that fit the slot ring, each uploaded (every other input slot poisoned), run, drained, collected"""
        nonlocal c
        bd = bind
        done = 0
        assert n > bd["delay"], "%s: a bound phase of %d calls does not cover the binding's delay of %d" % (case.name, n, bd["delay"])
        while done < n:
            nk = min(bd["chunk"], n - done)
            buf = np.full(bd["shape"], np.nan, np.float32)
            for k in range(bd["k"], bd["k"] + nk):
                blk = block_in(bd["c0"] + k)
                for s in range(B):
                    if bd.get("ragged"):
                        if not case.hole(bd["c0"] + k, s):
                            buf[k % bd["slots"], s, :blk[s].size] = blk[s].reshape(-1)
                    elif bd["f48"]:
                        buf[k % bd["slots"], s] = 0.0 if case.hole(bd["c0"] + k, s) else blk[s].reshape(bd["ch"], H, 480).transpose(1, 0, 2)
                    else:
                        buf[k % bd["slots"], s] = blk[s]
            hip.h2d(bd["d_in"], buf)
            for k in range(bd["k"], bd["k"] + nk):
                apply_events(c)
                if bd.get("ragged"):
                    ns = (C.c_int * B)(*[0 if case.hole(c, s) else bd["blocks"][s] for s in range(B)])
                    _rc(a.BeatriceBatch_ProcessBlocksRaggedDevice(h, ns))
                elif bd["f48"]:
                    if any(case.hole(c, s) for s in range(B)):      # (the caller flags the streams whose next blocks are silent)
                        _rc(a.BeatriceBatch_SetSilentStreams(h, bytes(1 if case.hole(c, s) else 0 for s in range(B))))
                    _rc(a.BeatriceBatch_ConvertBlocks48kDevice(h, None, None, bd["ch"]))
                else:
                    _rc(a.BeatriceBatch_ProcessBlocksDevice(h, None, None, bd["ch"], bd["n"]))
                c += 1
            bd["k"] += nk
            done += nk
            if done < n:      # (the last chunk of a phase is left in flight: the transition that follows has to drain it)
                _rc(a.BeatriceBatch_Synchronize(h))
                owed = 0 if bd["f48"] else a.BeatriceBatch_ResidentBlocksOwed(h)
                assert not bd.get("ragged") or owed == 0
                assert owed >= 0 and (H > 1 or owed == 0)
                collect(bd["k"] - owed)

    def new_binding(f48, ch, n, pick, blocks=None):
        nonlocal bind
        if blocks is not None:
            delay = stages - 1
            slots = delay + 2 + (5 if pick == 0 else 3)
            shape = (slots, B, ch * max(blocks))
        elif f48:
            slots = stages + (5 if pick == 0 else 2)
            shape = (slots, B, H, ch, 480)
            delay = stages - 1
        else:
            delay = a.BeatriceBatch_ResidentBlocksDelayFor(h, n)
            assert delay > 0
            slots = delay + 2 + (5 if pick == 0 else 3)      # a ring shorter than a phase: it wraps
            shape = (slots, B, ch, n)
        nbytes = int(np.prod(shape)) * 4
        d_in, d_out = hip.malloc(nbytes), hip.malloc(nbytes)
        bufs.extend([d_in, d_out])
        hip.h2d(d_out, np.full(shape, SENTINEL, np.float32))
        if blocks is not None:
            _rc(a.BeatriceBatch_BindResidentBlocksRagged(h, d_in, d_out, ch, max(blocks), slots))
            assert a.BeatriceBatch_ResidentBlocksDelay(h) == delay
        elif f48:
            _rc(a.BeatriceBatch_BindResidentIO48k(h, d_in, d_out, ch, slots))
        else:
            _rc(a.BeatriceBatch_BindResidentBlocks(h, d_in, d_out, ch, n, slots))
            assert a.BeatriceBatch_ResidentBlocksDelay(h) == delay
        bind = {"f48": f48, "ch": ch, "n": n, "slots": slots, "shape": shape, "delay": delay, "d_in": d_in, "d_out": d_out,
                "chunk": max(1, slots - delay - 1), "k": 0, "have": 0, "c0": c, "ragged": blocks is not None, "blocks": blocks}

    def end_binding(op_index):
        """after the op that ended (or restarted) the binding: everything but the owed calls is out"""
        owed = 0 if bind["f48"] else scheds[0].owed.get(op_index, 0)
        collect(bind["k"] - owed)

    for oi, op in enumerate(case.ops):
        kind = op[0]
        if kind == "cfg":
            _rc(a.BeatriceBatch_ConfigureWrapper(h, float(op[1])))
        elif kind == "cfgr":
            rates = (C.c_double * B)(*op[1])
            _rc(a.BeatriceBatch_ConfigureWrapperRates(h, rates))
            x = np.zeros((B, 1, 64), np.float32)      # "the uniform entry points above are off until BeatriceBatch_ConfigureWrapper is called again"
            assert a.BeatriceBatch_ProcessBlocks(h, bv.fptr(x), bv.fptr(np.zeros_like(x)), 1, 64) == -1
        elif kind == "io":
            for _ in range(op[1]):
                apply_events(c)
                blk = block_in(c)
                x = np.ascontiguousarray(np.stack(blk))
                y = np.zeros_like(x)
                _rc(a.BeatriceBatch_ProcessBlocks(h, bv.fptr(x), bv.fptr(y), op[3], op[2]))
                got[c] = [y[s] for s in range(B)]
                c += 1
        elif kind == "rag":
            rule = op[4] if len(op) > 4 else 0
            for _ in range(op[1]):
                apply_events(c)
                blk = block_in(c)
                lens = [0 if (c, s) in case.absent else op[2][s] for s in range(B)]
                blk = [np.zeros_like(b) if (c, s) in case.silent else b for s, b in enumerate(blk)]      # (the shell's rule: a block of zeros)
                assert rule or not case.silent
                x = np.ascontiguousarray(np.concatenate([b.reshape(-1) for s, b in enumerate(blk) if lens[s]]))
                y = np.full_like(x, SENTINEL)
                _rc(a.BeatriceBatch_ProcessBlocksRagged(h, bv.fptr(x), bv.fptr(y), op[3], (C.c_int * B)(*lens), rule))
                offs = np.cumsum([0] + [op[3] * n for n in lens])
                cells = [y[offs[s]:offs[s + 1]].reshape(op[3], -1) if lens[s] else None for s in range(B)]
                for s in range(B):
                    if (c, s) in case.silent:      # "its output block is zeros"
                        assert np.all(cells[s] == 0.0), "%s: call %d, the silent block of stream %d" % (case.name, c, s)
                        cells[s] = None
                got[c] = cells
                c += 1
        elif kind == "io48":
            for _ in range(op[1]):
                apply_events(c)
                x = np.stack(block_in(c))
                for s in range(B):
                    if case.hole(c, s):      # (S: the library finds the block of zeros itself)
                        x[s] = 0.0
                y = batch.convert48k(x, op[2])
                got[c] = [y[s] for s in range(B)]
                for s in range(B):
                    if case.hole(c, s):      # "the output is that down-mix"
                        assert np.all(y[s] == 0.0), "%s: call %d, the silent block of stream %d" % (case.name, c, s)
                        got[c][s] = None
                c += 1
        elif kind == "rule":
            _rc(a.BeatriceBatch_EnableSilentBlockRule(h, op[1]))
        elif kind in ("bind", "bind48"):
            if bind is not None:       # footnote 5: the call leaves the mode itself
                old = bind
                new_binding(kind == "bind48", op[2] if kind == "bind" else op[1], op[1] if kind == "bind" else 480, op[-1])
                fresh, bind = bind, old
                end_binding(oi)
                bind = fresh
            else:
                new_binding(kind == "bind48", op[2] if kind == "bind" else op[1], op[1] if kind == "bind" else 480, op[-1])
        elif kind == "bindr":
            assert bind is None
            new_binding(False, op[2], 0, op[3], blocks=list(op[1]))
        elif kind in ("g", "f", "p"):
            bound_calls(op[1])
        elif kind == "flush":
            _rc(a.BeatriceBatch_FlushResidentBlocks(h))
            _rc(a.BeatriceBatch_ResidentBlocksOwed(h))
            collect(bind["k"])
            if scheds[0].flush_kind[oi] != "noop":     # the binding has started over: the next call is call 0 and reads and writes slot 0
                bind["c0"] += bind["k"]
                bind["k"] = bind["have"] = 0
        elif kind in ("unbind", "unbindr"):      # ("either bind call unbinds either form")
            if (kind == "unbindr") != (len(op) > 1 and op[1] == "cross"):
                _rc(a.BeatriceBatch_BindResidentBlocksRagged(h, None, None, 0, 0, 0))
            else:
                _rc(a.BeatriceBatch_BindResidentBlocks(h, None, None, 0, 0, 0))
            end_binding(oi)
            bind = None
        elif kind == "unbind48":
            _rc(a.BeatriceBatch_BindResidentIO48k(h, None, None, 0, 0))
            end_binding(oi)
            bind = None
    assert c == case.n_calls and bind is None
    batch.close()
    for p in bufs:
        hip.free(p)
    return got
