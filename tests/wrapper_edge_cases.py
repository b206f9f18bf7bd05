"""The any-rate wrapper at the rate and block classes its kernels branch on: ONE table for the CPU witness
(tests/test_cpu_wrapper_edge_rates.py), the yardstick's pin (tests/test_wrapper_oracle.py, tests/test_cpu_wrapper_plan.py) and the
GPU parity file (tests/test_gpu_wrapper_edge_rates.py).  Plain data plus the class of every case, computed here from the rules of
beatrice-vst_amd/csrc/wrapper_plan.h (fraction, n_taps, hist, direction, longest_block); the CPU witness derives the same quantities
through the compiled header and fails where one differs.

The four kernel forms (csrc/wrapper.hip.h):
  1  uniform in order            wrap_in_kernel / wrap_out_kernel         ConfigureWrapper + ProcessBlocks
  2  uniform around the ticks    wrap_call_kernel with its post half      BindResidentBlocks (one block length per binding)
  3  per-stream clocks in order  wrapr_in_kernel / wrapr_out_kernel       ConfigureWrapperRates + ProcessBlocksRagged
  4  per-stream clocks, ticks    wrapr_call_kernel / wrapr_post_kernel    BindResidentBlocksRagged
"""
import math

import numpy as np

INNER = 48000.0
TAPS_PER_OUTPUT, BLOCK, MAX_SAMPLES, MAX_CHUNKS, MAX_HIST, TAPS_LDS = 32, 480, 4096, 12, 32 * 8 + 1, 7168

# rate -> the fraction stated for it (checked against simple_fraction below and against the compiled header by the witness)
RATES = {
    384000.0: (8, 1), 6000.0: (8, 1),
    192000.0: (4, 1), 12000.0: (4, 1), 8000.0: (6, 1),
    176400.0: (147, 40),
    11025.0: (640, 147), 22050.0: (320, 147),
    47952.0: (999, 998), 44056.0: (572, 525),
    47784.75: (223, 222), 47785.75: (224, 223),
    48048.0: (1, 1),
    48000.0: (1, 1),
}
CLASSES = ("ratio8_above", "ratio8_below", "ratio4_6", "large_hi_lds", "global_exact", "global_truncated", "edge_last_lds", "edge_first_global",
           "truncated_to_unity")
REFUSED_RATES = {5900.0: 261, 5000.0: 308, 390000.0: 261, 400000.0: 267}   # rate -> the history it would need (> 257)


def simple_fraction(ratio):
    """wrapper_plan.h simple_fraction: smallest-denominator search on the Stern-Brocot tree, parts < 1000"""
    a, b, c, d = 0, 1, 1, 0
    while True:
        mn, md = a + c, b + d
        big = mn >= 1000 or md >= 1000
        if ratio * md < mn:
            if big:
                return a, b
            c, d = mn, md
        else:
            if big:
                return c, d
            a, b = mn, md


class Rate:
    """what RateClass::configure fixes for a host rate"""

    def __init__(self, rate):
        self.rate = float(rate)
        self.high_is_outer = self.rate >= INNER
        high, low = (self.rate, INNER) if self.high_is_outer else (INNER, self.rate)
        self.exact = high / low
        self.hi, self.lo = simple_fraction(high / low)
        self.n_taps = TAPS_PER_OUTPUT * self.hi + 1
        self.hist = TAPS_PER_OUTPUT * self.hi // self.lo + 1
        self.accepted = self.hi > 0 and self.lo > 0 and self.hist <= MAX_HIST
        self.taps_in_lds = self.n_taps <= TAPS_LDS
        self.truncated = self.hi * low != self.lo * high          # the fraction is not the ratio
        self.longest = max(1, math.floor((MAX_SAMPLES - 8) * min(1.0, self.rate / INNER)))

    def most_hops(self, n):
        return (math.ceil(n * INNER / self.rate) + 2 + BLOCK - 1) // BLOCK + 1

    def classes(self):
        c = set()
        if (self.hi, self.lo) == (8, 1):
            c.add("ratio8_above" if self.high_is_outer else "ratio8_below")
        if self.lo == 1 and self.hi in (4, 6):
            c.add("ratio4_6")
        if self.lo > 1 and self.hi >= 100 and self.taps_in_lds and self.hist > 97:
            c.add("large_hi_lds")
        if not self.taps_in_lds:
            c.add("global_truncated" if self.truncated else "global_exact")
        if self.n_taps == 32 * 223 + 1:
            c.add("edge_last_lds")
        if self.n_taps == 32 * 224 + 1:
            c.add("edge_first_global")
        if self.truncated and (self.hi, self.lo) == (1, 1):
            c.add("truncated_to_unity")
        return c


class Clocks:
    """wrapper_plan.h plan_clocks: the two fractional clocks and the FIFO fill of one stream -> per call (inner samples, pieces)"""

    def __init__(self, r):
        self.r, self.down, self.up, self.fill = r, r.hi - 1, r.hi - 1, 0

    def call(self, n):
        r = self.r
        if r.high_is_outer:
            total = self.down + n * r.lo
            m, self.down = total // r.hi, total % r.hi
        else:
            m = ((n + 1) * r.hi - self.up - 1) // r.lo
            self.up = (self.up + m * r.lo) % r.hi
        pieces, at, fill = 0, 0, self.fill
        while at < m:
            take = min(BLOCK - fill, m - at)
            fill = 0 if fill + take == BLOCK else fill + take
            at += take
            pieces += 1
        self.fill = fill
        if r.high_is_outer:
            out = (m * r.hi + self.down - self.up) // r.lo
            self.up = (self.up + out * r.lo) % r.hi
        else:
            total = self.down + m * r.lo
            out, self.down = total // r.hi, total % r.hi
        assert out == n, (r.rate, n, out)
        return m, pieces


# ---- block scripts ---------------------------------------------------------------------------------------------------------------------------
PRIME = 97


def steady_block(rate):
    return int(round(rate / 100.0))        # 10 ms


def script_blocks(rate, kind):
    """The host block lengths of a case, call by call.
      steady   6 blocks of 10 ms: five model hops behind the FIFO's 10 ms
      ones     n = 1 for 48 consecutive calls between steady blocks (at 384 kHz: seven calls in eight yield no inner sample)
      longest  n = MaxWrapperBlock(rate), three calls in a row (six above 48 kHz, where a block is 10 ms): the history crosses a full buffer
      mixed    1, a prime and the longest block, in turns
      only1    nothing but n = 1: the one script a binding of form 2 (one block length) can run with n = 1; long enough for a hop to come back
    """
    s, L = steady_block(rate), Rate(rate).longest
    if kind == "steady":
        return [s] * 6
    if kind == "ones":
        return [s] * 2 + [1] * 48 + [s] * 4
    if kind == "longest":
        return [L] * (6 if rate > INNER else 3)
    if kind == "mixed":
        return [1, PRIME, L, 1, 1, PRIME, s, L, PRIME, 1, s, s]
    if kind == "only1":
        r = Rate(rate)
        per_call = r.hi / r.lo if not r.high_is_outer else r.lo / r.hi
        return [1] * int(math.ceil((BLOCK + 2.2 * BLOCK) / per_call))     # the FIFO's 10 ms, then two hops' worth of sound
    raise KeyError(kind)


class Case:
    def __init__(self, rate, kind, channels, forms, hops_per_step=(1,), blocks=None, name=None, gains=None):
        self.rate, self.kind, self.channels, self.forms, self.hops_per_step = float(rate), kind, channels, tuple(forms), tuple(hops_per_step)
        self.blocks = list(blocks) if blocks is not None else script_blocks(self.rate, kind)
        self.gains = gains          # stream -> gain events of its own, in place of gain_events()'s
        self.id = name or "%s-%s-%s" % (("%.2f" % self.rate).rstrip("0").rstrip("."), kind, "stereo" if channels == 2 else "mono")

    @property
    def total(self):
        return sum(self.blocks)


def _cases():
    out = []
    long_rates = (6000.0, 11025.0, 48000.0, 384000.0)
    mixed_rates = (384000.0, 6000.0, 47952.0, 22050.0, 176400.0)
    for i, rate in enumerate(RATES):
        if rate == 48000.0:
            continue                                  # (48 kHz is here for the longest block alone)
        # form 2 runs one block length per binding: the steady script; several hops per step at 384 kHz and 11 025 Hz
        out.append(Case(rate, "steady", 2 if i % 2 == 0 else 1, (1, 2, 3, 4), (1, 4) if rate in (384000.0, 11025.0) else (1,)))
        out.append(Case(rate, "ones", 1 if i % 2 == 0 else 2, (1, 3, 4)))
    for rate in long_rates:
        out.append(Case(rate, "longest", 2 if rate in (6000.0, 384000.0) else 1, (1, 2, 3, 4)))
    for rate in mixed_rates:
        out.append(Case(rate, "mixed", 1, (1, 3, 4)))
    for rate in (384000.0, 6000.0):
        out.append(Case(rate, "only1", 1, (2,)))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}

# Mixes for the forms with clocks per stream: stream s of a mix is stream s of the named case (its seed, voice, k-NN setting and gains), so the
# expected samples are those of the uniform case.  One launch then has streams on the LDS and on the global table, with no hop and with
# several hops per call; a stream whose script is over sits the remaining calls out (n = 0).
MIXES = [
    ("ratio8_both_and_global", 1, ((384000.0, "steady"), (6000.0, "steady"), (47952.0, "steady"))),
    ("ratio8_ones", 1, ((384000.0, "ones"), (6000.0, "ones"), (47952.0, "ones"))),
    ("ratio8_longest", 2, ((384000.0, "longest"), (6000.0, "longest"), (11025.0, "longest"))),
    ("ratio8_mixed", 1, ((384000.0, "mixed"), (6000.0, "mixed"), (47952.0, "mixed"))),
    ("ratio4_6", 2, ((192000.0, "steady"), (12000.0, "steady"), (8000.0, "steady"))),
    ("lds_global_edge", 1, ((47784.75, "steady"), (47785.75, "steady"), (176400.0, "steady"))),
    ("global_tables", 2, ((11025.0, "steady"), (22050.0, "steady"), (44056.0, "steady"))),
    ("unity", 1, ((48048.0, "steady"), (48000.0, "longest"), (22050.0, "mixed"))),
    ("second_ones", 2, ((176400.0, "ones"), (11025.0, "ones"), (48048.0, "ones"))),
]


def mix_cases(mix):
    """(name, channels, [Case per stream]) -- the cases looked up by rate and script, whatever channel count the uniform table gives them"""
    name, channels, keys = mix
    cases = []
    for rate, kind in keys:
        found = [c for c in CASES if c.kind == kind and c.rate == rate]
        assert len(found) == 1, (rate, kind)
        cases.append(found[0])
    return name, channels, cases


def cases_of_form(form):
    """the cases a kernel form runs: forms 1 and 2 run every case that names them, one batch per case; forms 3 and 4 run the mixes"""
    if form in (1, 2):
        return [c for c in CASES if form in c.forms]
    seen = []
    for mix in MIXES:
        for c in mix_cases(mix)[2]:
            assert 3 in c.forms and 4 in c.forms, c.id
            if c not in seen:
                seen.append(c)
    return seen


# One stream's SetStreamRateInFlight walk inside a binding of form 4: every leg shorter than the binding's delay, so that the records of the
# rate before are still owed when the next table arrives -- and the tap arena (wrapper_turnover_plan.h) grows from 44.1 kHz's 2 x 5 121
# floats to 47 952 Hz's 2 x 31 969.  (rate, blocks)
TURNOVER_LEGS = [(44100.0, [441] * 8), (47952.0, [480] * 8), (6000.0, [60] * 8), (384000.0, [3840] * 8)]


# ---- the streams of a case ---------------------------------------------------------------------------------------------------------------------
B = 3
VOICE = (0, 1, 2)
KNN = (0, 1, 2)


def seed_of(case, s, channel):
    return 7300 + 31 * sorted(RATES).index(case.rate) + 7 * s + channel + 1000 * ("steady", "ones", "longest", "mixed", "only1").index(case.kind)


def signal(case, s, channels):
    """[channels][total] of stream s; the second channel is another signal at 0.6, so that the down-mix is no copy of either"""
    import wrapperlib
    return np.stack([np.float32(0.6 if c else 1.0) * wrapperlib.test_signal(case.total, int(case.rate), seed=seed_of(case, s, c))
                     for c in range(channels)]).astype(np.float32)


def gain_events(case, s):
    """call -> (input dB or None, output dB or None), set in front of that call.  Stream 1 ramps both gains in both directions from the
    second call on, so that the kernels' amp[] arrays are built at the full length of whatever block follows -- the longest one included;
    stream 2 has a constant gain other than 0 dB from the start (a ramp that ends inside the first block)."""
    if case.gains is not None:
        return case.gains.get(s, {})
    if s == 1:
        ev = {1: (-24.0, 6.0), 2: (3.0, -18.0)}
        if len(case.blocks) > 8:
            ev[len(case.blocks) // 2] = (-9.0, 2.0)
        return ev
    if s == 2:
        return {0: (-3.0, 1.5)}
    return {}
