"""The shell's silent-block test (reference src/vst/processor.cc:183-214) in numpy float32: the yardstick of the device scan
(BeatriceBatch_ScanSilentBlocks*).  Test plumbing only; no HIP.  tests/test_cpu_silent_scan_abi.py holds it against the flag that
ProcessorProxy::ProcessChannels returns, on the CPU, before anything runs on a GPU."""
import numpy as np

TINY = np.float32(1.401298464324817e-45)   # the smallest positive float32 subnormal


def shell_silent(block):
    """block: [n] or [channels, n] float32, channels 1 or 2 -> 1 when no sample of the down-mix (x, or (x0 + x1) * 0.5f) differs from
    0.0f -- so NaN and Inf are loud, -0.0 and L = -R silent, a block of no samples silent."""
    x = np.asarray(block, np.float32)
    if x.ndim == 1:
        x = x[None]
    assert x.ndim == 2 and x.shape[0] in (1, 2)
    with np.errstate(all="ignore"):
        m = x[0] if x.shape[0] == 1 else (x[0] + x[1]).astype(np.float32) * np.float32(0.5)
    assert m.dtype == np.float32
    return 0 if bool(np.any(m != np.float32(0.0))) else 1


def edge_table(n, channels):
    """[(name, block [channels, n])]: the contents every shape of the edge-table tests is run with."""
    big = np.float32(3.0e38)
    z = lambda: np.zeros((channels, n), np.float32)
    rows = [("all +0", z()), ("all -0", -z())]

    def one(name, ch, i, v):
        b = z()
        b[ch, i] = v
        rows.append((name, b))

    one("tiny at 0", 0, 0, TINY)
    one("tiny at n-1", 0, n - 1, TINY)
    one("3 x tiny at n-1", 0, n - 1, np.float32(3) * TINY)
    one("nan", 0, n // 2, np.float32(np.nan))
    one("inf", 0, n - 1, np.float32(np.inf))
    one("1.0 in channel 0", 0, n // 3, np.float32(1.0))
    if channels == 2:
        one("tiny in channel 1 only", 1, 0, TINY)            # halves to 0 under round-to-even: silent
        one("3 x tiny in channel 1 only", 1, n - 1, np.float32(3) * TINY)
        one("1.0 in channel 1", 1, n - 1, np.float32(1.0))
        one("nan in channel 1", 1, 0, np.float32(np.nan))
        b = z()
        b[0] = np.linspace(-1.0, 1.0, n, dtype=np.float32)
        b[0, 0] = 0.25
        b[1] = -b[0]
        rows.append(("L = -R", b))
        b = z()
        b[0, n - 1] = big
        b[1, n - 1] = big
        rows.append(("sum overflows", b))
        b = z()
        b[0, 0] = TINY
        b[1, 0] = TINY      # 2 x tiny halves to tiny: loud
        rows.append(("tiny in both channels", b))
    return rows
