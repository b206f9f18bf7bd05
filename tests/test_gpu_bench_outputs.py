"""bench.py's plain run and --dump-outputs: the line a plain run prints (the headline and nothing that takes runs of its own), and outputs
that depend on the arguments only -- two runs whose device warm-ups take different numbers of steps dump the same samples."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bench(out_dir, *args):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--dump-outputs", str(out_dir)] + list(args),
                       capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.parametrize("config,extra,name,shape", [
    (2, [], "out24k", (32, 4 * 240)),                      # the headline's form: tick mode, four hops per step, resident slots
    (3, ["--speakers", "4"], "out24k", (32, 4 * 240)),     # speaker switches on a schedule of their own
    (4, [], "out48k", (32, 4, 2, 480)),                    # 48 kHz stereo blocks around the tick pipeline
])
def test_plain_run_and_its_outputs(tmp_path, config, extra, name, shape):
    args = ["--config", str(config), "--streams", "32", "--steps", "7", "--warmup", "3"] + extra
    lines, outs = [], []
    for warm_ms in (100, 400):
        d = tmp_path / ("warm%d" % warm_ms)
        lines.append(_bench(d, *(args + ["--device-warm-ms", str(warm_ms)])))
        assert sorted(os.listdir(d)) == [name + ".npy"]
        outs.append(np.load(d / (name + ".npy")))
    for line in lines:
        assert line["steps"] == 7 and line["warmup"] == 3 and line["unit"] == "frames/s" and line["higher_is_better"] is True
        assert line["dtype"] == "f32" and line["ms_per_step"] > 0
        assert abs(line["value"] - 32 * 4 / (line["ms_per_step"] * 1e-3)) / line["value"] < 0.01
        for k in ("roofline", "cpu_baseline", "host_work_ms_per_step", "steady_state", "kernels"):
            assert k not in line, k
    a, b = outs
    assert a.dtype == np.float32 and a.shape == shape
    assert np.isfinite(a).all() and np.abs(a).max() > 1e-3
    assert np.array_equal(a, b), "max-abs %g" % np.abs(a - b).max()
