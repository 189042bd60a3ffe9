"""
bench.py at a reduced frame size: a plain run prints the headline line and nothing it would need an extra run for;
--dump-outputs writes the maps of the last timed step, which must be the maps a match of the same seeded inputs returns;
--full adds the per-kernel figures and the evaluation-count statistics.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

ROWS, COLS = 96, 128


def _bench(*args):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--rows", str(ROWS), "--cols", str(COLS)] + list(args)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_plain_run_dumps_the_maps_of_the_timed_path(tmp_path):
    d = _bench("--dump-outputs", str(tmp_path))
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "Mpx/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["roofline"] is None and d["cpu_baseline"] is None and "Ncalls_mean" not in d["config"]

    from umpa_amd import model
    from umpa_amd.synth import CONFIGS, make_stack
    cfg = CONFIGS["C2"]
    sam, ref, _ = make_stack(ROWS, COLS, cfg["K"], cfg["max_shift"], df=True, seed=0)
    m = model.UMPAModelDF(sam, ref, window_size=cfg["Nw"], max_shift=cfg["max_shift"], device=0)
    m.debug = False
    want = m.match(quiet=True)
    assert sorted(os.listdir(tmp_path)) == sorted(k + ".npy" for k in ("f", "T", "dx", "dy", "df", "err"))
    for k in ("f", "T", "dx", "dy", "df", "err"):
        got = np.load(tmp_path / (k + ".npy"))
        assert got.dtype == (np.float32 if k == "err" else np.float64) and got.shape == want[k].shape, k
        np.testing.assert_array_equal(got, want[k].astype(got.dtype), err_msg=k)


def test_full_run_adds_the_kernel_figures():
    d = _bench("--full", "--no-cpu")
    assert d["roofline"]["kernel"] in d["roofline"]["kernels_ms"] and d["roofline"]["step"]["ms"] > 0
    assert d["config"]["Ncalls_mean"] > 0 and 0 < d["config"]["err_ok_fraction"] <= 1
