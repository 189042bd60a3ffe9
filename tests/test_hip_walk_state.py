"""
The kernels that inline walk_feed (umpa_amd/csrc/umpa_walk.h), on frames of 45 x 61 with Nw 2: the region is no multiple
of replay_walk's 4 rows or 16 columns, so there are partial blocks on both edges.

Each case (tests/golden/make_golden_walk_state.py defines them) is held
  * to the CPU checker under the suite's parity rules (oracle/parity.py: err and Ncalls exact, the maps to 1e-5) and, for
    the debug arrays d and a, which cells are known and which are NaN exactly, their costs to the same 1e-5 (they are
    sums in another order than the checker's; bit equality is what the second comparison is for), and
  * to tests/golden/walk_state_parent.npz, recorded on the GPU from the commit before walk_feed was rewritten into its
    single-exit form: every byte of every map, NaNs included (the two debug arrays by their SHA-256).
"""
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import assert_parity

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "make_golden_walk_state", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden_walk_state.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

# the route a case must take: last_path (1 match_direct, 2 the tiled path, 3 match_staged)
PATHS = {"tiled": 2, "direct": 1, "staged": 3}


@pytest.fixture(scope="module")
def hip_ns():
    from umpa_amd import _lib, model
    if _lib.hip().device_count() < 1:
        pytest.fail("no HIP device: the GPU tests cannot run (there is no CPU fallback)")
    return model


@pytest.fixture(scope="module")
def parent():
    return np.load(G.GOLDEN)


@pytest.fixture(scope="module")
def strict_ns(tmp_path_factory):
    """The CPU checker (oracle/umpa_oracle.c) once more, compiled WITHOUT -ffast-math.  The suite's build of it may assume
    that no NaN occurs: what `memo[lo] > memo[CENTRE] + TIE` answers for a NaN cost is then the compiler's choice, and
    on a dead patch its walks go where no IEEE evaluation of the same source goes.  Same source, same parity rules."""
    from umpa_amd import _lib, model
    from oracle import cpu_model
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    so = str(tmp_path_factory.mktemp("strict_oracle") / "libumpa_oracle_ieee.so")
    subprocess.run([cc, "-std=c11", "-O2", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared",
                    os.path.join(os.path.dirname(cpu_model.PORT_PATH), "umpa_oracle.c"), "-o", so, "-lm"], check=True)
    native = _lib.Native(so, "umpaor_", False)
    return type("strict", (), {b.__name__: type(b.__name__ + "_strict", (cpu_model._OwnGeometry, b), {"_native": lambda self: native})
                               for b in (model.UMPAModelNoDF, model.UMPAModelDF)})


@pytest.mark.parametrize("case", list(G.CASES))
def test_walk_state(hip_ns, port_ns, strict_ns, parent, case):
    K, df, ms, cap, zero, route, masked = G.CASES[case]
    got, path = G.run(hip_ns, case)
    assert path == PATHS[route], (case, path)
    want, _ = G.run(strict_ns if zero else port_ns, case, hip=False)   # NaN costs: the IEEE build of the checker
    n_ok = int((want["err"] == 1).sum())
    print("%s: %d of %d pixels ok, Ncalls %d .. %d" % (case, n_ok, want["err"].size, want["debug_Ncalls"].min(), want["debug_Ncalls"].max()))
    # the case is what it says: walks that complete, and the early exits it is there for
    if cap is not None:                       # (the cap is only tested after the centre and after a move: some walks pass it)
        assert 0 < n_ok < 0.55 * want["err"].size and want["debug_Ncalls"].max() < 25
    elif ms == 2:                             # shifts -1 .. 1: no 4x4 neighbourhood fits, every walk ends on the bound
        assert n_ok == 0 and want["debug_Ncalls"].max() > 4
    else:
        assert n_ok > want["err"].size // 2
    if zero:
        assert np.isnan(want["f"]).any() or np.isnan(want["debug_d"]).any()
    assert_parity(got, want, ms, "walk state " + case)
    # the debug arrays.  Which cells of the memo are known (-1 elsewhere) and which are NaN is exact; the costs themselves
    # are sums in another order than the checker's, so they are held to the bar of the maps, 1e-5, with parity.py's rule
    # for costs that cancel to nothing (1e-10 of the largest cost the walk has seen).  `a` where the walk completed:
    # elsewhere the checker leaves what its gather had collected and the kernels answer zeros.
    ok = want["err"] == 1
    gd, wd = got["debug_d"], want["debug_d"]
    np.testing.assert_array_equal(gd == -1.0, wd == -1.0, err_msg=case + " d: known cells")
    np.testing.assert_array_equal(np.isnan(gd), np.isnan(wd), err_msg=case + " d: NaN cells")
    fin = np.isfinite(wd)
    scale = np.abs(np.where(fin & (wd >= 0), wd, 0.0)).max(axis=-1, keepdims=True)
    assert (np.abs(gd - wd)[fin] <= (1e-5 * np.abs(wd) + 1e-10 * scale)[fin]).all(), case + " d"
    ga, wa = got["debug_a"][ok], want["debug_a"][ok]
    np.testing.assert_array_equal(np.isnan(ga), np.isnan(wa), err_msg=case + " a: NaN cells")
    fin = np.isfinite(wa)
    assert (np.abs(ga - wa)[fin] <= (1e-5 * np.abs(wa) + 1e-10 * scale[ok])[fin]).all(), case + " a"
    # bit for bit what the parent commit answered
    rec = G.record(got)
    keys = sorted(k[len(case) + 1:] for k in parent.files if k.startswith(case + "/"))
    assert keys == sorted(rec), (case, keys, sorted(rec))
    for k in keys:
        a, b = rec[k], parent[case + "/" + k]
        assert a.dtype == b.dtype and a.shape == b.shape, (case, k)
        assert a.tobytes() == b.tobytes(), "%s: %s is not what the parent commit computed (%d of %d entries differ)" % (
            case, k, int((a.view(np.uint8).reshape(a.shape + (-1,)) != b.view(np.uint8).reshape(b.shape + (-1,))).any(-1).sum()) if a.ndim else 1, a.size)
