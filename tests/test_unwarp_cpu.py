"""
Detector distortion correction, what can be checked without a GPU: the third library's build and symbol sets, the hook in
the main library, the host logic of umpa_amd.unwarp, the expectation the GPU tests use (tests/unwarp_expect.py) on three
pinned points, and the farm's hand-over of the map to its workers.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import REPO

import unwarp_expect as UE
from nativelibs import assert_claimed, build_all as _build, declared as _declared, exported, kernel_keys

UNWARP_LIB = os.path.join(REPO, "umpa_amd", "libumpa_unwarp.so")
FAMILY = "unwarp_kernel"


# ----------------------------------------------------------------------------- 1. the library builds

def test_build_produces_the_unwarp_library_with_the_declared_symbols():
    g = _build()
    assert g.UNWARP_LIB == UNWARP_LIB and os.path.exists(UNWARP_LIB)
    from umpa_amd import _lib
    declared = _declared("umpa_unwarp.h", "umpa_unwarp_")
    assert declared == sorted("umpa_unwarp_" + s for s in _lib.UNWARP_SYMBOLS) and len(declared) == 5
    own = sorted(n for n in exported(UNWARP_LIB) if n.startswith("umpa"))
    assert own == declared, own                                       # its C ABI and nothing else of its own
    _lib.hip()
    lib = ctypes.CDLL(UNWARP_LIB)
    for name in declared:
        assert hasattr(lib, name), name
    assert _lib.unwarp().path == UNWARP_LIB


def test_main_library_exports_the_stage_filter_setter_and_no_new_public_symbol():
    g = _build()
    from umpa_amd import _lib
    names = exported(g.HIP_LIB)
    assert "umpa_hipx_set_stage_filter" in names
    public = sorted(n for n in names if n.startswith("umpa_hip_"))
    assert public == sorted("umpa_hip_" + s for s in _lib.HIP_SYMBOLS), set(public) ^ set("umpa_hip_" + s for s in _lib.HIP_SYMBOLS)
    hdr = open(os.path.join(REPO, "include", "umpa_hip.h")).read()
    assert "umpa_hipx" not in hdr and "stage_filter" not in hdr


def test_every_unwarp_kernel_is_claimed_by_a_gpu_test():
    _build()
    syms = [k for k in kernel_keys(UNWARP_LIB) if k.split("<", 1)[0] == FAMILY]
    assert len(syms) == 6, syms                                       # three raw dtypes x two interpolation kinds
    assert_claimed(syms, "unwarp")


# ----------------------------------------------------------------------------- 2. host logic

def test_from_coordinates_equals_hand_built_displacements():
    from umpa_amd.unwarp import UnwarpMap
    h, w = 5, 7
    rng = np.random.default_rng(3)
    want0 = rng.uniform(-3, 3, size=(h, w)).astype(np.float32)
    want1 = rng.uniform(-3, 3, size=(h, w)).astype(np.float32)
    src0 = np.empty((h, w)); src1 = np.empty((h, w))
    for i in range(h):
        for j in range(w):
            src0[i, j] = i + float(want0[i, j])                       # exact: small integers plus a float32
            src1[i, j] = j + float(want1[i, j])
    d0, d1 = UnwarpMap.displacements(src0, src1)
    assert d0.dtype == np.float32 and d1.dtype == np.float32
    np.testing.assert_array_equal(d0, (src0 - np.arange(h)[:, None]).astype(np.float32))
    np.testing.assert_array_equal(d1, (src1 - np.arange(w)[None, :]).astype(np.float32))
    # i + d is not always representable, so the round trip may move a displacement by an ulp of i + d, no more
    assert np.abs(d0 - want0).max() <= 2.0 ** -50 * h and np.abs(d1 - want1).max() <= 2.0 ** -50 * w


@pytest.mark.parametrize("interp", ["linear", "cubic"])
def test_valid_equals_a_brute_force_footprint_check(interp):
    from umpa_amd.unwarp import footprint_valid
    d0, d1 = UE.maps()["radial_x4"]
    want = UE.footprint_valid_bruteforce(d0, d1, interp)
    got = footprint_valid(d0, d1, interp)
    assert got.dtype == bool
    np.testing.assert_array_equal(got, want)
    # the map leaves the frame on all four sides, and not everywhere
    assert (~want[0]).any() and (~want[-1]).any() and (~want[:, 0]).any() and (~want[:, -1]).any() and want.any()
    # ... by the sign of the displacement too: the clamp is met at both ends of both axes
    ii, jj = np.arange(UE.H, dtype=np.float64)[:, None], np.arange(UE.W, dtype=np.float64)[None, :]
    assert (ii + d0 < 0).any() and (ii + d0 > UE.H - 1).any() and (jj + d1 < 0).any() and (jj + d1 > UE.W - 1).any()


def test_unwarp_map_property_valid_uses_that_function():
    """UnwarpMap.valid is footprint_valid of the stored planes (checked on the class without building a device map)."""
    from umpa_amd import unwarp
    d0, d1 = UE.maps()["radial"]
    m = unwarp.UnwarpMap.__new__(unwarp.UnwarpMap)
    m._d0, m._d1, m._interp, m._valid, m._handle = d0, d1, "cubic", None, None
    np.testing.assert_array_equal(m.valid, UE.footprint_valid_bruteforce(d0, d1, "cubic"))
    assert m.shape == (UE.H, UE.W) and m.interp == "cubic"


# ----------------------------------------------------------------------------- 3. the helper, on three pinned points

@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("dtype", [np.uint16, np.float32, np.float64])
def test_helper_identity_is_flat_correction_bit_for_bit(interp, dtype):
    raw = UE.stack(dtype)
    dark, flat = UE.dark_flat()
    z = np.zeros((UE.H, UE.W), np.float32)
    got = UE.reference(raw, z, z, interp, dark, flat)
    np.testing.assert_array_equal(got, (raw.astype(np.float64) - dark) / flat)
    np.testing.assert_array_equal(UE.reference(raw, z, z, interp), raw.astype(np.float64))


@pytest.mark.parametrize("interp", ["linear", "cubic"])
def test_helper_integer_shift_returns_shifted_copies(interp):
    raw = UE.stack(np.uint16)
    d0, d1 = UE.maps()["shift"]                                       # (+2, -3)
    got = UE.reference(raw, d0, d1, interp)
    ii = np.clip(np.arange(UE.H) + 2, 0, UE.H - 1)
    jj = np.clip(np.arange(UE.W) - 3, 0, UE.W - 1)
    np.testing.assert_array_equal(got, raw.astype(np.float64)[:, ii[:, None], jj[None, :]])


@pytest.mark.parametrize("interp", ["linear", "cubic"])
def test_helper_half_pixel_shift_reproduces_a_linear_ramp(interp):
    """Catmull-Rom reproduces linear data, bilinear does by construction; with integer-valued data and t = 1/2 every
    product and sum is exact, so the ramp comes back exactly -- where no tap was clamped."""
    from umpa_amd.unwarp import footprint_valid
    ii, jj = np.meshgrid(np.arange(UE.H, dtype=np.float64), np.arange(UE.W, dtype=np.float64), indexing="ij")
    ramp = 3.0 * ii + 5.0 * jj + 7.0
    half = np.full((UE.H, UE.W), 0.5, np.float32)
    got = UE.reference(ramp, half, half, interp)
    want = 3.0 * (ii + 0.5) + 5.0 * (jj + 0.5) + 7.0
    ok = footprint_valid(half, half, interp)
    assert ok.sum() >= (UE.H - 3) * (UE.W - 3)
    np.testing.assert_array_equal(got[ok], want[ok])


def test_helper_spreads_a_nan_over_its_footprint():
    raw = UE.stack(np.float32, nan_at=(0, 10, 20))
    z = np.zeros((UE.H, UE.W), np.float32)
    lin = np.isnan(UE.reference(raw, z, z, "linear")[0])
    cub = np.isnan(UE.reference(raw, z, z, "cubic")[0])
    assert sorted(map(tuple, np.argwhere(lin))) == [(i, j) for i in (9, 10) for j in (19, 20)]
    assert sorted(map(tuple, np.argwhere(cub))) == [(i, j) for i in (8, 9, 10, 11) for j in (18, 19, 20, 21)]


# ----------------------------------------------------------------------------- 4. no CPU fallback

def test_unwarp_map_without_gpu_raises_the_librarys_error():
    _build()
    from umpa_amd import UnwarpMap, _lib
    if _lib.hip().device_count() > 0:                                 # a GPU is present: the same call must then succeed
        assert UnwarpMap.identity((8, 8)).shape == (8, 8)
        return
    with pytest.raises(RuntimeError, match="no HIP device"):
        UnwarpMap.identity((8, 8))


# ----------------------------------------------------------------------------- 5. the farm hands the map to its workers

def echo_worker(device, cfg, tasks, results, in_name, out_name):
    """A stand-in worker (umpa_amd.farm.ProjectionFarm(worker=...)): writes what it found in cfg["unwarp"] into the result
    slot of every projection instead of matching."""
    from umpa_amd.farm import _Slots
    slots_out = _Slots(None, cfg["depth_out"], cfg["out_bytes"], name=out_name)
    K, H, W = np.asarray(cfg["refs"]).shape[-3:]
    P = cfg["window_size"] + cfg["max_shift"]
    N0, N1 = H - 2 * P, W - 2 * P
    while True:
        item = tasks.get()
        if item is None:
            return
        seq, pid, q_in, q_out, kw = item
        vals, off = slots_out.view(q_out, (5 if cfg["df"] else 4, N0, N1), np.float64, 0)
        err, off = slots_out.view(q_out, (N0, N1), np.int32, off)
        vals[...] = 0.0
        uw = cfg.get("unwarp")
        err[...] = -1 if uw is None else len(uw)
        if uw is not None:
            d0, d1, interp = uw
            vals[0] = d0[P:H - P, P:W - P]
            vals[1] = d1[P:H - P, P:W - P]
            vals[2] = {"linear": 0.0, "cubic": 1.0}[interp]
            vals[3] = float(d0.dtype == np.float32 and d1.dtype == np.float32 and d0.shape == (H, W) and d1.shape == (H, W))
        results.put(("done", seq, q_in, q_out, None))


@pytest.mark.parametrize("interp", ["linear", "cubic"])
def test_farm_carries_the_map_in_the_worker_configuration(interp):
    from umpa_amd.farm import ProjectionFarm
    h, w, k, Nw, ms = 24, 30, 2, 2, 3
    d0, d1 = UE.radial_map(h, w)
    refs = np.ones((k, h, w))
    with ProjectionFarm(refs, Nw, ms, df=True, devices=[None], worker=echo_worker, unwarp=(d0, d1, interp)) as farm:
        out = dict(farm.map([(5, np.ones((k, h, w)))], timeout=120.0))
    res = out[5]
    P = Nw + ms
    assert np.all(res["err"] == 3)
    np.testing.assert_array_equal(res["f"], d0[P:h - P, P:w - P].astype(np.float64))
    np.testing.assert_array_equal(res["T"], d1[P:h - P, P:w - P].astype(np.float64))
    assert np.all(res["dx"] == (1.0 if interp == "cubic" else 0.0)) and np.all(res["dy"] == 1.0)
    with ProjectionFarm(refs, Nw, ms, df=True, devices=[None], worker=echo_worker) as farm:
        out = dict(farm.map([(5, np.ones((k, h, w)))], timeout=120.0))
    assert np.all(out[5]["err"] == -1)                                # without the option the configuration says so
    with pytest.raises(ValueError):
        ProjectionFarm(refs, Nw, ms, devices=[None], worker=echo_worker, unwarp=(d0[1:], d1[1:], interp))
