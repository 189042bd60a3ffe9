"""
Detector distortion correction on the GPU (libumpa_unwarp.so): the arithmetic bit for bit against the numpy restatement of
include/umpa_unwarp.h (tests/unwarp_expect.py), the fused path through stage_sample against the stand-alone call, the
attach rules, the farm, and device arrays on a side stream.

REACHES names, per test, the kernels of libumpa_unwarp.so it is there for (tests/test_unwarp_cpu.py checks on the CPU that
every unwarp_kernel symbol of the built library is claimed here, and that no claim is stale).
"""
import numpy as np
import pytest

import unwarp_expect as UE

pytestmark = pytest.mark.gpu

RAW_C = {np.uint16: "unsigned short", np.float32: "float", np.float64: "double"}
REACHES = {
    "tests/test_hip_unwarp.py::test_apply_equals_the_helper_bit_for_bit":
        ["unwarp_kernel<%s, %d>" % (c, k) for c in RAW_C.values() for k in (0, 1)],
}

DTYPES = [np.uint16, np.float32, np.float64]
INTERPS = ["linear", "cubic"]
CORR = ["plain", "dark", "dark_flat"]
MAPS = ["identity", "shift", "radial", "radial_x4", "last_row_col"]

Nw, MS = 2, 3                    # the matches of the fused tests
MH, MW, MK = 64, 72, 3


@pytest.fixture(scope="module")
def hip_ns():
    from umpa_amd import _lib, model
    if _lib.hip().device_count() < 1:
        pytest.fail("no HIP device: the GPU tests cannot run (there is no CPU fallback)")
    return model


@pytest.fixture(scope="module")
def device_maps(hip_ns):
    """(map name, interp) -> UnwarpMap at 37 x 71, built once"""
    from umpa_amd import UnwarpMap
    planes = UE.maps()
    return {(n, it): UnwarpMap(planes[n][0], planes[n][1], interp=it) for n in MAPS for it in INTERPS}


KEYS = ("f", "T", "dx", "dy", "df", "err")


def _maps_equal(got, want, what):
    for k in KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (what, k))


def _copy(res):
    return {k: np.array(v) for k, v in res.items() if isinstance(v, np.ndarray)}


# ----------------------------------------------------------------------------- 1. the arithmetic

@pytest.mark.parametrize("name", MAPS)
@pytest.mark.parametrize("corr", CORR)
@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["u16", "f32", "f64"])
def test_apply_equals_the_helper_bit_for_bit(device_maps, dtype, interp, corr, name):
    m = device_maps[(name, interp)]
    raw = UE.stack(dtype)
    dark, flat = UE.dark_flat()
    dark = dark if corr != "plain" else None
    flat = flat if corr == "dark_flat" else None
    got = m.apply(raw, dark=dark, flat=flat)
    want = UE.reference(raw, *UE.maps()[name], interp, dark, flat)
    assert got.dtype == np.float64 and got.shape == (UE.K, UE.H, UE.W) and np.isfinite(want).all()
    np.testing.assert_array_equal(got, want)
    if name == "radial_x4":
        assert not m.valid.all() and m.valid.any()


@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("name", ["shift", "radial"])
def test_a_nan_pixel_appears_exactly_where_the_helper_puts_it(device_maps, name, interp):
    raw = UE.stack(np.float32, nan_at=(1, 17, 33))
    dark, flat = UE.dark_flat()
    got = device_maps[(name, interp)].apply(raw, dark=dark, flat=flat)
    want = UE.reference(raw, *UE.maps()[name], interp, dark, flat)
    n = np.isnan(want)
    assert n[1].any() and not n[0].any()
    if name == "shift":                                               # the whole footprint, zero weights included
        assert n[1].sum() == (4 if interp == "linear" else 16)
    np.testing.assert_array_equal(np.isnan(got), n)
    np.testing.assert_array_equal(got[~n], want[~n])


# ----------------------------------------------------------------------------- shared inputs of the fused tests

_cache = {}


def series(h=MH, w=MW, k=MK, n_proj=4):
    """Two references, flats, a dark frame and n_proj uint16 projections (bench_c5's construction, small)."""
    key = (h, w, k, n_proj)
    if key not in _cache:
        from umpa_amd.synth import make_stack
        sam0, ref0, _ = make_stack(h, w, k, MS, df=True, seed=0, order=1)
        sam1, ref1, _ = make_stack(h, w, k, MS, df=True, seed=100, order=1)
        rng = np.random.default_rng(5)
        dark = 100.0 + rng.uniform(0, 2, size=(k, h, w))
        flats = 20000.0 * (1.0 + 0.05 * rng.standard_normal((2, k, h, w)))
        refs = np.stack([ref0, ref1])
        raws = []
        for p in range(n_proj):
            base = sam0 if p % 2 == 0 else sam1                       # the references alternate
            raws.append(np.ascontiguousarray(np.rint(base * (1.0 - 0.004 * p) * flats[p % 2] + dark).astype(np.uint16)))
        _cache[key] = (refs, flats, dark, raws)
    return _cache[key]


def _device_frames(a):
    import torch
    return list(torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0"))


def _staged_match(hip_ns, raw, dark, flat, ref, unwarp=None, detach=False):
    m = hip_ns.UMPAModelDF(np.zeros_like(ref), ref, window_size=Nw, max_shift=MS)
    if unwarp is not None:
        m.set_unwarp(unwarp)
    if detach:
        m.set_unwarp(None)
    m.stage_sample(list(raw), dark=_device_frames(dark), flat=_device_frames(flat))
    return _copy(m.match(quiet=True)), m


def _expected(hip_ns, umap, raw, dark, flat, ref):
    """a fresh model matched on the stand-alone unwarp of the projection"""
    sam = umap.apply(raw, dark=dark, flat=flat)
    return _copy(hip_ns.UMPAModelDF(sam, ref, window_size=Nw, max_shift=MS).match(quiet=True))


# ----------------------------------------------------------------------------- 2. identity equals today's path

@pytest.mark.parametrize("interp", INTERPS)
def test_identity_map_attached_equals_the_plain_stage_sample(hip_ns, interp):
    from umpa_amd import UnwarpMap
    refs, flats, dark, raws = series()
    want, _ = _staged_match(hip_ns, raws[0], dark, flats[0], refs[0])
    got, _ = _staged_match(hip_ns, raws[0], dark, flats[0], refs[0], unwarp=UnwarpMap.identity((MH, MW), interp=interp))
    assert want["err"].mean() > 0.5
    _maps_equal(got, want, "identity " + interp)


# ----------------------------------------------------------------------------- 3. fused equals stand-alone

def _run_streaming(hip_ns, umap, h, w, k, n_proj):
    from umpa_amd.farm import StreamingMatcher
    refs, flats, dark, raws = series(h, w, k, n_proj)
    sm = StreamingMatcher(refs, Nw, MS, df=True, device=0, flats=flats, dark=dark, ref_nums=[0, 1], unwarp=umap)
    got = [(pid, _copy(res)) for pid, res in sm.run((p % 2, raws[p]) for p in range(n_proj))]
    assert [pid for pid, _ in got] == [p % 2 for p in range(n_proj)]
    for p, (pid, res) in enumerate(got):
        want = _expected(hip_ns, umap, raws[p], dark, flats[p % 2], refs[p % 2])
        assert want["err"].mean() > 0.5
        _maps_equal(res, want, "projection %d" % p)
    return got


@pytest.mark.parametrize("interp", INTERPS)
def test_streaming_matcher_with_a_map_equals_apply_then_match(hip_ns, interp):
    from umpa_amd import UnwarpMap
    d0, d1 = UE.radial_map(MH, MW)
    got = _run_streaming(hip_ns, UnwarpMap(d0, d1, interp=interp), MH, MW, MK, 4)
    # the map did something: projection 0 differs from the match of the raw geometry
    refs, flats, dark, raws = series()
    plain, _ = _staged_match(hip_ns, raws[0], dark, flats[0], refs[0])
    assert not np.array_equal(plain["dx"], got[0][1]["dx"])


def test_streaming_matcher_with_a_map_at_512(hip_ns):
    from umpa_amd import UnwarpMap
    d0, d1 = UE.radial_map(512, 512)
    _run_streaming(hip_ns, UnwarpMap(d0, d1, interp="cubic"), 512, 512, 5, 2)


# ----------------------------------------------------------------------------- 4. attach rules

def test_attach_is_refused_for_borrowed_frames_and_other_shapes(hip_ns):
    import torch
    from umpa_amd import UnwarpMap
    refs, flats, dark, raws = series()
    umap = UnwarpMap.identity((MH, MW))
    t = torch.from_numpy(refs[0]).to("cuda:0")
    borrowed = hip_ns.UMPAModelDF(list(t), list(t.clone()), window_size=Nw, max_shift=MS)
    with pytest.raises(RuntimeError, match="borrows"):
        borrowed.set_unwarp(umap)
    own = hip_ns.UMPAModelDF(np.zeros_like(refs[0]), refs[0], window_size=Nw, max_shift=MS)
    with pytest.raises(RuntimeError, match="%d x %d" % (MH, MW + 1)):
        own.set_unwarp(UnwarpMap.identity((MH, MW + 1)))
    # a refused attach leaves the model as it was: it stages and matches as a model without a map
    own.stage_sample(list(raws[0]), dark=_device_frames(dark), flat=_device_frames(flats[0]))
    want, _ = _staged_match(hip_ns, raws[0], dark, flats[0], refs[0])
    _maps_equal(_copy(own.match(quiet=True)), want, "after a refused attach")


def test_detach_restores_the_plain_stage_sample(hip_ns):
    from umpa_amd import UnwarpMap
    refs, flats, dark, raws = series()
    d0, d1 = UE.radial_map(MH, MW)
    want, _ = _staged_match(hip_ns, raws[0], dark, flats[0], refs[0])
    got, _ = _staged_match(hip_ns, raws[0], dark, flats[0], refs[0], unwarp=UnwarpMap(d0, d1), detach=True)
    _maps_equal(got, want, "attach, then attach(None)")


def test_map_and_model_may_be_destroyed_in_either_order(hip_ns):
    """The rule (include/umpa_unwarp.h): destroying the handle gives up the caller's reference; a model the map is attached
    to keeps unwarping until it detaches or is destroyed."""
    from umpa_amd import UnwarpMap
    refs, flats, dark, raws = series()
    d0, d1 = UE.radial_map(MH, MW)
    umap = UnwarpMap(d0, d1)
    want_unwarped = _expected(hip_ns, umap, raws[1], dark, flats[1], refs[1])
    want_plain, _ = _staged_match(hip_ns, raws[1], dark, flats[1], refs[1])
    m = hip_ns.UMPAModelDF(np.zeros_like(refs[1]), refs[1], window_size=Nw, max_shift=MS)
    m.set_unwarp(umap)
    umap.destroy()                                                    # the map first ...
    with pytest.raises(RuntimeError, match="destroyed"):
        umap.apply(raws[1])
    dk, fl = _device_frames(dark), _device_frames(flats[1])
    m.stage_sample(list(raws[1]), dark=dk, flat=fl)                   # ... the model still unwarps
    _maps_equal(_copy(m.match(quiet=True)), want_unwarped, "map destroyed while attached")
    m.set_unwarp(None)                                                # ... and stages without one afterwards
    m.stage_sample(list(raws[1]), dark=dk, flat=fl)
    _maps_equal(_copy(m.match(quiet=True)), want_plain, "map destroyed, then detached")
    # the model first: the map stays usable
    umap2 = UnwarpMap(d0, d1)
    m2 = hip_ns.UMPAModelDF(np.zeros_like(refs[1]), refs[1], window_size=Nw, max_shift=MS)
    m2.set_unwarp(umap2)
    m2.__del__()
    raw = UE.stack(np.uint16, MH, MW, 1)
    np.testing.assert_array_equal(umap2.apply(raw), UE.reference(raw, d0, d1, "cubic"))


# ----------------------------------------------------------------------------- 5. the farm

def test_projection_farm_with_a_map_on_one_gpu(hip_ns):
    from umpa_amd import UnwarpMap
    from umpa_amd.farm import ProjectionFarm
    refs, flats, dark, raws = series()
    d0, d1 = UE.radial_map(MH, MW)
    umap = UnwarpMap(d0, d1, interp="cubic")
    with ProjectionFarm(refs, Nw, MS, df=True, devices=[0], flats=flats, dark=dark, ref_nums=[0, 1],
                        raw_dtype=np.uint16, unwarp=umap) as farm:
        got = dict(farm.map(((p, raws[p]) for p in range(3)), timeout=300.0))     # projection p: nearest reference min(p, 1)
    assert sorted(got) == [0, 1, 2]
    for p in range(3):
        r = min(p, 1)
        want = _expected(hip_ns, umap, raws[p], dark, flats[r], refs[r])
        _maps_equal(got[p], want, "farm projection %d" % p)


# ----------------------------------------------------------------------------- 6. device arrays on a side stream

@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=["u16", "f32"])
def test_device_arrays_on_a_side_stream_equal_the_host_call(device_maps, dtype):
    import torch
    umap = device_maps[("radial", "cubic")]
    raw = UE.stack(dtype)
    dark, flat = UE.dark_flat()
    want = umap.apply(raw, dark=dark, flat=flat)
    d_raw, d_dark, d_flat = _device_frames(raw), _device_frames(dark), _device_frames(flat)
    out = [torch.zeros((UE.H, UE.W), dtype=torch.float64, device="cuda:0") for _ in range(UE.K)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=0)
    umap.apply_device(d_raw, out, dark=d_dark, flat=d_flat, stream=s.cuda_stream)
    s.synchronize()
    np.testing.assert_array_equal(np.stack([o.cpu().numpy() for o in out]), want)
