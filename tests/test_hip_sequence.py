"""
model.sequence() / umpa_grid_sequence on the GPU (libumpa_grid.so).  In every case each output EQUALS the restatement of
tests/sequence_expect.py applied to the device's own cost_volume(with_fit=True) of the same model and region and to the
state that was handed in -- the next state, shift, cost, total, cost0, moved, err, T, df, and dx, dy, f bit for bit (the 4x4
fit of the sub-pixel modes -1 and 1 is the device's own entry point for one array), pixels without a finite sum included.

REACHES names, per test, the kernels of libumpa_grid.so it is there for (tests/test_sequence_cpu.py checks on the CPU that
every grid_sequence_kernel symbol of the built library is claimed here, and that no claim is stale).
"""
import ctypes
import functools

import numpy as np
import pytest

import basins_expect as BE
import sequence_expect as SE

pytestmark = pytest.mark.gpu

KTEMPL = 24                      # UMPA_KTEMPL: frame counts with their own instantiation (dark-field model)
REACHES = {
    "tests/test_hip_sequence.py::test_every_frame_count": ["grid_sequence_kernel<1, %d>" % (n if n <= KTEMPL else 0) for n in range(1, KTEMPL + 2)],
    "tests/test_hip_sequence.py::test_smallest_shapes": ["grid_sequence_kernel<0, 0>"],
}
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def hip_ns():
    from umpa_amd import _lib, model
    if _lib.hip().device_count() < 1:
        pytest.fail("no HIP device: the GPU tests cannot run (there is no CPU fallback)")
    return model


def _model(hip_ns, kind, sam, ref, Nw, ms, assign="sam", subpx=0, **kw):
    m = (hip_ns.UMPAModelDF if kind else hip_ns.UMPAModelNoDF)(sam, ref, window_size=Nw, max_shift=ms, **kw)
    m.assign_coordinates = assign
    m.sub_pixel_mode = subpx
    return m


def _launches(m, fn):
    """fn() with the library's timers on: (result, {kernel family: launches})"""
    lib, h = m._lib, m._handle
    lib.timing_enable(h, 1)
    try:
        out = fn()
    finally:
        lib.timing_enable(h, 0)
    seen = {}
    for q in range(lib.timing_collect(h)):
        nm, tot, cnt = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_int()
        lib.timing_read(h, q, ctypes.byref(nm), ctypes.byref(tot), ctypes.byref(cnt))
        seen[nm.value.decode()] = cnt.value
    return out, seen


def _scale(vol):
    """the scale of a volume's costs (from the volume alone): the median gap between the two lowest costs of a pixel"""
    U = vol["cost"].shape[0]
    with np.errstate(invalid="ignore"):
        c = np.sort(np.where(vol["cost"] < np.inf, vol["cost"], np.inf).reshape(U * U, -1), axis=0)
        gap = (c[1] - c[0])[np.isfinite(c[1])]
    return float(np.median(gap)) if gap.size else 1.0


def _state(vol, seed, special=False):
    """a previous state on the scale of the volume: the volume's own costs, permuted among the pixels' shifts by a roll that
    differs per call, plus noise -- a state whose minimum lies elsewhere than the data term's; with `special`, NaN and +Inf
    entries, an all-NaN pixel, an all-Inf pixel and a -Inf entry"""
    rng = np.random.default_rng(seed)
    c = np.where(np.isfinite(vol["cost"]), vol["cost"], 0.0)
    U = c.shape[0]
    prev = np.roll(c, (1 + seed % (U - 1), 1 + (seed // 3) % (U - 1)), axis=(0, 1)) + _scale(vol) * rng.random(c.shape)
    if special:
        w = rng.random(prev.shape)
        prev[w < 0.05] = NAN
        prev[(w >= 0.05) & (w < 0.08)] = INF
        prev[:, :, 0, 0] = NAN
        prev[:, :, 1, 2] = INF
        prev[0, 1, 2, 1] = -INF
    return np.ascontiguousarray(prev)


def _check(m, cases, what="", vol=None, **region):
    """sequence() of the region for every (state, lam, trunc) of `cases` against the restatement on the device's own volume:
    ([results], volume)"""
    vol = vol or m.cost_volume(with_fit=True, **region)
    sub = m.sub_pixel_mode
    fit = BE.device_fit(sub, m._device) if sub else None
    res = []
    for q, (state, lam, trunc) in enumerate(cases):
        t = m.sequence(state=state, lam=lam, trunc=trunc, **region)
        want = SE.restate(vol["cost"], vol["T"], vol.get("df"), state, lam, trunc, sub, fit=fit)
        SE.assert_equal(t, want, "%s case %d (lam %r trunc %r)" % (what, q, lam, trunc))
        res.append(t)
    return res, vol


def _grid_equal(t, grid, kind, what):
    for n in ("dx", "dy", "f", "T", "err") + (("df",) if kind else ()):
        np.testing.assert_array_equal(t[n], grid[n], err_msg="%s against search='grid': %s" % (what, n))
    np.testing.assert_array_equal(t["cost"], t["cost0"])
    np.testing.assert_array_equal(t["total"], t["cost"])
    assert (np.asarray(t["moved"]) == 0).all()


# ----------------------------------------------------------------------------- 1. every instantiation

@pytest.mark.parametrize("K", list(range(1, KTEMPL + 2)))
def test_every_frame_count(hip_ns, K):
    from umpa_amd.synth import make_stack
    Nw, ms = 1, 2
    sam, ref, _ = make_stack(20, 44, K, ms, df=True, seed=100 + K)    # 14 x 38 pixels: three blocks, the last one ragged
    m = _model(hip_ns, 1, sam, ref, Nw, ms, "sam" if K % 2 else "ref")
    vol = m.cost_volume(with_fit=True)
    s = _scale(vol)
    (res, _), seen = _launches(m, lambda: _check(m, [(None, 0.1 * s, None), (_state(vol, K), 0.3 * s, 2.0 * s)], "K %d" % K, vol=vol))
    assert seen.get("table_consumer") == 2 and "replay_walk" not in seen, seen
    assert (res[1]["moved"] == 1).any()


# ----------------------------------------------------------------------------- 2. the smallest shapes where it can go wrong

@pytest.mark.parametrize("Nw,ms", [(1, 2), (2, 3), (2, 4)], ids=["ms2", "ms3", "ms4"])
@pytest.mark.parametrize("kind", [0, 1], ids=["NoDF", "DF"])
def test_smallest_shapes(hip_ns, kind, Nw, ms):
    from umpa_amd.synth import make_stack
    sam, ref, _ = make_stack(40, 48, 3, ms, df=True, seed=200 + ms)
    for assign in ("sam", "ref"):
        for subpx in (-1, 0, 1):
            m = _model(hip_ns, kind, sam, ref, Nw, ms, assign, subpx)
            vol = m.cost_volume(with_fit=True)
            s = _scale(vol)
            prev = _state(vol, 7 + ms)
            cases = [(prev, 0.25 * s, None), (prev, 0.25 * s, 1.5 * s), (_state(vol, 11, special=True), 0.1 * s, 3.0 * s)]
            res, _ = _check(m, cases, "%s subpx %d" % (assign, subpx), vol=vol)
            grid = m.match(quiet=True, search="grid")
            m.ROI = None
            # lam = 0 and no state: the grid search, bit for bit; trunc = 0: M = 0 wherever the state's minimum is finite
            for what, args in (("lam 0", dict(state=prev, lam=0.0, trunc=0.7 * s)), ("no state", dict(state=None, lam=0.25 * s))):
                t = m.sequence(**args)
                _grid_equal(t, grid, kind, what)
                np.testing.assert_array_equal(t["state"], vol["cost"] + 0.0)
            t = m.sequence(state=prev, lam=0.25 * s, trunc=0.0)
            np.testing.assert_array_equal(t["state"], vol["cost"] + 0.0)
            _grid_equal(t, grid, kind, "trunc 0")
            assert (res[0]["moved"] == 1).any() and (res[0]["moved"] == 0).any()
            if ms > 2:
                assert (res[0]["err"] == 1).any() and (res[0]["err"] == 0).any()
            else:
                assert (res[0]["err"] == 0).all()                     # a box of 3 x 3 shifts holds no 4 x 4 neighbourhood


def test_the_largest_state_per_pixel(hip_ns):
    """ms = 8: U = 15, 1800 bytes of state per pixel, a wave takes 32 pixels"""
    from umpa_amd.synth import make_stack
    sam, ref, _ = make_stack(52, 52, 3, 8, df=True, seed=308)
    for kind in (0, 1):
        m = _model(hip_ns, kind, sam, ref, 1, 8, "sam" if kind else "ref", -1)
        vol = m.cost_volume(with_fit=True)
        s = _scale(vol)
        res, _ = _check(m, [(_state(vol, 5), 0.05 * s, None), (_state(vol, 6, special=True), 0.05 * s, 4.0 * s)], "ms 8 kind %d" % kind, vol=vol)
        assert (res[0]["moved"] == 1).any() and (res[0]["err"] == 1).any()


def test_through_the_marching_table(hip_ns):
    from umpa_amd.synth import make_stack
    Nw, ms = 6, 2
    sam, ref, _ = make_stack(70, 83, 3, ms, df=True, seed=5, order=1)
    for kind, assign in ((1, "sam"), (0, "ref")):
        m = _model(hip_ns, kind, sam, ref, Nw, ms, assign)
        vol = m.cost_volume(with_fit=True)
        s = _scale(vol)
        _, seen = _launches(m, lambda: _check(m, [(_state(vol, 3), 0.2 * s, None), (_state(vol, 4, special=True), 0.2 * s, s)], "march kind %d" % kind, vol=vol))
        assert seen.get("corr_march", 0) >= 1 and seen.get("table_consumer") == 2 and "corr_volume" not in seen and "replay_walk" not in seen, seen


# ----------------------------------------------------------------------------- 3. chunks, chains, regions

def test_four_row_chunks_change_nothing(hip_ns, monkeypatch):
    from nativelibs import gpu_test_module
    sam, ref = gpu_test_module("widen")._chunk_stack()
    rng = np.random.default_rng(13)
    s = _scale(_model(hip_ns, 1, sam, ref, 3, 5).cost_volume(ROI=((40, 60, 1), (100, 200, 1))))
    prev = 5.0 * s * rng.random((9, 9, 128, 512))
    res = {}
    for mb in (None, "16"):
        if mb:
            monkeypatch.setenv("UMPA_HIP_TABLE_MB", mb)
        else:
            monkeypatch.delenv("UMPA_HIP_TABLE_MB", raising=False)
        m = _model(hip_ns, 1, sam, ref, 3, 5, subpx=-1)
        res[mb], seen = _launches(m, lambda: [m.sequence(state=None, lam=0.2 * s), m.sequence(state=prev, lam=0.2 * s, trunc=3.0 * s)])
        assert seen.get("table_consumer") == (8 if mb else 2), (mb, seen)
    for a, b in zip(res["16"], res[None]):
        SE.assert_equal(a, {n: np.asarray(v) for n, v in b.items()}, "four chunks")
    assert (res[None][1]["moved"] == 1).any()


@functools.lru_cache(maxsize=None)
def _hp_stack():
    import grid_expect as GE
    return GE.stack("64x72x3")


def test_a_three_step_chain(hip_ns):
    """step t's state is fed to step t + 1, on three different sample stacks; equality with the restatement at every step"""
    sam, ref, c = _hp_stack()
    rng = np.random.default_rng(31)
    for kind in (0, 1):
        m = _model(hip_ns, kind, sam, ref, c["Nw"], c["ms"], subpx=1)
        state, s = None, None
        for t in range(3):
            m.update_frames(sam_list=np.ascontiguousarray(sam * (1.0 + 0.02 * rng.standard_normal(sam.shape))))
            vol = m.cost_volume(with_fit=True)
            s = s or _scale(vol)
            (r,), _ = _check(m, [(state, 0.2 * s, 3.0 * s)], "chain kind %d step %d" % (kind, t), vol=vol)
            state = r["state"]
        assert (r["moved"] == 1).any() and (r["total"] >= r["cost"]).all()


def test_roi_steps_and_ragged_blocks(hip_ns):
    sam, ref, c = _hp_stack()
    for kind in (0, 1):
        m = _model(hip_ns, kind, sam, ref, c["Nw"], c["ms"], subpx=-1)
        roi_before = m.ROI
        for region in (dict(step=2), dict(step=3), dict(ROI=((3, 40, 2), (5, 44, 3))), dict(ROI=((1, 6, 1), (2, 19, 1))), dict(ROI=((0, 37, 1), (0, 33, 1)))):
            vol = m.cost_volume(with_fit=True, **region)
            s = _scale(vol)
            _check(m, [(_state(vol, 9), 0.2 * s, None), (_state(vol, 10, special=True), 0.2 * s, 2.0 * s)], "kind %d %r" % (kind, region), vol=vol, **region)
        assert m.ROI == roi_before                                    # the model's own ROI is left alone


# ----------------------------------------------------------------------------- 4. special pixels

@pytest.mark.parametrize("bad", ["nan", "+inf"])
def test_special_pixels_in_the_sample(hip_ns, bad):
    """a NaN and an Inf pixel in the sample stack, placed as tests/regimes.py places them: pixels without any cost (err = 0,
    zeros, a NaN state) and pixels with NaN cells in the box must be the restatement's on the dirty volume, with a clean and
    with a special state"""
    import regimes
    from umpa_amd.synth import make_stack
    cfg = dict(Nw=2, K=3, ms=3, H=60, W=70)
    sam, ref, _ = make_stack(cfg["H"], cfg["W"], cfg["K"], cfg["ms"], df=True, seed=77)
    pos = regimes.bad_positions(cfg)
    for kind, assign in ((1, "sam"), (0, "ref")):
        s_, r_ = regimes.bad_pixels(sam, ref, bad, "sam", pos)
        m = _model(hip_ns, kind, s_, r_, cfg["Nw"], cfg["ms"], assign, -1)
        vol = m.cost_volume(with_fit=True)
        s = _scale(vol)
        (a, b), _ = _check(m, [(_state(vol, 2), 0.2 * s, None), (_state(vol, 3, special=True), 0.2 * s, 2.0 * s)], "%s kind %d" % (bad, kind), vol=vol)
        with np.errstate(invalid="ignore"):
            none = ~(vol["cost"] < np.inf).any(axis=(0, 1))
        assert none.any() and not none.all()
        assert (a["err"][none] == 0).all() and (a["total"][none] == 0).all() and (a["moved"][none] == 0).all() and np.isnan(a["state"][:, :, none]).all()


# ----------------------------------------------------------------------------- 5. repeats, I/O sides, Sequence

def test_repeats_device_arrays_and_a_side_stream(hip_ns):
    import torch
    from umpa_amd import _lib
    sam, ref, c = _hp_stack()
    for kind in (0, 1):
        m = _model(hip_ns, kind, sam, ref, c["Nw"], c["ms"], subpx=-1)
        vol = m.cost_volume(with_fit=True)
        s = _scale(vol)
        prev = _state(vol, 21, special=True)
        host = {n: np.asarray(v) for n, v in m.sequence(state=prev, lam=0.2 * s, trunc=2.0 * s).items()}
        SE.assert_equal(m.sequence(state=prev, lam=0.2 * s, trunc=2.0 * s), host, "second call")
        out = np.empty_like(prev)
        r = m.sequence(state=prev, lam=0.2 * s, trunc=2.0 * s, out=out)
        assert r["state"] is out
        SE.assert_equal(r, host, "into a given array")
        dev = torch.device("cuda", m._device)
        stream = torch.cuda.Stream(device=dev)
        tprev, tout = torch.from_numpy(prev).to(dev), torch.empty(prev.shape, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(stream):
            d1 = m.sequence(state=tprev, lam=0.2 * s, trunc=2.0 * s)
            d2 = m.sequence(state=tprev, lam=0.2 * s, trunc=2.0 * s, out=tout)
            d3 = m.sequence(state=None, lam=0.2 * s, out=tout.clone())
        stream.synchronize()
        assert all(isinstance(v, torch.Tensor) and v.is_cuda for d in (d1, d2, d3) for v in d.values()) and d2["state"] is tout
        SE.assert_equal(d1, host, "device arrays")
        SE.assert_equal(d2, host, "device arrays, given out")
        SE.assert_equal(d3, {n: np.asarray(v) for n, v in m.sequence(state=None, lam=0.2 * s).items()}, "device arrays, no state")
        with pytest.raises(ValueError, match="both numpy arrays or both HIP tensors"):
            m.sequence(state=tprev, lam=0.1, out=out)
        # the C ABI: df with the plain model is refused by name, and the model works afterwards
        if kind == 0:
            g = _lib.grid()
            N0, N1 = m.extent
            d = [np.zeros((N0, N1)) for _ in range(6)] + [np.zeros((N0, N1), np.int32) for _ in range(3)] + [np.zeros((N0, N1)), np.zeros((N0, N1)), np.zeros((N0, N1), np.int32)]
            ptrs = [a.ctypes.data for a in d]
            rc = g.sequence(m._handle, 0, 1, N0, 0, 1, N1, None, 0.0, INF, None, *ptrs, 0, None)
            assert rc < 0 and g.error() == "grid: sequence: a dark-field map (df) needs the dark-field model", (rc, g.error())
            SE.assert_equal(m.sequence(state=prev, lam=0.2 * s, trunc=2.0 * s), host, "after a refusal")


def test_sequence_steps_over_four_staged_projections(hip_ns):
    """uint16 raw frames with dark and flat on the device: Sequence.step against four explicit model.sequence calls on a
    second model that stages the same stacks"""
    import torch
    from umpa_amd import Sequence
    sam, ref, c = _hp_stack()
    rng = np.random.default_rng(17)
    K, H, W = sam.shape
    dark = 90.0 + 4.0 * rng.random((K, H, W))
    flat = 0.8 + 0.4 * rng.random((K, H, W))
    gain = 3000.0 / sam.max()
    m = _model(hip_ns, 1, sam, ref, c["Nw"], c["ms"], subpx=-1)
    m2 = _model(hip_ns, 1, sam, ref, c["Nw"], c["ms"], subpx=-1)
    dev = torch.device("cuda", m._device)
    tdark, tflat = [torch.from_numpy(x).to(dev) for x in dark], [torch.from_numpy(x).to(dev) for x in flat]
    lam = 0.2 * _scale(m2.cost_volume())
    q = Sequence(m, lam, trunc=10.0 * lam)
    state, buffers = None, set()
    for t in range(4):
        true = sam * (1.0 + 0.03 * rng.standard_normal(sam.shape))
        raw = np.clip(np.rint(true * gain * flat + dark), 0, 65535).astype(np.uint16)
        r = q.step(list(raw), dark=tdark, flat=tflat)
        assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in r.values()) and q.state is r["state"]
        buffers.add(r["state"].data_ptr())
        m2.stage_sample(list(raw), dark=tdark, flat=tflat)
        want = m2.sequence(state=state, lam=lam, trunc=10.0 * lam)
        SE.assert_equal(r, {n: np.asarray(v) for n, v in want.items()}, "step %d" % t)
        state = want["state"]
    assert len(buffers) == 2                                          # two tensors take turns
    q.reset()
    r = q.step(list(raw), dark=tdark, flat=tflat)
    SE.assert_equal(r, {n: np.asarray(v) for n, v in m2.sequence(state=None, lam=lam, trunc=10.0 * lam).items()}, "after reset")


def test_python_refusals_on_real_models_and_the_walk_afterwards(hip_ns):
    sam, ref, c = _hp_stack()
    kw = dict(window_size=c["Nw"], max_shift=c["ms"])
    mask = np.ones_like(sam)
    mask[:, 20:24, 30:40] = 0.0
    tail = r" \(grid search / cost volume\): "
    with pytest.raises(RuntimeError, match="sequence" + tail + "masked models are not supported"):
        hip_ns.UMPAModelDF(sam, ref, mask_list=mask, **kw).sequence(lam=0.1)
    with pytest.raises(RuntimeError, match="sequence" + tail + "frames at different positions"):
        hip_ns.UMPAModelNoDF(sam, ref, pos_list=[np.array(p) for p in ((0, 0), (2, 1), (1, 3))], **kw).sequence(lam=0.1)
    assert not hasattr(hip_ns.UMPAModelDFKernel(sam, ref, **kw), "sequence")
    with pytest.raises(RuntimeError, match="sequence: max_shift must be 2 to 8, not 9"):
        hip_ns.UMPAModelNoDF(sam, ref, window_size=1, max_shift=9).sequence(lam=0.1)
    m = hip_ns.UMPAModelDF(sam, ref, **kw)
    before = m.match(quiet=True)
    with pytest.raises(RuntimeError, match="sequence: .*grid"):
        m.sequence(lam=0.1, step=10)                                  # past the tiled path's limit: the library's refusal
    with pytest.raises(ValueError, match="sequence: lam must be a finite number"):
        m.sequence(lam=-1.0)
    with pytest.raises(ValueError, match="sequence: state must be of shape"):
        m.sequence(state=np.zeros((3, 3)), lam=0.1)
    # the library's own refusal of a search range it does not take, with its code and a text that names the value
    from umpa_amd import _lib
    g = _lib.grid()
    m9 = hip_ns.UMPAModelNoDF(sam, ref, window_size=1, max_shift=9)
    N0, N1 = m9.extent
    d = [np.zeros((N0, N1)) for _ in range(5)] + [None] + [np.zeros((N0, N1), np.int32) for _ in range(3)] + [np.zeros((N0, N1)), np.zeros((N0, N1)), np.zeros((N0, N1), np.int32)]
    rc = g.sequence(m9._handle, 0, 1, N0, 0, 1, N1, None, 0.0, INF, None, *[a.ctypes.data if a is not None else None for a in d], 0, None)
    assert rc == -4 and g.error() == "grid: sequence: max_shift must be 2 to 8, not 9", (rc, g.error())
    m.sequence(lam=0.1)
    after = m.match(quiet=True)                                       # the consumer was cleared: the walk is what it was
    for n in before:
        np.testing.assert_array_equal(before[n], after[n], err_msg=n)
