"""
The grid consumers on a masked model whose switch is on (model.masked_grid, umpa_grid_set_masked; libumpa_grid.so's masked_*
kernels), on the GPU: the cost volume against extended precision (tests/masked_grid_expect.py), the volume and the walk on one
table, the grid search against the extended-precision expectation, every consumer EQUAL to its numpy restatement on the device's
own masked volume, bit-identity across repeats, device arrays and row chunks, match_smooth, and the switch's default.

REACHES names, per test, the kernels of libumpa_grid.so it is there for (tests/test_masked_grid_cpu.py checks on the CPU that
every masked_* kernel of the built library is claimed here, and that no claim is stale).
"""
import ctypes

import numpy as np
import pytest

from conftest import assert_parity

import basins_expect as BE
import consumer_expect as CE
import grid_expect as GE
import masked_grid_expect as ME
import sequence_expect as SE
import track_expect as TE

pytestmark = pytest.mark.gpu

T = "tests/test_hip_masked_grid.py::"
REACHES = {
    T + "test_cost_volume_against_extended_precision": ["masked_volume_kernel<0>", "masked_volume_kernel<1>"],
    T + "test_grid_search_against_extended_precision": ["masked_min_kernel<0>", "masked_min_kernel<1>"],
    T + "test_basins_equal_their_restatement": ["masked_basins_kernel<0>", "masked_basins_kernel<1>"],
    T + "test_track_equals_its_restatement": ["masked_track_kernel<0>", "masked_track_kernel<1>"],
    T + "test_sequence_equals_its_restatement": ["masked_sequence_kernel<0>", "masked_sequence_kernel<1>"],
}
TODAY = "masked models are not supported (their table holds finished costs)"
INF = float("inf")
MODES = [(0, "sam"), (0, "ref"), (1, "sam"), (1, "ref")]
MODE_IDS = ["%s-%s" % ("DF" if k else "NoDF", a) for k, a in MODES]
SMALL = "64x72x3"


@pytest.fixture(scope="module")
def hip_ns():
    from umpa_amd import _lib, model
    if _lib.hip().device_count() < 1:
        pytest.fail("no HIP device: the GPU tests cannot run (there is no CPU fallback)")
    return model


def _model(hip_ns, name, which, kind, assign="sam", subpx=-1, on=True):
    sam, ref, c = ME.stack(name)
    m = (hip_ns.UMPAModelDF if kind else hip_ns.UMPAModelNoDF)(sam, ref, mask_list=ME.masks(name)[which], window_size=c["Nw"],
                                                              max_shift=c["ms"])
    m.assign_coordinates = assign
    m.sub_pixel_mode = subpx
    if on:
        m.masked_grid = True
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


def _bare(d):
    """a result without the key the masked models add (the restatements and the siblings' assert_equal know the plain keys)"""
    return {n: v for n, v in d.items() if n != "covered"}


def _same(a, b, what=""):
    assert sorted(a) == sorted(b), what
    for k in a:
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg="%s %s" % (what, k))


# ----------------------------------------------------------------------------- 1. the volume against extended precision

@pytest.mark.parametrize("name,which,kind,assign", ME.CASES, ids=ME.IDS)
def test_cost_volume_against_extended_precision(hip_ns, name, which, kind, assign):
    """Dead cells (wt = 0 in hp_cells) are not < +Inf and not -Inf on the device; every other cell is within hp's bound, and
    the device may turn one non-finite only where the window is rank-deficient (hp's bound >= |cost|, or fewer weighted pixels
    than parameters: masked_grid_expect.hp); T and df at the parity helper's tolerance on the well-posed cells.  Measured on an
    MI355X: no cell with weight is non-finite on the device; max |gpu - hp| / bound 0.057 (plain), 0.029 (dark-field) over the
    sixteen cases, so the pair weight's extra roundings need no term of their own.  Then the walk forced onto the tiled path:
    every known cell of its memo is the volume's entry, bit for bit."""
    from oracle import hp_cost
    from umpa_amd import _lib
    m = _model(hip_ns, name, which, kind, assign, 0)
    ms = m.max_shift
    (vol, only), seen = _launches(m, lambda: (m.cost_volume(with_fit=True), m.cost_volume()))
    assert seen.get("corr_masked", 0) >= 2 and seen.get("table_consumer") == 2 and "replay_cost" not in seen, seen
    v = ME.hp(name, which, kind, assign)
    cost = vol["cost"]
    assert cost.shape == v["cost"].shape == (2 * ms - 1, 2 * ms - 1) + m.extent
    assert sorted(vol) == sorted(["cost", "T", "covered"] + (["df"] if kind else []))
    assert sorted(only) == ["cost", "covered"]
    np.testing.assert_array_equal(only["cost"], cost)
    np.testing.assert_array_equal(vol["covered"], ME.covered(name, which))
    assert vol["covered"].dtype == np.bool_
    dead, deficient = v["dead"], v["deficient"]
    with np.errstate(invalid="ignore"):
        assert not (cost[dead] < INF).any() and not (cost[dead] == -INF).any()
    # (a window with fewer weighted pixels than parameters has singular normal equations: hp's numbers there are NaN or the
    # quotient of two rounding residues, masked_grid_expect.hp; it is among the rank-deficient cells, and hp says nothing of
    # the device's number there)
    valued = np.isfinite(v["cost"].astype(np.float64)) & ~v["singular"]
    assert not (~dead & ~valued & ~deficient).any()
    lost = ~dead & ~np.isfinite(cost)
    held = valued & np.isfinite(cost)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.abs(cost.astype(np.longdouble) - v["cost"]) / v["bound"]
    well = held & ~deficient
    rT = np.abs(vol["T"][well] - v["T"][well]) / np.abs(v["T"][well])
    print("%s %s kind %d %s: dead %d, rank-deficient %d of which non-finite on the device %d, max |gpu - hp| / bound %.4f "
          "(well-posed %.4f), T rel %.2e" % (name, which, kind, assign, dead.sum(), deficient.sum(), lost.sum(), ratio[held].max(),
                                             ratio[well].max(), rT.max()), end="")
    assert not (lost & ~deficient).any(), "%d well-posed cells are not finite on the device" % (lost & ~deficient).sum()
    assert lost.sum() <= deficient.sum()
    assert np.all(ratio[held] <= 1.0), "max |gpu - hp| / bound = %.4f" % ratio[held].max()
    assert np.all(rT <= CE.RTOL)
    if kind:
        rdf = np.abs(vol["df"][well] - v["df"][well]) / np.abs(v["df"][well])
        print(", df rel %.2e" % rdf.max(), end="")
        assert np.all(rdf <= CE.RTOL)
    print()
    # 2. the volume and the walk read one table
    m._force = _lib.F_FORCE_TILED
    walk, seen = _launches(m, lambda: m.match(quiet=True))
    m._force = 0
    assert seen.get("replay_cost", 0) >= 1 and "table_consumer" not in seen, seen
    (xi, xj, q), _, (si, sj) = hp_cost.memo_cells(walk, m.padding)
    assert xi.size > 10 * walk["err"].sum() > 0
    np.testing.assert_array_equal(walk["debug_d"][xi, xj, q], cost[si + ms - 1, sj + ms - 1, xi, xj])


# ----------------------------------------------------------------------------- 3. the grid search

@pytest.mark.parametrize("name,which,kind,assign", ME.CASES, ids=ME.IDS)
def test_grid_search_against_extended_precision(hip_ns, name, which, kind, assign):
    """Against grid_expect.expected fed with the masked extended-precision volumes, outside the near-tie mask and on the pixels
    whose costs are finite at every shift; the pixels below the coverage threshold keep their zeros, the pixels without a
    finite cost have err = 0 and zeros; everywhere, the minimum is the first strict minimum of the device's own volume."""
    v = ME.hp(name, which, kind, assign)
    none, some, whole = ME.pixel_classes(v)
    cov = ME.covered(name, which)
    keys = ("err", "debug_Ncalls", "dx", "dy", "f", "T", "debug_a", "debug_d") + (("df",) if kind else ())
    for subpx in (0, -1, 1):
        m = _model(hip_ns, name, which, kind, assign, subpx)
        got, seen = _launches(m, lambda: m.match(quiet=True, search="grid"))
        assert seen.get("table_consumer", 0) >= 1 and "replay_cost" not in seen, seen
        exp, near, _ = ME.expected_for(name, which, kind, assign, subpx)
        judged = whole & ~near & cov
        assert judged.mean() > 0.8
        # skipped pixels keep the zeros they were allocated with
        for k in keys:
            assert not np.asarray(got[k])[~cov].any(), k
        # no finite cost (all of them are uncovered in these stacks too, but the rule is the kernel's): err 0 and zeros
        assert not got["err"][none].any() and not any(np.asarray(got[k])[none].any() for k in ("dx", "dy", "f", "T"))
        want = {k: exp[k] for k in keys}
        mine = {k: np.array(got[k]) for k in keys}
        for k in keys:
            mine[k][~judged] = want[k][~judged]
        if subpx == 0:
            np.testing.assert_array_equal(got["dy"][judged], exp["ci"][judged])
            np.testing.assert_array_equal(got["dx"][judged], exp["cj"][judged])
        st = assert_parity(mine, want, m.max_shift, "masked grid %s %s %s %s subpx %d" % (name, which, "DF" if kind else "NoDF", assign, subpx),
                           subpx=subpx)
        print("%s %s kind %d %s subpx %d: judged %d of %d pixels (near-tie %d, some NaN %d, none %d, uncovered %d), ok %d" % (
            name, which, kind, assign, subpx, judged.sum(), judged.size, near.sum(), some.sum(), none.sum(), (~cov).sum(), st["ok"]))
        if subpx == 0:
            # every covered pixel, NaN shifts or not: the first strict minimum of the device's own volume and the err rule
            vol = m.cost_volume()["cost"]
            ci, cj, cmin, found = CE.first_strict_minimum(vol)
            err, ip, jp = CE.grid_err_rule(ci, cj, vol, m.max_shift)
            sel = cov & found
            np.testing.assert_array_equal(got["debug_d"][..., 12][sel], cmin[sel])
            np.testing.assert_array_equal(got["err"][sel], err[sel])
            np.testing.assert_array_equal(got["dy"][sel & (err == 0)], ci[sel & (err == 0)])
            np.testing.assert_array_equal(got["dx"][sel & (err == 0)], cj[sel & (err == 0)])
            np.testing.assert_array_equal(got["f"][sel & (err == 1)], (1.0 - ip)[sel & (err == 1)])
            assert not got["err"][cov & ~found].any()
            np.testing.assert_array_equal(got["debug_Ncalls"][cov], vol.shape[0] ** 2)


# ----------------------------------------------------------------------------- 4. the consumers EQUAL their restatements

def _volume(m, **region):
    vol = m.cost_volume(with_fit=True, **region)
    fin = np.isfinite(vol["cost"])
    U = fin.shape[0]
    n = fin.reshape((U * U,) + fin.shape[2:]).sum(axis=0)
    assert (n == 0).any() and ((n > 0) & (n < U * U)).any(), "the volume has pixels with NaN at all and at some shifts"
    return vol


def _fit(m):
    return BE.device_fit(m.sub_pixel_mode, m._device) if m.sub_pixel_mode else None


@pytest.mark.parametrize("kind,assign", MODES, ids=MODE_IDS)
def test_basins_equal_their_restatement(hip_ns, kind, assign):
    for which, subpx in (("binary", -1), ("real", 1), ("binary", 0)):
        m = _model(hip_ns, SMALL, which, kind, assign, subpx)
        vol = _volume(m)
        for k in (1, 4, 8):
            b = m.basins(k=k)
            want = BE.restate(vol["cost"], vol["T"], vol.get("df"), k, subpx, fit=_fit(m))
            BE.assert_equal(_bare(b), want, "%s k %d subpx %d" % (which, k, subpx))
            np.testing.assert_array_equal(b["covered"], vol["covered"])
        # rank 0 is the grid minimum: at every pixel against the volume, at covered pixels against match(search='grid')
        g = m.match(quiet=True, search="grid")
        cov = vol["covered"]
        for n in ("dx", "dy", "f", "T") + (("df",) if kind else ()):
            np.testing.assert_array_equal(b[n][0][cov], g[n][cov], err_msg=n)
        np.testing.assert_array_equal(np.maximum(b["err"][0], 0)[cov], g["err"][cov])


def _prior(ms, shape, seed):
    rng = np.random.default_rng(seed)
    pdx, pdy = (ms - 1) * (2 * rng.random(shape) - 1), (ms - 1) * (2 * rng.random(shape) - 1)
    pdx[rng.random(shape) < 0.05] = np.nan                               # NaN priors: the data term decides
    pdy[rng.random(shape) < 0.05] = np.nan
    return pdx, pdy


@pytest.mark.parametrize("kind,assign", MODES, ids=MODE_IDS)
def test_track_equals_its_restatement(hip_ns, kind, assign):
    for which, subpx in (("binary", -1), ("real", 0)):
        m = _model(hip_ns, SMALL, which, kind, assign, subpx)
        vol = _volume(m)
        pdx, pdy = _prior(m.max_shift, m.sh, 31)
        for lam, radius in ((None, None), (None, 2.5), (0.02, None), (0.02, 3.0), (0.0, None)):
            t = m.track(pdx, pdy, lam=lam, radius=radius)
            want = TE.restate(vol["cost"], vol["T"], vol.get("df"), pdy, pdx, TE.NEAREST if lam is None else TE.PENALTY,
                              0.0 if lam is None else lam, radius, subpx, fit=_fit(m))
            TE.assert_equal(_bare(t), want, "%s lam %r radius %r" % (which, lam, radius))
            np.testing.assert_array_equal(t["covered"], vol["covered"])
        # track(lam=0) is the grid search: the last case, on finite priors
        t0 = m.track(0.0, 0.0, lam=0.0)
        g = m.match(quiet=True, search="grid")
        cov = vol["covered"]
        for n in ("dx", "dy", "f", "T", "err") + (("df",) if kind else ()):
            np.testing.assert_array_equal(t0[n][cov], g[n][cov], err_msg=n)
        ci, cj, cmin, found = CE.first_strict_minimum(vol["cost"])
        np.testing.assert_array_equal(t0["shift"][0][found], ci[found])
        np.testing.assert_array_equal(t0["shift"][1][found], cj[found])
        assert (t0["found"][~found] == 0).all()


@pytest.mark.parametrize("kind,assign", MODES, ids=MODE_IDS)
def test_sequence_equals_its_restatement(hip_ns, kind, assign):
    for which, subpx in (("binary", -1), ("real", 0)):
        m = _model(hip_ns, SMALL, which, kind, assign, subpx)
        vol = _volume(m)
        args = (vol["cost"], vol["T"], vol.get("df"))
        # no state, then two steps with lam > 0, finite and infinite trunc
        s0 = m.sequence(lam=0.3)
        SE.assert_equal(_bare(s0), SE.restate(*args, None, 0.3, None, subpx, fit=_fit(m)), "%s no state" % which)
        scale = float(np.median(vol["cost"][np.isfinite(vol["cost"])]))
        lam = 0.05 * scale
        for trunc in (None, 0.5 * scale):
            s1 = m.sequence(state=s0["state"], lam=lam, trunc=trunc)
            SE.assert_equal(_bare(s1), SE.restate(*args, s0["state"], lam, trunc, subpx, fit=_fit(m)), "%s step 1 trunc %r" % (which, trunc))
            s2 = m.sequence(state=s1["state"], lam=lam, trunc=trunc)
            SE.assert_equal(_bare(s2), SE.restate(*args, s1["state"], lam, trunc, subpx, fit=_fit(m)), "%s step 2 trunc %r" % (which, trunc))
            np.testing.assert_array_equal(s2["covered"], vol["covered"])
        # lam = 0 and no state are the grid search
        g = m.match(quiet=True, search="grid")
        cov = vol["covered"]
        for s in (s0, m.sequence(state=s0["state"], lam=0.0, trunc=0.2 * scale)):
            for n in ("dx", "dy", "f", "T", "err") + (("df",) if kind else ()):
                np.testing.assert_array_equal(s[n][cov], g[n][cov], err_msg=n)
            assert not s["moved"].any()


# ----------------------------------------------------------------------------- 5. bit-identical

def _five(m, pdx, pdy, state, **region):
    """the five calls of one region as dictionaries of numpy arrays"""
    out = {"grid": m.match(quiet=True, search="grid", **region)}
    m.ROI = None
    out["volume"] = m.cost_volume(with_fit=True, **region)
    out["basins"] = m.basins(k=5, **region)
    out["track"] = m.track(pdx, pdy, lam=0.02, radius=3.0, **region)
    out["sequence"] = m.sequence(state=state, lam=0.01, trunc=0.5, **region)
    return {k: {n: np.asarray(a) for n, a in v.items() if not n.startswith("_")} for k, v in out.items()}


def _cut(d, s0, s1):
    """the pixels (s0, s1) of every map of a result: the pixel axes are the last two, of debug_d and debug_a the first two"""
    return {n: np.ascontiguousarray(a[s0, s1] if n in ("debug_d", "debug_a") else a[..., s0, s1]) for n, a in d.items()}


def _chunk_inputs():
    """tests/test_hip_grid.py's chunk stack (128 x 512 output pixels, 81 shifts) with a mask of both kinds of damage: with
    UMPA_HIP_TABLE_MB=16 the masked table of NV planes per shift holds one 32-row piece, so a call takes several row chunks"""
    from umpa_amd.synth import make_stack
    sam, ref = make_stack(144, 528, 4, 5, df=True, seed=9, order=1)[:2]
    rng = np.random.default_rng(109)
    mask = (rng.random(sam.shape) >= 0.10).astype(np.float64)
    mask[:, 60:80, 200:230] = 0.0
    return sam, ref, mask


@pytest.mark.parametrize("kind", [0, 1], ids=["NoDF", "DF"])
def test_repeats_row_chunks_and_steps_change_nothing(hip_ns, kind, monkeypatch):
    sam, ref, mask = _chunk_inputs()
    res = {}
    for mb in (None, "16"):
        if mb:
            monkeypatch.setenv("UMPA_HIP_TABLE_MB", mb)
        else:
            monkeypatch.delenv("UMPA_HIP_TABLE_MB", raising=False)
        m = (hip_ns.UMPAModelDF if kind else hip_ns.UMPAModelNoDF)(sam, ref, mask_list=mask, window_size=3, max_shift=5)
        m.masked_grid = True
        N0, N1 = m.extent
        pdx, pdy = _prior(5, (N0, N1), 7)
        state = np.random.default_rng(8).random((9, 9, N0, N1))
        res[mb], seen = _launches(m, lambda: _five(m, pdx, pdy, state))
        assert (seen.get("table_consumer") > 5) == bool(mb), (mb, seen)
        if mb is None:
            again = _five(m, pdx, pdy, state)
            for k in again:
                _same(again[k], res[None][k], "repeat " + k)
            # an ROI with steps (2, 3): slices of the full result (the dense table read strided) -- within the masked step
            # limit of the plain model (16); the dark-field model's limit is 5 and the same region is refused by name
            roi = ((17, 90, 2), (5, 400, 3))
            s0, s1 = slice(17, 90, 2), slice(5, 400, 3)
            if kind == 0:
                part = _five(m, np.ascontiguousarray(pdx[s0, s1]), np.ascontiguousarray(pdy[s0, s1]),
                             np.ascontiguousarray(state[:, :, s0, s1]), ROI=roi)
                for k in part:
                    _same(part[k], _cut(res[None][k], s0, s1), "ROI " + k)
            else:
                with pytest.raises(RuntimeError) as e:
                    m.cost_volume(ROI=roi)
                assert "steps 2 x 3" in str(e.value) and "step limit is 5" in str(e.value), str(e.value)
                roi, s0, s1 = ((17, 90, 2), (5, 400, 2)), slice(17, 90, 2), slice(5, 400, 2)
                part = _five(m, np.ascontiguousarray(pdx[s0, s1]), np.ascontiguousarray(pdy[s0, s1]),
                             np.ascontiguousarray(state[:, :, s0, s1]), ROI=roi)
                for k in part:
                    _same(part[k], _cut(res[None][k], s0, s1), "ROI " + k)
            # a step beyond the masked limit is refused by name, by every call, and the model works afterwards
            m.ROI = None
            far = ((0, 120, 5), (0, 500, 4))
            for call in (lambda: m.match(quiet=True, search="grid", ROI=far), lambda: m.cost_volume(ROI=far), lambda: m.basins(ROI=far),
                         lambda: m.track(0.0, 0.0, ROI=far), lambda: m.sequence(lam=0.0, ROI=far)):
                with pytest.raises(RuntimeError) as e:
                    call()
                assert "steps 5 x 4" in str(e.value) and "step limit is %d" % (5 if kind else 16) in str(e.value), str(e.value)
            m.ROI = None
            _same({n: np.asarray(a) for n, a in m.cost_volume(with_fit=True).items()}, res[None]["volume"], "after the refusals")
    for k in res[None]:
        _same(res["16"][k], res[None][k], "row chunks " + k)


@pytest.mark.parametrize("kind", [0, 1], ids=["NoDF", "DF"])
def test_device_arrays_on_a_side_stream(hip_ns, kind):
    import torch
    from umpa_amd import _lib
    m = _model(hip_ns, "96x112x4", "binary", kind, "sam", -1)
    N0, N1 = m.extent
    U, npar = 2 * m.max_shift - 1, m.Nparam
    pdx, pdy = _prior(m.max_shift, (N0, N1), 3)
    state = np.random.default_rng(4).random((U, U, N0, N1))
    host = _five(m, pdx, pdy, state)
    cov = np.ascontiguousarray(m.coverage())
    thr = .1 * cov.max() / 4
    dev = torch.device("cuda", m._device)
    stream = torch.cuda.Stream(device=dev)
    tdx, tdy, tstate, tcov = (torch.from_numpy(a).to(dev) for a in (pdx, pdy, state, cov))
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(stream):
        values = torch.zeros((N0, N1, npar), dtype=torch.float64, device=dev)
        err = torch.zeros((N0, N1), dtype=torch.int32, device=dev)
        dd = torch.zeros((N0, N1, 25), dtype=torch.float64, device=dev)
        da = torch.zeros((N0, N1, 16), dtype=torch.float64, device=dev)
        dn = torch.zeros((N0, N1), dtype=torch.int32, device=dev)
        g = _lib.grid()
        g.check(g.match_region(m._handle, 0, 1, N0, 0, 1, N1, values.data_ptr(), npar, None, err.data_ptr(), tcov.data_ptr(), thr,
                               dd.data_ptr(), da.data_ptr(), dn.data_ptr(), _lib.F_DEVICE_IO, ctypes.c_void_p(stream.cuda_stream)),
                "grid match_region")
        keys = ["cost", "T"] + (["df"] if kind else [])
        vols = m._grid_cost_volume(None, None, lambda U, N0, N1: {k: torch.empty((U, U, N0, N1), dtype=torch.float64, device=dev) for k in keys})[2]
        track = m.track(tdx, tdy, lam=0.02, radius=3.0)
        seq = m.sequence(state=tstate, lam=0.01, trunc=0.5)

        def alloc(k, N0, N1):
            out = {n: torch.empty((k, N0, N1), dtype=torch.float64, device=dev) for n in ["f", "T", "dx", "dy", "cost"] + (["df"] if kind else [])}
            out.update({n: torch.empty((k, N0, N1), dtype=torch.int32, device=dev) for n in ("si", "sj", "err")})
            out["count"] = torch.empty((N0, N1), dtype=torch.int32, device=dev)
            return out
        basins = m._grid_basins(5, None, None, alloc)[2]
    stream.synchronize()
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for n, t in list(track.items()) + list(seq.items()) if n != "covered")
    v = values.cpu().numpy()
    for q, k in enumerate(("f", "T", "dx", "dy") + (("df",) if kind else ())):
        np.testing.assert_array_equal(v[..., q], host["grid"][k], err_msg=k)
    for k, t in (("err", err), ("debug_d", dd), ("debug_a", da), ("debug_Ncalls", dn)):
        np.testing.assert_array_equal(t.cpu().numpy(), host["grid"][k], err_msg=k)
    for k in keys:
        np.testing.assert_array_equal(vols[k].cpu().numpy(), host["volume"][k], err_msg="volume " + k)
    assert track["covered"].dtype == np.bool_ and np.array_equal(track["covered"], host["track"]["covered"])
    TE.assert_equal(_bare(track), _bare(host["track"]), "track on device arrays")
    SE.assert_equal(_bare(seq), _bare(host["sequence"]), "sequence on device arrays")
    got = {n: t.cpu().numpy() for n, t in basins.items()}
    got["shift"] = np.stack([got.pop("si"), got.pop("sj")], axis=1)
    BE.assert_equal(got, {n: a for n, a in host["basins"].items() if n != "covered"}, "basins on device arrays")


# ----------------------------------------------------------------------------- 6. match_smooth

@pytest.mark.parametrize("kind", [0, 1], ids=["NoDF", "DF"])
def test_match_smooth_is_aggregate_on_the_model_s_own_volume(hip_ns, kind):
    import torch
    from umpa_amd import smooth
    m = _model(hip_ns, SMALL, "binary", kind, "sam", -1)
    got = smooth.match_smooth(m, lam=0.02, trunc=0.3)
    vol = m.cost_volume()["cost"]
    agg = smooth.aggregate(torch.from_numpy(vol).to(torch.device("cuda", m._device)), 0.02, 0.3)
    start = agg["shift"].cpu().numpy()
    np.testing.assert_array_equal(got["start"], start)
    want = m.match(dxdy=(start[0], start[1]), quiet=True)
    for k in ("dx", "dy", "f", "T", "err") + (("df",) if kind else ()):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    np.testing.assert_array_equal(got["valid"], agg["valid"].cpu().numpy())


# ----------------------------------------------------------------------------- 7. off by default

@pytest.mark.parametrize("kind", [0, 1], ids=["NoDF", "DF"])
def test_default_off_then_on_and_off_again(hip_ns, kind):
    from umpa_amd import _lib
    m = _model(hip_ns, SMALL, "binary", kind, "sam", -1, on=False)
    assert m.masked_grid is False
    before = m.match(quiet=True)
    calls = [("search='grid'", lambda: m.match(quiet=True, search="grid")), ("cost_volume", lambda: m.cost_volume()),
             ("basins", lambda: m.basins()), ("track", lambda: m.track(0.0, 0.0)), ("sequence", lambda: m.sequence(lam=0.0))]

    def refused():
        for what, call in calls:
            with pytest.raises(RuntimeError) as e:
                call()
            assert str(e.value) == "%s (grid search / cost volume): %s" % (what, TODAY), what
        # and past the Python layer: the library's own refusal, with the code and the text it always had
        g = _lib.grid()
        n0, n1 = m.extent
        v2, e2 = np.zeros((n0, n1, 5)), np.zeros((n0, n1), np.int32)
        cov = np.ascontiguousarray(m.coverage())
        rc = g.match_region(m._handle, 0, 1, n0, 0, 1, n1, v2.ctypes.data, m.Nparam, None, e2.ctypes.data, cov.ctypes.data, 0.1,
                            None, None, None, 0, None)
        assert rc == -4 and "a table consumer is set (grid search / cost volume): the plain tiled path does not take" in g.error(), (rc, g.error())
        _same(m.match(quiet=True), before, "the walk")

    refused()
    m.masked_grid = True
    assert m.masked_grid is True
    on = [call() for _, call in calls]
    assert all("covered" in r for r in on[1:]) and "covered" not in on[0]
    _same(m.match(quiet=True), before, "the walk with the switch on")
    m.masked_grid = False
    assert m.masked_grid is False
    refused()
    m.masked_grid = True
    again = [call() for _, call in calls]
    for a, b in zip(on, again):
        _same({n: v for n, v in a.items() if not n.startswith("_")}, {n: v for n, v in b.items() if not n.startswith("_")}, "on again")
    # window widening and scale space stay refused, by the library too
    g = _lib.grid()
    n0, n1 = m.extent
    U = 2 * m.max_shift - 1
    vol = np.zeros((U, U, n0, n1))
    rc = g.wide_cost_volume(m._handle, 0, 1, n0, 0, 1, n1, 2, vol.ctypes.data, None, None, 0, None)
    assert rc == -4 and "not linear in the windowed sums" in g.error(), (rc, g.error())
    with pytest.raises(RuntimeError, match="not linear in the windowed sums"):
        m.cost_volume(widen=1)
    # a model without masks: the switch changes nothing and stays off
    sam, ref, c = ME.stack(SMALL)
    plain = (hip_ns.UMPAModelDF if kind else hip_ns.UMPAModelNoDF)(sam, ref, window_size=c["Nw"], max_shift=c["ms"])
    a = plain.cost_volume(widen=1)
    plain.masked_grid = True
    assert plain.masked_grid is False
    b = plain.cost_volume(widen=1)
    assert sorted(a) == sorted(b) == ["cost", "region"]
    np.testing.assert_array_equal(a["cost"], b["cost"])
