"""
Window widening on the GPU: ``widen=b`` on match(search='grid'), cost_volume, basins and track (umpa_grid_wide_*,
libumpa_grid.so).  The widened volume is judged against extended precision under the window W' (tests/widen_expect.py:
oracle/hp_cost.py given W', its fp64 bound scaled for the pooled route); the rules of the consumers are then checked bit
for bit on the device's own widened volume, as tests/test_hip_basins.py and tests/test_hip_track.py do without widening.

REACHES names, per test, the widen kernels of libumpa_grid.so it is there for (tests/test_widen_cpu.py checks on the CPU
that every widen_* kernel symbol of the built library is claimed here, and that no claim is stale).
"""
import ctypes
import functools

import numpy as np
import pytest

import basins_expect as BE
import grid_expect as GE
import track_expect as TE
import widen_expect as WE
from conftest import assert_parity

pytestmark = pytest.mark.gpu

MAXB = 8                         # UMPA_GRID_MAX_WIDEN
REACHES = {
    "tests/test_hip_widen.py::test_every_half_width": ["widen_table_kernel<%d, false>" % b for b in range(1, MAXB + 1)]
                                                      + ["widen_map_kernel<%d, %s>" % (b, p) for b in range(1, MAXB + 1) for p in ("false", "true")],
    "tests/test_hip_widen.py::test_strip_blocked_input": ["widen_table_kernel<%d, true>" % b for b in range(1, MAXB + 1)],
    "tests/test_hip_widen.py::test_row_chunks_change_nothing": ["widen_carry_kernel"],
}
NAN = float("nan")


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


def _np(a):
    return a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)


def _same(a, b, what=""):
    """two result dictionaries, bit for bit (NaN == NaN), the region included"""
    assert sorted(a) == sorted(b), (what, sorted(a), sorted(b))
    for k in a:
        if k == "region":
            assert tuple(a[k]) == tuple(b[k]), (what, a[k], b[k])
        else:
            np.testing.assert_array_equal(_np(a[k]), _np(b[k]), err_msg="%s %s" % (what, k))


def _maps(res):
    return {k: v for k, v in res.items() if k != "region"}


def _full_region(m, b):
    N0, N1 = m.extent
    return ((b, N0 - b, 1), (b, N1 - b, 1))


def _within(vol, hp, kind, what):
    """every entry of a widened volume within the scaled bound of its extended-precision value; T and df within the bar"""
    ratio = np.abs(vol["cost"].astype(np.longdouble) - hp["cost"]) / hp["bound"]
    rT = np.abs(vol["T"] - hp["T"]) / np.abs(hp["T"])
    print("%s: max |gpu - hp| / bound %.4f, T rel %.2e" % (what, ratio.max(), rT.max()), end="")
    assert np.all(ratio <= 1.0), "%s: max |gpu - hp| / bound = %.4f" % (what, ratio.max())
    assert np.all(rT <= 1e-5), what
    if kind:
        rdf = np.abs(vol["df"] - hp["df"]) / np.abs(hp["df"])
        print(", df rel %.2e" % rdf.max(), end="")
        assert np.all(rdf <= 1e-5), what
    print()


HP_CASES = [(n, b, k, a) for (n, b) in WE.CASES for k in (0, 1) for a in ("sam", "ref")]
HP_IDS = ["%s-b%d-%s-%s" % (n, b, "DF" if k else "NoDF", a) for n, b, k, a in HP_CASES]


# ----------------------------------------------------------------------------- 1. the volume against extended precision

@pytest.mark.parametrize("name,b,kind,assign", HP_CASES, ids=HP_IDS)
def test_volume_against_extended_precision(hip_ns, name, b, kind, assign):
    sam, ref, c = GE.stack(name)
    ms = c["ms"]
    m = _model(hip_ns, kind, sam, ref, c["Nw"], ms, assign)
    vol = m.cost_volume(with_fit=True, widen=b)
    hp = WE.volumes_for(name, b, kind, assign)
    assert tuple(vol.pop("region")) == _full_region(m, b)
    assert vol["cost"].shape == hp["cost"].shape == (2 * ms - 1, 2 * ms - 1, m.extent[0] - 2 * b, m.extent[1] - 2 * b)
    assert sorted(vol) == ["T", "cost"] + (["df"] if kind else [])
    _within(vol, hp, kind, "%s b %d kind %d %s" % (name, b, kind, assign))


@pytest.mark.parametrize("kind", [0, 1], ids=["NoDF", "DF"])
def test_the_border_ring_is_nan_cell_for_cell(hip_ns, kind):
    """the library's own call on the whole extent (no growing, no cropping): the first and last b rows and columns are NaN in
    every plane, every other cell is the number the cropped Python call returns; the other consumers follow their NaN rules"""
    from umpa_amd import _lib
    sam, ref, c = GE.stack("64x72x3")
    b, ms = 2, c["ms"]
    m = _model(hip_ns, kind, sam, ref, c["Nw"], ms)
    N0, N1 = m.extent
    U = 2 * ms - 1
    g = _lib.grid()
    out = {k: np.full((U, U, N0, N1), -7.0) for k in ("cost", "T") + (("df",) if kind else ())}
    g.check(g.wide_cost_volume(m._handle, 0, 1, N0, 0, 1, N1, b, out["cost"].ctypes.data, out["T"].ctypes.data,
                               out["df"].ctypes.data if kind else None, 0, None), "wide_cost_volume")
    ring = np.ones((N0, N1), bool)
    ring[b:N0 - b, b:N1 - b] = False
    vol = m.cost_volume(with_fit=True, widen=b)
    for k, a in out.items():
        assert np.isnan(a[:, :, ring]).all() and np.isfinite(a[:, :, ~ring]).all(), k
        np.testing.assert_array_equal(a[:, :, b:N0 - b, b:N1 - b], vol[k], err_msg=k)
    # match_region: err = 0 and zeros; basins: count = 0; track: found = 0, err = -1
    values, err = np.full((m.Nparam, N0, N1), -7.0), np.full((N0, N1), -7, np.int32)
    g.check(g.wide_match_region(m._handle, 0, 1, N0, 0, 1, N1, b, values.ctypes.data, m.Nparam, None, err.ctypes.data, None, 0.0,
                                None, None, None, _lib.F_PLANAR, None), "wide_match_region")
    assert (err[ring] == 0).all() and (values[:, ring] == 0).all()
    grid = m.match(quiet=True, search="grid", widen=b)
    m.ROI = None
    np.testing.assert_array_equal(err[~ring].reshape(grid["err"].shape), grid["err"])
    np.testing.assert_array_equal(values[2][~ring].reshape(grid["dx"].shape), grid["dx"])
    dbl = {n: np.full((2, N0, N1), -7.0) for n in ("f", "T", "dx", "dy", "cost") + (("df",) if kind else ())}
    ints = {n: np.full((2, N0, N1), -7, np.int32) for n in ("si", "sj", "err")}
    count = np.full((N0, N1), -7, np.int32)
    p = lambda a: a.ctypes.data
    g.check(g.wide_basins(m._handle, 0, 1, N0, 0, 1, N1, b, 2, p(dbl["f"]), p(dbl["T"]), p(dbl["dx"]), p(dbl["dy"]), p(dbl["cost"]),
                          p(dbl["df"]) if kind else None, p(ints["si"]), p(ints["sj"]), p(ints["err"]), p(count), 0, None), "wide_basins")
    assert (count[ring] == 0).all() and (ints["err"][:, ring] == -1).all() and (count[~ring] >= 1).all()
    t = {n: np.full((N0, N1), -7.0) for n in ("f", "T", "dx", "dy", "cost", "cost0") + (("df",) if kind else ())}
    ti = {n: np.full((N0, N1), -7, np.int32) for n in ("si", "sj", "err", "count", "found")}
    prior = np.zeros((N0, N1))
    g.check(g.wide_track(m._handle, 0, 1, N0, 0, 1, N1, b, p(prior), p(prior), 0, 0.0, -1.0, p(t["f"]), p(t["T"]), p(t["dx"]), p(t["dy"]),
                         p(t["cost"]), p(t["df"]) if kind else None, p(ti["si"]), p(ti["sj"]), p(ti["err"]), p(t["cost0"]), p(ti["count"]),
                         p(ti["found"]), 0, None), "wide_track")
    assert (ti["found"][ring] == 0).all() and (ti["err"][ring] == -1).all() and (ti["count"][ring] == 0).all() and (t["cost0"][ring] == 0).all()
    assert (ti["found"][~ring] >= 1).all()


# ----------------------------------------------------------------------------- 2. the search against extended precision

@pytest.mark.parametrize("name,b,kind,assign", HP_CASES, ids=HP_IDS)
def test_search_against_extended_precision(hip_ns, name, b, kind, assign):
    sam, ref, c = GE.stack(name)
    ms, Nw = c["ms"], c["Nw"]
    hp = WE.volumes_for(name, b, kind, assign)
    for subpx in (-1, 0, 1):
        m = _model(hip_ns, kind, sam, ref, Nw, ms, assign, subpx)
        got = m.match(quiet=True, search="grid", widen=b)
        assert tuple(got.pop("region")) == _full_region(m, b)
        exp, near = GE.expected(kind, sam, ref, WE.window(Nw, b), ms, ms + Nw + b, assign, subpx, volumes=hp)
        assert near.mean() <= GE.NEAR_TIE_CAP
        want = {k: exp[k] for k in ("err", "debug_Ncalls", "dx", "dy", "f", "T", "debug_a", "debug_d") + (("df",) if kind else ())}
        got = {k: np.array(got[k]) for k in want}
        for k in want:                                                # near-tie pixels: out of both sides
            got[k][near] = want[k][near]
        st = assert_parity(got, want, ms, "widen %d %s %s %s subpx %d" % (b, name, "DF" if kind else "NoDF", assign, subpx), subpx=subpx)
        assert st["ok"] > 0.5 * near.size


# ----------------------------------------------------------------------------- 3. the rules, on the device's own widened volume

def _rules(m, b, what, **region):
    """grid search, basins(k = 8) and track in both modes against the restatements applied to cost_volume(widen=b)"""
    vol = m.cost_volume(with_fit=True, widen=b, **region)
    reg = vol.pop("region")
    sub = m.sub_pixel_mode
    fit = BE.device_fit(sub, m._device) if sub else None
    bas = m.basins(k=8, widen=b, **region)
    assert tuple(bas["region"]) == tuple(reg)
    BE.assert_equal(_maps(bas), BE.restate(vol["cost"], vol["T"], vol.get("df"), 8, sub, fit=fit), what + " basins")
    roi_before = m.ROI
    grid = m.match(quiet=True, search="grid", widen=b, **region)
    m.ROI = roi_before
    assert tuple(grid["region"]) == tuple(reg)
    for n in ("dx", "dy", "f", "T", "err") + (("df",) if "df" in vol else ()):
        np.testing.assert_array_equal(grid[n], bas[n][0], err_msg="%s grid against rank 0: %s" % (what, n))
    ms = m.max_shift
    rng = np.random.default_rng(11 + b)
    sh = vol["cost"].shape[2:]
    pdx, pdy = rng.uniform(-(ms + 1), ms + 1, sh), rng.uniform(-(ms + 1), ms + 1, sh)
    pdx[rng.random(sh) < 0.03] = NAN
    out = [grid, bas]
    for lam, radius in ((None, None), (0.05, 3.0)):
        t = m.track(pdx, pdy, lam=lam, radius=radius, widen=b, **region)
        assert tuple(t["region"]) == tuple(reg)
        want = TE.restate(vol["cost"], vol["T"], vol.get("df"), pdy, pdx, TE.NEAREST if lam is None else TE.PENALTY,
                          0.0 if lam is None else lam, radius, sub, fit=fit)
        TE.assert_equal(_maps(t), want, "%s track lam %r" % (what, lam))
        out.append(t)
    return vol, out


@pytest.mark.parametrize("kind", [0, 1], ids=["NoDF", "DF"])
@pytest.mark.parametrize("subpx", [-1, 0, 1])
def test_rules_on_the_widened_volume(hip_ns, kind, subpx):
    sam, ref, c = GE.stack("64x72x3")
    for assign, b in (("sam", 2), ("ref", 1)):
        m = _model(hip_ns, kind, sam, ref, c["Nw"], c["ms"], assign, subpx)
        _rules(m, b, "%s b %d subpx %d" % (assign, b, subpx))


# ----------------------------------------------------------------------------- 4. b = 0 is the sibling

def test_b_zero_is_the_sibling(hip_ns):
    from umpa_amd import _lib
    sam, ref, c = GE.stack("64x72x3")
    g = _lib.grid()
    p = lambda a: None if a is None else a.ctypes.data
    for kind in (0, 1):
        m = _model(hip_ns, kind, sam, ref, c["Nw"], c["ms"], subpx=-1)
        N0, N1 = m.extent
        U = 2 * c["ms"] - 1
        region = (m._handle, 0, 1, N0, 0, 1, N1)
        for wide in (False, True):
            fn = lambda name: getattr(g, ("wide_" if wide else "") + name)
            bz = (0,) if wide else ()
            res = {}
            v = [np.full((m.Nparam, N0, N1), -7.0), np.full((N0, N1), -7, np.int32), np.full((N0, N1, 25), -7.0), np.full((N0, N1, 16), -7.0),
                 np.full((N0, N1), -7, np.int32)]
            g.check(fn("match_region")(*region, *bz, p(v[0]), m.Nparam, None, p(v[1]), None, 0.0, p(v[2]), p(v[3]), p(v[4]), _lib.F_PLANAR, None), "match_region")
            res["match"] = v
            vol = [np.full((U, U, N0, N1), -7.0) for _ in range(3 if kind else 2)]
            g.check(fn("cost_volume")(*region, *bz, p(vol[0]), p(vol[1]), p(vol[2]) if kind else None, 0, None), "cost_volume")
            res["volume"] = vol
            d = [np.full((3, N0, N1), -7.0) for _ in range(6)]
            q = [np.full((3, N0, N1), -7, np.int32) for _ in range(3)] + [np.full((N0, N1), -7, np.int32)]
            g.check(fn("basins")(*region, *bz, 3, *[p(a) for a in d[:5]], p(d[5]) if kind else None, *[p(a) for a in q], 0, None), "basins")
            res["basins"] = d[:5 + kind] + q
            pr = np.full((N0, N1), 0.5)
            d = [np.full((N0, N1), -7.0) for _ in range(7)]
            q = [np.full((N0, N1), -7, np.int32) for _ in range(5)]
            g.check(fn("track")(*region, *bz, p(pr), p(pr), 1, 0.05, 3.0, *[p(a) for a in d[:5]], p(d[5]) if kind else None,
                                p(q[0]), p(q[1]), p(q[2]), p(d[6]), p(q[3]), p(q[4]), 0, None), "track")
            res["track"] = d[:5 + kind] + [d[6]] + q
            if wide:
                for name in res:
                    for n, (x, y) in enumerate(zip(res[name], sibling[name])):
                        np.testing.assert_array_equal(x, y, err_msg="%s array %d" % (name, n))
            else:
                sibling = res


# ----------------------------------------------------------------------------- 5. every instantiation

def _lattice(shape, n, seed):
    """a seeded sample of n pixels of maps of `shape`: (xi, xj)"""
    rng = np.random.default_rng(seed)
    flat = rng.choice(shape[0] * shape[1], size=min(n, shape[0] * shape[1]), replace=False)
    return flat // shape[1], flat % shape[1]


@pytest.mark.parametrize("b", list(range(1, MAXB + 1)))
def test_every_half_width(hip_ns, b):
    """every half-width on corr_volume's plain table, both models (the map kernel of doubles, and of frame pairs with an odd
    tail: K = 3): a seeded sample of pixels against extended precision, and the rules on the whole widened volume"""
    from umpa_amd.synth import make_stack
    Nw, ms, K = 2, 3, 3
    sam, ref, _ = make_stack(48, 84, K, ms, df=True, seed=500 + b)
    for kind, assign in ((1, "sam"), (0, "ref")):
        m = _model(hip_ns, kind, sam, ref, Nw, ms, assign, -1)
        (vol, _), seen = _launches(m, lambda: _rules(m, b, "b %d kind %d" % (b, kind)))
        assert seen.get("table_consumer") == 5 and "replay_walk" not in seen, seen
        assert vol["cost"].shape[2:] == (m.extent[0] - 2 * b, m.extent[1] - 2 * b)
        xi, xj = _lattice(vol["cost"].shape[2:], 150, b)
        hp = WE.volumes(kind, sam, ref, Nw, b, ms, assign, pixels=(xi, xj))
        _within({k: v[:, :, xi, xj] for k, v in vol.items()}, hp, kind, "b %d kind %d" % (b, kind))


@pytest.mark.parametrize("K", [1, 2, 3, 25])
def test_frame_counts(hip_ns, K):
    """the pair planes with and without an odd tail, and the generic path beyond UMPA_KTEMPL frames"""
    from umpa_amd.synth import make_stack
    Nw, ms, b = 2, 3, 1
    sam, ref, _ = make_stack(44, 80, K, ms, df=True, seed=100 + K)
    for assign in ("sam", "ref"):
        m = _model(hip_ns, 1, sam, ref, Nw, ms, assign, 0)
        vol, _ = _rules(m, b, "K %d %s" % (K, assign))
        xi, xj = _lattice(vol["cost"].shape[2:], 150, K)
        hp = WE.volumes(1, sam, ref, Nw, b, ms, assign, pixels=(xi, xj))
        _within({k: v[:, :, xi, xj] for k, v in vol.items()}, hp, 1, "K %d %s" % (K, assign))


@pytest.mark.parametrize("b", list(range(1, MAXB + 1)))
def test_strip_blocked_input(hip_ns, b):
    """corr_march's strip-blocked table as the input (wide windows), the pooled table in the plain layout"""
    from umpa_amd.synth import make_stack
    Nw, K, ms = 6, 3, 3
    sam, ref, _ = make_stack(66, 92, K, ms, df=True, seed=77, order=1)
    m = _model(hip_ns, 1, sam, ref, Nw, ms, "sam", 0)
    vol, seen = _launches(m, lambda: m.cost_volume(with_fit=True, widen=b))
    assert seen.get("corr_march", 0) >= 1 and "corr_volume" not in seen and seen.get("table_consumer") == 1, seen
    vol.pop("region")
    assert vol["cost"].shape[2:] == (m.extent[0] - 2 * b, m.extent[1] - 2 * b)
    xi, xj = _lattice(vol["cost"].shape[2:], 200, 40 + b)
    hp = WE.volumes(1, sam, ref, Nw, b, ms, "sam", pixels=(xi, xj))
    _within({k: v[:, :, xi, xj] for k, v in vol.items()}, hp, 1, "strip-blocked b %d" % b)
    grid = m.match(quiet=True, search="grid", widen=b)
    U = 2 * ms - 1
    arg = np.argmin(vol["cost"].reshape((U * U,) + vol["cost"].shape[2:]), axis=0)
    np.testing.assert_array_equal(grid["dy"], arg // U - (ms - 1))
    np.testing.assert_array_equal(grid["dx"], arg % U - (ms - 1))


# ----------------------------------------------------------------------------- 6. row chunks, regions

def _chunk_stack():
    from umpa_amd.synth import make_stack
    # 128 x 512 output pixels, 81 planes of 512 doubles per row: a 16 MB table holds 32 rows -> four row chunks
    return make_stack(144, 528, 4, 5, df=True, seed=9, order=1)[:2]


def _four(m, b, **region):
    """the four consumers of a region: [grid, volume, basins, track]"""
    roi = m.ROI
    grid = m.match(quiet=True, search="grid", widen=b, **region)
    m.ROI = roi
    sh = grid["dx"].shape
    rng = np.random.default_rng(5)
    pdx, pdy = rng.uniform(-5, 5, sh), rng.uniform(-5, 5, sh)
    return [grid, m.cost_volume(with_fit=True, widen=b, **region), m.basins(k=3, widen=b, **region),
            m.track(pdx, pdy, lam=0.02, radius=4.0, widen=b, **region)]


@pytest.mark.parametrize("b", [1, 3, 8])
def test_row_chunks_change_nothing(hip_ns, monkeypatch, b):
    sam, ref = _chunk_stack()
    res = {}
    for mb in (None, "16"):
        if mb:
            monkeypatch.setenv("UMPA_HIP_TABLE_MB", mb)
        else:
            monkeypatch.delenv("UMPA_HIP_TABLE_MB", raising=False)
        m = _model(hip_ns, 1, sam, ref, 3, 5, subpx=-1)
        res[mb], seen = _launches(m, lambda: _four(m, b))
        assert seen.get("table_consumer") == 4 * (4 if mb else 1), (mb, seen)
    for name, one, four in zip(("grid", "volume", "basins", "track"), res[None], res["16"]):
        _same(one, four, "b %d, four chunks: %s" % (b, name))
    assert res[None][1]["cost"].shape[2:] == (128 - 2 * b, 512 - 2 * b) and np.isfinite(res[None][1]["cost"]).all()


def test_roi_and_steps_are_slices_of_the_full_result(hip_ns):
    from umpa_amd import widen
    sam, ref = _chunk_stack()
    b = 2
    for kind in (0, 1):
        m = _model(hip_ns, kind, sam, ref, 3, 5, subpx=-1)
        full = _four(m, b)
        N0, N1 = m.extent
        assert all(tuple(r["region"]) == ((b, N0 - b, 1), (b, N1 - b, 1)) for r in full)

        def cut(r, region):
            """the pixels of `region` out of a full result (whose pixel (0, 0) is image pixel (b, b))"""
            s0, s1 = (slice(t[0] - b, t[1] - b, t[2]) for t in region)
            return {k: (tuple(region) if k == "region" else np.ascontiguousarray(_np(v)[..., s0, s1]) if k not in ("debug_d", "debug_a")
                        else np.ascontiguousarray(v[s0, s1])) for k, v in r.items()}

        for region in (dict(step=2), dict(step=3), dict(ROI=((17, 90, 2), (5, 400, 3))), dict(ROI=((0, 40, 1), (500, 512, 1)))):
            m.ROI = None
            want = widen.valid_region(m, b, **region)
            part = _four(m, b, **region)
            m.ROI = None
            for name, r, f in zip(("grid", "volume", "basins"), part, full):     # (track: the priors are drawn per shape)
                assert tuple(r["region"]) == tuple(want)
                _same(r, cut(f, want), "%s %s" % (region, name))
            assert all(len(range(*t)) >= 1 for t in want)
        assert widen.valid_region(m, b, ROI=((17, 90, 2), (5, 400, 3))) == ((17, 90, 2), (5, 399, 3))
        assert widen.valid_region(m, b, step=3) == ((3, 124, 3), (3, 508, 3))


# ----------------------------------------------------------------------------- 7. special pixels

@pytest.mark.parametrize("bad", ["nan", "+inf", "zero"])
@pytest.mark.parametrize("where", ["sam", "ref"])
def test_special_pixels(hip_ns, bad, where):
    """NaN, +Inf and 0 pixels: the device's non-finite cells are exactly those of extended precision under W', the finite
    ones are within the bound"""
    import regimes
    sam, ref, c = GE.stack("64x72x3")
    b, ms, Nw = 2, c["ms"], c["Nw"]
    cfg = dict(H=c["H"], W=c["W"], K=c["K"], Nw=Nw, ms=ms)
    pos = [p for p in regimes.bad_positions(cfg) if p[1] < c["H"] and p[2] < c["W"]]
    assert len(pos) >= 3
    sam, ref = regimes.bad_pixels(sam, ref, bad, where, pos)
    for kind in (0, 1):
        m = _model(hip_ns, kind, sam, ref, Nw, ms)
        vol = m.cost_volume(with_fit=True, widen=b)
        vol.pop("region")
        with np.errstate(all="ignore"):
            hp = WE.volumes(kind, sam, ref, Nw, b, ms, "sam")
        fin = np.isfinite(hp["cost"].astype(np.float64))
        np.testing.assert_array_equal(np.isfinite(vol["cost"]), fin)
        assert fin.any() and (bad == "zero" or (~fin).any())
        ratio = np.abs(vol["cost"][fin].astype(np.longdouble) - hp["cost"][fin]) / hp["bound"][fin]
        assert np.all(ratio <= 1.0), "kind %d: max |gpu - hp| / bound = %.4f" % (kind, ratio.max())


# ----------------------------------------------------------------------------- 8. repeats, HIP tensors on a side stream

def test_repeats_and_device_arrays_on_a_side_stream(hip_ns):
    import torch
    sam, ref, c = GE.stack("64x72x3")
    b = 2
    for kind in (0, 1):
        m = _model(hip_ns, kind, sam, ref, c["Nw"], c["ms"], subpx=-1)
        host = _four(m, b)
        for name, x, y in zip(("grid", "volume", "basins", "track"), _four(m, b), host):
            _same(x, y, "second call: " + name)
        sh = host[0]["dx"].shape
        rng = np.random.default_rng(5)                               # _four's priors
        pdx, pdy = rng.uniform(-5, 5, sh), rng.uniform(-5, 5, sh)
        dev = torch.device("cuda", m._device)
        stream = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(stream):
            t = m.track(torch.as_tensor(pdx, device=dev), torch.as_tensor(pdy, device=dev), lam=0.02, radius=4.0, widen=b)
            U = 2 * c["ms"] - 1
            _, _, vol = m._grid_cost_volume(None, None, lambda U, N0, N1: {k: torch.full((U, U, N0, N1), -7.0, dtype=torch.float64, device=dev)
                                                                         for k in ("cost", "T") + (("df",) if kind else ())}, b)
        stream.synchronize()
        assert hasattr(t["dx"], "data_ptr")
        _same(t, host[3], "track on device arrays")
        _same(vol, _maps(host[1]), "volume on device arrays")


# ----------------------------------------------------------------------------- 9. the use case

@functools.lru_cache(maxsize=None)
def _use():
    from nativelibs import gpu_test_module
    mod = gpu_test_module("basins")
    sam, ref, known = mod._use_case()
    return mod.USE, sam, ref, known


def test_a_wide_window_finds_the_true_shift_and_coarse_to_fine_keeps_it(hip_ns):
    from umpa_amd import widen
    u, sam, ref, known = _use()
    ty, tx = u["true"]
    Nw, ms = u["Nw"], u["ms"]
    m = _model(hip_ns, 0, sam, ref, Nw, ms, "sam", 0)                 # sub-pixel mode 0: dx, dy are the integer shifts
    plain = m.match(quiet=True, search="grid", widen=0)
    assert "region" not in plain
    np.testing.assert_array_equal(plain["dy"][known], ty)
    np.testing.assert_array_equal(plain["dx"][known], tx - u["period"])   # the alias
    levels = (4, 2, 1, 0)
    sure = {b: WE.use_case_sure(sam, ref, Nw, ms, b, (ty, tx)) for b in levels}
    wide = m.match(quiet=True, search="grid", widen=4)
    assert wide["dx"].shape == sure[4].shape and sure[4].mean() >= 0.95
    np.testing.assert_array_equal(wide["dy"][sure[4]], ty)
    np.testing.assert_array_equal(wide["dx"][sure[4]], tx)
    # coarse to fine: wherever the true shift is a sure basin at every level -- below its eight neighbours by more than the
    # bounds -- the nearest basin to a prior on the true shift is the true shift, level after level, down to b = 0
    last, every = widen.coarse_to_fine(m, levels=levels)
    assert [tuple(r["region"]) for r in every] == [widen.valid_region(m, b) for b in levels] and last is every[-1]
    N0, N1 = m.extent
    chain = np.zeros((N0, N1), bool)
    chain[4:N0 - 4, 4:N1 - 4] = sure[4]                               # the first level: the grid search finds the true shift
    for b in levels[1:]:
        inside = np.zeros((N0, N1), bool)
        inside[b:N0 - b, b:N1 - b] = _sure_basin(sam, ref, Nw, ms, b, (ty, tx))
        chain &= inside
    print("use: %d of %d pixels are sure at every level, %d of them among the %d known" % (chain.sum(), chain.size, (chain & known).sum(), known.sum()))
    assert chain.any() and (chain & known).any()
    np.testing.assert_array_equal(last["dy"][chain], ty)
    np.testing.assert_array_equal(last["dx"][chain], tx)


def _sure_basin(sam, ref, Nw, ms, b, true):
    """the true shift lies below each of its eight neighbours by more than the two bounds (a basin for any fp64 evaluation
    within its bound), over the pixels whose widened window fits"""
    v = WE.volumes(0, sam, ref, Nw, b, ms, "sam") if b else GE.hp_volumes(0, sam, ref, GE.window(Nw), ms, ms + Nw, "sam")
    a, c = true[0] + ms - 1, true[1] + ms - 1
    ok = np.ones(v["cost"].shape[2:], bool)
    for da in (-1, 0, 1):
        for dc in (-1, 0, 1):
            if da or dc:
                ok &= (v["cost"][a + da, c + dc] - v["bound"][a + da, c + dc]) > (v["cost"][a, c] + v["bound"][a, c])
    return ok
