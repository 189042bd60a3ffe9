"""
Tracked search (umpa_grid_track, model.track, umpa_amd.track), what can be checked without a GPU: the restatement the GPU
tests use (tests/track_expect.py) against a brute-force loop and against the host route it replaces (basins + nearest +
select), the library's build, the refusals that come before any device work, the host logic of prior_from / Tracker, and
the CPU-decided pixel sets of the use case.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import REPO

import basins_expect as BE
import grid_expect as GE
import track_expect as TE
from nativelibs import assert_claimed, build_all as _build, declared, exported, kernel_keys, tool

GRID_LIB = os.path.join(REPO, "umpa_amd", "libumpa_grid.so")
KTEMPL = 24
NAN, INF = float("nan"), float("inf")


# ----------------------------------------------------------------------------- 1. the restatement against the loop

_volumes = {}


def _hp(name, kind):
    """the extended-precision volumes of a stack of grid_expect.STACKS (assign 'sam') rounded to fp64"""
    if (name, kind) not in _volumes:
        sam, ref, c = GE.stack(name)
        v = GE.hp_volumes(kind, sam, ref, GE.window(c["Nw"]), c["ms"], c["ms"] + c["Nw"], "sam")
        _volumes[(name, kind)] = (c, {k: (np.asarray(v[k], dtype=np.float64) if v.get(k) is not None else None) for k in ("cost", "T", "df")})
    return _volumes[(name, kind)]


def _priors(ms, N0, N1, seed):
    """{name: (prior_i, prior_j)}: a constant, a random field within +-(ms + 1), a field with NaN and +-Inf entries"""
    rng = np.random.default_rng(seed)
    field = lambda: rng.uniform(-(ms + 1), ms + 1, (N0, N1))
    si, sj = field(), field()
    for a in (si, sj):
        w = rng.random((N0, N1))
        a[w < 0.10] = NAN
        a[(w >= 0.10) & (w < 0.17)] = INF
        a[(w >= 0.17) & (w < 0.24)] = -INF
    pr = {"constant": (0.75, -1.5), "random": (field(), field()), "special": (si, sj)}
    assert all(np.abs(a).max() <= ms + 1 and np.abs(a).max() > ms - 1 for a in pr["random"])
    assert all(np.isnan(a).any() and (a == INF).any() and (a == -INF).any() and np.isfinite(a).any() for a in pr["special"])
    return pr


def _mid_lam(r):
    """a penalty weight on the scale of the volume: the median cost gap between the two best basins per unit of d2"""
    b = BE.restate(r["cost"], r["T"], r["df"], 2, 0)
    two = b["count"] >= 2
    assert two.mean() > 0.5
    return float(np.median((b["cost"][1] - b["cost"][0])[two]) / 4.0)


HP = [(n, k) for n in sorted(GE.STACKS) for k in (0, 1)]
HP_IDS = ["%s-%s" % (n, "DF" if k else "NoDF") for n, k in HP]


@pytest.mark.parametrize("name,kind", HP, ids=HP_IDS)
def test_restatement_against_the_brute_force_loop(name, kind):
    c, full = _hp(name, kind)
    ms = c["ms"]
    # the loop costs a millisecond per pixel and shift row: every 6th row and 8th column of the maps, 72 to 156 pixels
    r = {k: (np.ascontiguousarray(v[:, :, 3::6, 2::8]) if v is not None else None) for k, v in full.items()}
    N0, N1 = r["cost"].shape[2:]
    assert N0 * N1 >= 60
    pr = _priors(ms, N0, N1, 700 + ms + kind)
    mid = _mid_lam(r)
    modes = {"nearest": (TE.NEAREST, 0.0), "lam0": (TE.PENALTY, 0.0), "mid": (TE.PENALTY, mid), "huge": (TE.PENALTY, 1e300)}
    radii = {"none": None, "zero": 0.0, "1.5": 1.5, "tight": 0.7}
    seen = {}
    for pn, (pi, pj) in pr.items():
        for mn, (mode, lam) in modes.items():
            for rn, radius in radii.items():
                subs = (-1, 0, 1) if (pn, mn, rn) in (("random", "nearest", "none"), ("random", "mid", "1.5"), ("special", "mid", "none")) else (0,)
                for subpx in subs:
                    a = TE.restate(r["cost"], r["T"], r["df"], pi, pj, mode, lam, radius, subpx)
                    b = TE.brute(r["cost"], r["T"], r["df"], pi, pj, mode, lam, radius, subpx)
                    TE.assert_equal(a, b, "%s %s radius %s subpx %d" % (pn, mn, rn, subpx))
                    assert sorted(a) == sorted(["dx", "dy", "f", "T", "cost", "cost0", "shift", "err", "count", "found"] + (["df"] if kind else []))
                seen[(pn, mn, rn)] = a
    # what the definition says about these inputs, spelled out (conditions on the inputs and on the restatement)
    count = seen[("random", "nearest", "none")]["count"]
    assert (count >= 1).all() and (count >= 2).mean() > 0.5
    for pn in pr:
        for mn in modes:
            free, zero, tight = (seen[(pn, mn, rn)] for rn in ("none", "zero", "tight"))
            np.testing.assert_array_equal(free["found"], count)      # no limit: every basin is admissible
            np.testing.assert_array_equal(free["count"], count)
            assert (tight["found"] <= seen[(pn, mn, "1.5")]["found"]).all() and (seen[(pn, mn, "1.5")]["found"] <= count).all()
            for d in (free, zero, tight):
                empty = d["found"] == 0
                assert (d["err"][empty] == 0).all() and all((d[n][empty] == 0).all() for n in ("dx", "dy", "f", "T", "cost")) and (d["shift"][:, empty] == 0).all()
                assert (d["cost"] >= d["cost0"])[~empty].all() and (d["cost0"][count > 0] == free["cost0"][count > 0]).all()
    # the tight radius leaves some pixels without an admissible basin, and others with one
    t = seen[("random", "nearest", "tight")]["found"]
    assert (t == 0).any() and (t > 0).any()
    # radius 0 admits a basin only where the prior is an integer shift, or blind: the special field's NaN pixels
    z = seen[("special", "nearest", "zero")]["found"]
    blind = np.isnan(pr["special"][0]) | np.isnan(pr["special"][1])
    np.testing.assert_array_equal(z[blind], count[blind])
    assert (z[~blind] == 0).all() and (seen[("random", "mid", "zero")]["found"] == 0).all()
    # the mid weight is between the extremes: it differs from lam = 0 and from the nearest basin somewhere, and a huge
    # weight picks a basin as near as the nearest mode's
    sh = lambda d: d["shift"].astype(np.float64)
    m, l0, nr, hg = (seen[("random", mn, "none")] for mn in ("mid", "lam0", "nearest", "huge"))
    assert (sh(m) != sh(l0)).any(axis=0).any() and (sh(m) != sh(nr)).any(axis=0).any()
    d2 = lambda d: (sh(d)[0] - pr["random"][0]) ** 2 + (sh(d)[1] - pr["random"][1]) ** 2
    np.testing.assert_array_equal(d2(hg), d2(nr))
    assert (d2(nr) <= d2(l0)).all() and (d2(nr) < d2(l0)).any()
    assert (m["cost"] > m["cost0"]).any() and (l0["cost"] == l0["cost0"]).all()


# ----------------------------------------------------------------------------- 2. equivalences in numpy

def _ms17_volume():
    """an ms = 17 volume (U = 33) of 40 pixels of the stack tests/test_hip_track.py searches at ms 17"""
    from umpa_amd.synth import make_stack
    ms, Nw = 17, 2
    sam, ref, _ = make_stack(58, 108, 3, 4, df=True, seed=300 + ms)
    xi, xj = np.meshgrid(np.arange(1, 20, 4), np.arange(2, 70, 9), indexing="ij")
    v = GE.hp_volumes(0, sam, ref, GE.window(Nw), ms, ms + Nw, "sam", pixels=(xi, xj))
    return {k: np.asarray(v[k], dtype=np.float64) for k in ("cost", "T")}


def _same_as_select(t, b, pdx, pdy, where, what):
    from umpa_amd import basins as B
    s = B.select(b, B.nearest(b, pdx, pdy))
    for n in ("dx", "dy", "f", "T", "df", "cost", "err", "shift"):
        if n in s:
            np.testing.assert_array_equal(t[n][..., where], s[n][..., where], err_msg="%s %s" % (what, n))


def test_nearest_mode_is_basins_nearest_select_where_all_basins_are_kept():
    vols = [("%s kind %d" % (n, k), _hp(n, k)[1]) for n, k in HP] + [("ms 17", dict(_ms17_volume(), df=None))]
    for what, r in vols:
        U, _, N0, N1 = r["cost"].shape
        ms = (U + 1) // 2
        rng = np.random.default_rng(N0 * U)
        pi, pj = rng.uniform(-(ms + 1), ms + 1, (N0, N1)), rng.uniform(-(ms + 1), ms + 1, (N0, N1))
        pi[::5, ::3] = NAN
        pj[1::5, 1::3] = INF
        for subpx in (0, -1):
            b = BE.restate(r["cost"], r["T"], r["df"], 8, subpx)
            t = TE.restate(r["cost"], r["T"], r["df"], pi, pj, TE.NEAREST, 0.0, None, subpx)
            all_kept = b["count"] <= 8
            print("%s: %.1f %% of the pixels have at most 8 basins, at most %d" % (what, 100 * all_kept.mean(), b["count"].max()))
            assert what == "ms 17" or all_kept.mean() >= 0.90           # (at ms 17 every pixel of the sample has more than 8)
            _same_as_select(t, b, pj, pi, all_kept, what)
            np.testing.assert_array_equal(t["count"], b["count"])
            np.testing.assert_array_equal(t["cost0"], np.where(b["count"] > 0, b["cost"][0], 0.0))
        if what == "ms 17":
            assert (b["count"] > 8).any()


@pytest.mark.parametrize("name,kind", HP, ids=HP_IDS)
def test_lam_0_and_a_nan_prior_are_rank_0(name, kind):
    c, r = _hp(name, kind)
    ms = c["ms"]
    N0, N1 = r["cost"].shape[2:]
    rng = np.random.default_rng(5)
    pi, pj = rng.uniform(-(ms + 1), ms + 1, (N0, N1)), rng.uniform(-(ms + 1), ms + 1, (N0, N1))
    b = BE.restate(r["cost"], r["T"], r["df"], 1, 1)
    every = np.ones((N0, N1), bool)
    for what, args in (("lam 0", (pi, pj, TE.PENALTY, 0.0, None)), ("lam 0, radius 40", (pi, pj, TE.PENALTY, 0.0, 40.0)),
                       ("NaN prior, nearest", (NAN, pj, TE.NEAREST, 0.0, None)), ("NaN prior, penalty", (pi, NAN, TE.PENALTY, 3.0, 0.0))):
        t = TE.restate(r["cost"], r["T"], r["df"], *args, 1)
        _same_as_select(t, b, 0.0, 0.0, every, what)               # k = 1: select(nearest) is rank 0
        np.testing.assert_array_equal(t["cost"], t["cost0"])


# ----------------------------------------------------------------------------- 3. the library

def test_grid_library_exports_track_and_its_kernels_are_claimed():
    g = _build()
    from umpa_amd import _lib
    assert len(g.LIBRARIES) == 8                                      # a fifth consumer in libumpa_grid.so, not a ninth library
    assert "umpa_grid_track" in declared("umpa_grid.h", "umpa_grid_") and "track" in _lib.GRID_SYMBOLS
    assert declared("umpa_grid.h", "umpa_grid_") == sorted("umpa_grid_" + s for s in _lib.GRID_SYMBOLS)
    assert "umpa_grid_track" in exported(GRID_LIB)
    assert sorted(n for n in exported(GRID_LIB) if n.startswith("umpa")) == declared("umpa_grid.h", "umpa_grid_")
    assert hasattr(_lib.grid(), "track")
    assert (_lib.GRID_TRACK_NEAREST, _lib.GRID_TRACK_PENALTY) == (0, 1)
    hdr = open(os.path.join(REPO, "include", "umpa_grid.h")).read()
    assert "#define UMPA_GRID_TRACK_NEAREST 0" in hdr and "#define UMPA_GRID_TRACK_PENALTY 1" in hdr
    syms = [k for k in kernel_keys(GRID_LIB) if k.split("<", 1)[0] == "grid_track_kernel"]
    want = ["grid_track_kernel<1, %d>" % n for n in range(KTEMPL + 1)] + ["grid_track_kernel<0, 0>"]
    assert sorted(syms) == sorted(want) and len(syms) == 26, sorted(set(syms) ^ set(want))
    assert_claimed(syms, "track")
    # tools/kernel_coverage.py lists the family
    assert sum("grid_track_kernel<" in s for s in tool("kernel_coverage").kernel_symbols(GRID_LIB)) == 26
    # the main library: no new public symbol
    public = sorted(n for n in exported(g.HIP_LIB) if n.startswith("umpa_hip_"))
    assert public == sorted("umpa_hip_" + s for s in _lib.HIP_SYMBOLS)


E_ARG = -1
NULL_TEXT = "grid: track: null argument"
MODE_TEXT = "grid: track: mode must be UMPA_GRID_TRACK_NEAREST (0) or UMPA_GRID_TRACK_PENALTY (1), not %d"
LAM_TEXT = "grid: track: lam must be finite and not negative"
RADIUS_TEXT = "grid: track: radius must not be NaN"
FLAGS_TEXT = "grid: track takes UMPA_HIP_F_DEVICE_IO, UMPA_HIP_F_USE_STAGED and no other flag"


def test_c_abi_refusals_come_before_any_device_work():
    """No device, no model: a pointer that is never followed stands for one.  Every refusal has its code and its full text;
    of two faults the first in the header's order (null pointers, mode, lam, radius, flags) is the one reported."""
    _build()
    from umpa_amd import _lib
    g = _lib.grid()
    fake = ctypes.create_string_buffer(64)
    # the arrays in the order of the arguments: prior_i, prior_j | f T dx dy cost df | si sj err | cost0 | count found
    bufs = [np.zeros(8) for _ in range(8)] + [np.zeros(8, np.int32) for _ in range(3)] + [np.zeros(8)] + [np.zeros(8, np.int32) for _ in range(2)]

    def call(model=ctypes.addressof(fake), mode=0, lam=0.0, radius=-1.0, flags=0, drop=None):
        ptrs = [None if q == drop else a.ctypes.data for q, a in enumerate(bufs)]
        return g.track(model, 0, 1, 1, 0, 1, 1, ptrs[0], ptrs[1], mode, lam, radius, *ptrs[2:], flags, None), g.error()

    assert call(model=None) == (E_ARG, NULL_TEXT)
    for q in range(14):
        if q != 7:                                                    # every array but df is needed
            assert call(drop=q) == (E_ARG, NULL_TEXT), q
    for mode in (-1, 2, 1 << 20):
        assert call(mode=mode) == (E_ARG, MODE_TEXT % mode), mode
    for lam in (-1.0, -1e-300, INF, -INF, NAN):
        assert call(mode=1, lam=lam) == (E_ARG, LAM_TEXT), lam
    assert call(radius=NAN) == (E_ARG, RADIUS_TEXT) and call(mode=1, lam=1.0, radius=NAN) == (E_ARG, RADIUS_TEXT)
    for flags in (_lib.F_FORCE_DIRECT, _lib.F_FORCE_TILED, _lib.F_PLANAR, _lib.F_REUSE_REF_MAPS, _lib.F_ASYNC, _lib.F_FORCE_PLAIN_DIRECT,
                  _lib.F_DEVICE_IO | _lib.F_PLANAR, _lib.F_USE_STAGED | _lib.F_ASYNC, 256):
        assert call(flags=flags) == (E_ARG, FLAGS_TEXT), flags
        assert call(mode=0, lam=NAN, radius=INF, flags=flags) == (E_ARG, FLAGS_TEXT), flags   # nearest mode ignores lam; an infinite radius is a number
    # double refusals: the header's order
    assert call(model=None, mode=7) == (E_ARG, NULL_TEXT)
    assert call(drop=13, flags=_lib.F_PLANAR) == (E_ARG, NULL_TEXT)
    assert call(mode=2, lam=-1.0) == (E_ARG, MODE_TEXT % 2)
    assert call(mode=1, lam=-1.0, radius=NAN) == (E_ARG, LAM_TEXT)
    assert call(mode=1, lam=NAN, flags=_lib.F_PLANAR) == (E_ARG, LAM_TEXT)
    assert call(radius=NAN, flags=_lib.F_PLANAR) == (E_ARG, RADIUS_TEXT)
    assert all((a == 0).all() for a in bufs)


# ----------------------------------------------------------------------------- 4. the Python layer

class _HipLib:
    is_hip = True


def _stub(cls, **kw):
    """a model object that has what the checks in front of the native call read, and no device: 28 x 36 pixels"""
    from umpa_amd import model
    m = object.__new__(getattr(model, cls))
    m._lib, m._mask, m._force, m._device = _HipLib(), None, 0, 0
    m._pos_list, m._shape_list, m._padding = [(0, 0)] * 3, [(40, 48)] * 3, 6
    m._ROI = ((0, 28, 1), (0, 36, 1))
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def test_python_refusals():
    import torch
    from umpa_amd import _lib, model
    tail = " (grid search / cost volume): "
    for cls in ("UMPAModelDF", "UMPAModelNoDF"):
        cases = [(dict(_mask=np.ones((3, 40, 48))), "masked models are not supported (their table holds finished costs)"),
                 (dict(_pos_list=[(0, 0), (2, 1), (1, 3)]), "frames at different positions (pos_list) or of different shapes are not supported"),
                 (dict(_shape_list=[(40, 48), (40, 48), (40, 50)]), "frames at different positions (pos_list) or of different shapes are not supported"),
                 (dict(_force=_lib.F_FORCE_DIRECT), "the model is forced onto the direct kernel")]
        for kw, why in cases:
            for args in ((0.0, 0.0), (0.0, 0.0, -1.0), (np.zeros((2, 2)), 0.0)):   # the model's refusal comes before any other
                with pytest.raises(RuntimeError) as e:
                    _stub(cls, **kw).track(*args)
                assert str(e.value) == "track" + tail + why
        for lam in (-1.0, -1e-300, INF, NAN, "1", True, [1.0], 1j):
            with pytest.raises(ValueError) as e:
                _stub(cls).track(0.0, 0.0, lam=lam)
            assert str(e.value) == "track: lam must be None (the nearest basin) or a finite number >= 0, not %r" % (lam,)
        for radius in (-1.0, NAN, "2", False, (1.0,)):
            with pytest.raises(ValueError) as e:
                _stub(cls).track(0.0, 0.0, radius=radius)
            assert str(e.value) == "track: radius must be None (no limit) or a number >= 0, not %r" % (radius,)
            with pytest.raises(ValueError, match="track: lam must be None"):   # lam's refusal comes first
                _stub(cls).track(0.0, 0.0, lam=-2.0, radius=radius)
        # prior shapes, against the region asked for
        for shape, region in (((28, 35), {}), ((36, 28), {}), ((28,), {}), ((1, 28, 36), {}), ((28, 36), dict(step=2)), ((14, 18), dict(ROI=((0, 28, 2), (0, 30, 2))))):
            want = (14, 15) if "ROI" in region else (14, 18) if region else (28, 36)
            for args in ((np.zeros(shape), 0.0), (0.0, np.zeros(shape)), (np.zeros(want), np.zeros(shape))):
                with pytest.raises(ValueError) as e:
                    _stub(cls).track(*args, **region)
                assert str(e.value) == "track: a prior must be a scalar or of shape %s, not %s" % (want, shape)
        with pytest.raises(ValueError) as e:
            _stub(cls).track(np.zeros((28, 36), dtype=complex), 0.0)
        assert str(e.value) == "track: a prior must be of a real number type, not complex128"
        # sides: a tensor beside a numpy array; a tensor that is not a float64 HIP tensor on the model's device
        t = torch.zeros((28, 36), dtype=torch.float64)
        for args in ((t, np.zeros((28, 36))), (np.zeros((28, 36)), t)):
            with pytest.raises(ValueError) as e:
                _stub(cls).track(*args)
            assert str(e.value) == "track: the priors must be both numpy arrays (or scalars) or both HIP tensors"
        for args in ((t, t), (t, 1.0), (t.float(), t.float())):
            with pytest.raises(ValueError) as e:
                _stub(cls).track(*args)
            assert str(e.value) == "track: a device prior must be a float64 HIP tensor on the model's device"
    assert not hasattr(model.UMPAModelDFKernel, "track")
    with pytest.raises(RuntimeError) as e:
        _stub("UMPAModelDFKernel")._grid_check("track")
    assert str(e.value) == "track" + tail + "the kernel dark-field model has no shift table"


def test_prior_from():
    import torch
    import umpa_amd
    from umpa_amd import track as T
    assert umpa_amd.track is T and T.__all__ == ["Tracker", "prior_from"]
    assert umpa_amd.Tracker is T.Tracker and umpa_amd.prior_from is T.prior_from
    assert all(n in umpa_amd.__all__ for n in ("track", "Tracker", "prior_from"))
    res = {"dx": np.array([[1.5, NAN, 2.0], [INF, -1.0, 0.0]]), "dy": np.array([[0.5, 1.0, -INF], [1.0, 2.0, 0.0]]),
           "err": np.array([[1, 1, 1], [1, 0, 1]], np.int32), "f": np.zeros((2, 3))}
    want_dx, want_dy = np.array([[1.5, NAN, NAN], [NAN, NAN, 0.0]]), np.array([[0.5, NAN, NAN], [NAN, NAN, 0.0]])
    dx, dy = T.prior_from(res)
    np.testing.assert_array_equal(dx, want_dx)
    np.testing.assert_array_equal(dy, want_dy)
    assert dx.dtype == dy.dtype == np.float64
    tdx, tdy = T.prior_from({k: torch.from_numpy(v) for k, v in res.items()})
    assert isinstance(tdx, torch.Tensor) and tdx.dtype == tdy.dtype == torch.float64
    np.testing.assert_array_equal(tdx.numpy(), want_dx)
    np.testing.assert_array_equal(tdy.numpy(), want_dy)


class _FakeModel:
    """what Tracker touches of a model; its 'device' is the host, its results come from a list"""
    _device = "cpu"
    sh = (2, 3)

    def __init__(self, results):
        self.results, self.calls, self.staged = list(results), [], []

    def stage_sample(self, raw_frames, dark=None, flat=None):
        self.staged.append((raw_frames, dark, flat))

    def track(self, prior_dx, prior_dy, lam=None, radius=None):
        assert len(self.staged) == len(self.calls) + 1               # the stack was staged first
        self.calls.append((prior_dx, prior_dy, lam, radius))
        return self.results[len(self.calls) - 1]


def test_tracker_on_a_fake_model():
    import torch
    from umpa_amd import track as T
    rng = np.random.default_rng(3)

    def result(bad):
        err = np.ones((2, 3), np.int32)
        err[bad] = 0
        return {"dx": torch.from_numpy(rng.standard_normal((2, 3))), "dy": torch.from_numpy(rng.standard_normal((2, 3))), "err": torch.from_numpy(err)}
    results = [result((0, 1)), result((1, 2)), result((0, 0)), result((1, 1))]
    m = _FakeModel(results)
    t = T.Tracker(m, lam=0.25, radius=3.0)
    assert t.prior is None
    frames = [object() for _ in results]
    for n in (0, 1, 2):
        assert t.step(frames[n], dark="d%d" % n, flat="f%d" % n) is results[n]
        assert m.staged[n] == (frames[n], "d%d" % n, "f%d" % n)
        pdx, pdy, lam, radius = m.calls[n]
        assert (lam, radius) == (0.25, 3.0)
        assert isinstance(pdx, torch.Tensor) and pdx.dtype == pdy.dtype == torch.float64 and tuple(pdx.shape) == tuple(pdy.shape) == (2, 3)
        if n == 0:
            assert torch.isnan(pdx).all() and torch.isnan(pdy).all()   # the first step: the grid search
        else:
            ok = results[n - 1]["err"].numpy() == 1
            np.testing.assert_array_equal(pdx.numpy(), np.where(ok, results[n - 1]["dx"].numpy(), NAN))
            np.testing.assert_array_equal(pdy.numpy(), np.where(ok, results[n - 1]["dy"].numpy(), NAN))
            assert (~ok).sum() == 1
        assert t.prior is not None
    t.reset()
    assert t.prior is None
    t.step(frames[3])
    assert torch.isnan(m.calls[3][0]).all() and torch.isnan(m.calls[3][1]).all() and m.staged[3] == (frames[3], None, None)
    with pytest.raises(RuntimeError, match=r"Tracker needs a model with track\(\)"):
        T.Tracker(object())


# ----------------------------------------------------------------------------- 5. the use case's sets

def test_the_use_case_sets_are_decided_beyond_the_bounds():
    u = TE.use_case()
    known, sure = u["known"], u["sure"]
    period = u["use"]["period"]
    assert known.sum() >= 20 and (u["gap"] > 0).all()
    assert u["lam"] == 2 * u["gap"].max() / period ** 2 or abs(u["lam"] - 2 * u["gap"].max() / period ** 2) <= 1e-15 * u["lam"]
    print("use: lam %.3e; the penalty choice is the true shift beyond the bounds at %d of %d pixels, %d of the %d known ones" % (
        u["lam"], sure.sum(), sure.size, (sure & known).sum(), known.sum()))
    assert sure.sum() >= 20 and (sure & known).sum() >= 20
    # the noise-free sample of the same reference: the true shift is the global minimum beyond the bounds at every pixel
    assert u["clean"].all(), (~u["clean"]).sum()
    assert u["sam0"].shape == u["sam"].shape and not np.array_equal(u["sam0"], u["sam"])
