"""
Basin enumeration (umpa_grid_basins, model.basins, umpa_amd.basins), what can be checked without a GPU: the restatement the
GPU tests use (tests/basins_expect.py) against a brute-force loop and against the grid search's expectation, the
admissibility of the GPU tests' inputs, the library's build, the refusals that come before any device work, and the host
logic of the helpers.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import REPO

import basins_expect as BE
import grid_expect as GE
from nativelibs import assert_claimed, build_all as _build, declared, exported, kernel_keys

GRID_LIB = os.path.join(REPO, "umpa_amd", "libumpa_grid.so")
KTEMPL = 24
NAN, INF = float("nan"), float("inf")


# ----------------------------------------------------------------------------- 1. the restatement against the loop

def _hand_made(U, rng):
    """{name: [U, U] cost array} -- one pixel each"""
    base = lambda: 1.0 + rng.random((U, U))
    px = {"random": rng.standard_normal((U, U)), "constant": np.full((U, U), 2.5), "all_nan": np.full((U, U), NAN),
          "all_inf": np.full((U, U), INF), "all_minus_inf": np.full((U, U), -INF)}
    for n, v in (("nan", NAN), ("inf", INF), ("minus_inf", -INF)):
        for share in (0.15, 0.6):
            a = rng.standard_normal((U, U))
            a[rng.random((U, U)) < share] = v
            px["%s_%d" % (n, int(100 * share))] = a
    a = rng.standard_normal((U, U))
    a[rng.random((U, U)) < 0.2] = NAN
    a[rng.random((U, U)) < 0.2] = INF
    a[rng.random((U, U)) < 0.2] = -INF
    px["mixed"] = a
    g = rng.integers(0, 3, U).astype(np.float64)                      # equal values in adjacent rows too
    px["row_constant"] = np.repeat(g[:, None], U, axis=1)             # every cost row is a plateau along sj
    px["column_constant"] = np.repeat(g[None, :], U, axis=0)
    px["few_values"] = rng.integers(0, 3, (U, U)).astype(np.float64)  # plateaus of every shape
    if U >= 3:
        a = base()
        a[0, 0] = a[0, U - 1] = a[U - 1, 0] = a[U - 1, U - 1] = 0.0   # a minimum in each corner, all equal
        px["corners"] = a
        a = base()
        h = U // 2
        a[0, h], a[h, 0], a[h, U - 1], a[U - 1, h] = 0.25, 0.5, 0.5, 0.125   # ... and on each edge
        px["edges"] = a
        a = base()
        a[::2, ::2] = 0.0                                             # equal non-adjacent minima: scan order ranks them
        px["equal_lattice"] = a
        a = base()
        a[::2, ::2] = -rng.integers(0, 4, a[::2, ::2].shape)          # ... with ties among some of them
        px["lattice"] = a
    return px


@pytest.mark.parametrize("U", [1, 3, 5, 9])
def test_restatement_against_the_brute_force_loop(U):
    rng = np.random.default_rng(1000 + U)
    px = _hand_made(U, rng)
    names = sorted(px)
    cost = np.stack([px[n] for n in names], axis=-1).reshape(U, U, 1, len(names))
    T, df = rng.random(cost.shape), rng.random(cost.shape)
    ms = (U + 1) // 2
    for subpx in (-1, 0, 1):
        for k in (1, 4, 8):
            for with_df in (False, True):
                a = BE.restate(cost, T, df if with_df else None, k, subpx)
                b = BE.brute(cost, T, df if with_df else None, k, subpx)
                BE.assert_equal(a, b, "U %d subpx %d k %d" % (U, subpx, k))
    r = BE.restate(cost, T, df, 8, 0)
    at = lambda n: names.index(n)
    count = lambda n: int(r["count"][0, at(n)])
    # what the definition says about these inputs, spelled out
    assert [count(n) for n in ("all_nan", "all_inf")] == [0, 0] and (r["err"][:, 0, at("all_nan")] == -1).all()
    for n in ("constant", "all_minus_inf"):                           # one plateau: its earliest member
        assert count(n) == 1 and tuple(r["shift"][0, :, 0, at(n)]) == (1 - ms, 1 - ms)
    kept = r["err"][:, 0, at("row_constant")] >= 0
    assert kept.any() and (r["shift"][kept, 1, 0, at("row_constant")] == 1 - ms).all()
    kept = r["err"][:, 0, at("column_constant")] >= 0
    assert kept.any() and (r["shift"][kept, 0, 0, at("column_constant")] == 1 - ms).all()
    for n in names:                                                   # ranks: cost ascending, scan order among equals; empty slots are zeros
        c, e, sh = r["cost"][:, 0, at(n)], r["err"][:, 0, at(n)], r["shift"][:, :, 0, at(n)]
        nk = min(count(n), 8)
        assert (e[:nk] >= 0).all() and (e[nk:] == -1).all() and (c[nk:] == 0).all() and (sh[nk:] == 0).all()
        key = [(c[q], sh[q, 0], sh[q, 1]) for q in range(nk)]
        assert key == sorted(key), (n, key)
    if U >= 3:
        assert count("corners") >= 4                                  # (an inner cell far from every corner may be a fifth)
        assert [tuple(s) for s in r["shift"][:4, :, 0, at("corners")]] == [(1 - ms, 1 - ms), (1 - ms, ms - 1), (ms - 1, 1 - ms), (ms - 1, ms - 1)]
        assert U == 3 or [tuple(s) for s in r["shift"][:4, :, 0, at("edges")]] == [(ms - 1, 0), (1 - ms, 0), (0, 1 - ms), (0, ms - 1)]
        assert count("equal_lattice") == ((U + 1) // 2) ** 2
        assert (r["err"][:4, 0, at("corners")] == 0).all()           # on the border: no 4x4 neighbourhood
    if U == 9:
        assert count("equal_lattice") == 25 > BE.MAX_K and count("lattice") > BE.MAX_K   # more basins than are kept
        inner = [(a, b) for a in range(-2, 3, 2) for b in range(-2, 3, 2)]                  # |shift| <= ms - 3: both quadrants fit
        assert all(r["err"][q, 0, at("equal_lattice")] == (1 if tuple(r["shift"][q, :, 0, at("equal_lattice")]) in inner else 0) for q in range(8))


# ----------------------------------------------------------------------------- 2. rank 0 is the grid search's minimum; the inputs

_volumes = {}


def _hp(name, kind):
    """the extended-precision volumes of a stack of grid_expect.STACKS (assign 'sam'), and their fp64 roundings"""
    if (name, kind) not in _volumes:
        sam, ref, c = GE.stack(name)
        v = GE.hp_volumes(kind, sam, ref, GE.window(c["Nw"]), c["ms"], c["ms"] + c["Nw"], "sam")
        r = {k: (np.asarray(v[k], dtype=np.float64) if v.get(k) is not None else None) for k in ("cost", "T", "df")}
        _volumes[(name, kind)] = (sam, ref, c, v, r)
    return _volumes[(name, kind)]


HP = [(n, k) for n in sorted(GE.STACKS) for k in (0, 1)]
HP_IDS = ["%s-%s" % (n, "DF" if k else "NoDF") for n, k in HP]


@pytest.mark.parametrize("name,kind", HP, ids=HP_IDS)
def test_rank_0_is_the_grid_search_and_the_inputs_have_basins(name, kind):
    sam, ref, c, v, r = _hp(name, kind)
    ms, U = c["ms"], 2 * c["ms"] - 1
    count = None
    for subpx in (-1, 0, 1):
        exp, near = GE.expected(kind, sam, ref, GE.window(c["Nw"]), ms, ms + c["Nw"], "sam", subpx, volumes=v)
        b = BE.restate(r["cost"], r["T"], r["df"], 5, subpx)
        keep = ~near
        assert near.mean() <= GE.NEAR_TIE_CAP
        np.testing.assert_array_equal(b["shift"][0, 0][keep], exp["ci"][keep])
        np.testing.assert_array_equal(b["shift"][0, 1][keep], exp["cj"][keep])
        for n in ("err", "dx", "dy", "f", "T") + (("df",) if kind else ()):
            np.testing.assert_array_equal(b[n][0][keep], exp[n][keep], err_msg="%s subpx %d" % (n, subpx))
        count = b["count"]
    # the inputs exercise the feature (conditions on the inputs: the reference side meets them alone)
    print("%s kind %d: pixels with >= 2 basins %.1f %%, with > 4 %.1f %%, at most %d" % (
        name, kind, 100 * (count >= 2).mean(), 100 * (count > 4).mean(), count.max()))
    assert (count >= 1).all() and (count >= 2).mean() >= 0.70 and (count > 4).any()
    # ... and the ranking of the five best basins is decided beyond the fp64 bounds of the costs at every pixel
    basin = BE.is_basin(r["cost"]).reshape(U * U, -1)
    cc = np.where(basin, r["cost"].reshape(U * U, -1), np.inf)
    order = np.argsort(cc, axis=0, kind="stable")[:5]
    cs = np.take_along_axis(cc, order, axis=0)
    bs = np.take_along_axis(np.asarray(v["bound"], dtype=np.float64).reshape(U * U, -1), order, axis=0)
    amb = np.zeros(cs.shape[1], bool)
    with np.errstate(invalid="ignore"):                               # (fewer than five basins: Inf - Inf)
        for q in range(4):
            amb |= np.isfinite(cs[q + 1]) & ((cs[q + 1] - cs[q]) < (bs[q] + bs[q + 1]))
    assert amb.mean() == 0.0, amb.mean()


# ----------------------------------------------------------------------------- 3. the library

def test_grid_library_exports_basins_and_its_kernels_are_claimed():
    g = _build()
    from umpa_amd import _lib
    assert len(g.LIBRARIES) == 8                                      # a fourth consumer in libumpa_grid.so, not a ninth library
    assert "umpa_grid_basins" in declared("umpa_grid.h", "umpa_grid_") and "basins" in _lib.GRID_SYMBOLS
    assert declared("umpa_grid.h", "umpa_grid_") == sorted("umpa_grid_" + s for s in _lib.GRID_SYMBOLS)
    assert "umpa_grid_basins" in exported(GRID_LIB)
    assert sorted(n for n in exported(GRID_LIB) if n.startswith("umpa")) == declared("umpa_grid.h", "umpa_grid_")
    assert hasattr(_lib.grid(), "basins")
    syms = [k for k in kernel_keys(GRID_LIB) if k.split("<", 1)[0] == "grid_basins_kernel"]
    want = ["grid_basins_kernel<1, %d>" % n for n in range(KTEMPL + 1)] + ["grid_basins_kernel<0, 0>"]
    assert sorted(syms) == sorted(want) and len(syms) == 26, sorted(set(syms) ^ set(want))
    assert_claimed(syms, "basins")
    # the main library: no new public symbol
    public = sorted(n for n in exported(g.HIP_LIB) if n.startswith("umpa_hip_"))
    assert public == sorted("umpa_hip_" + s for s in _lib.HIP_SYMBOLS)


E_ARG = -1
NULL_TEXT = "grid: basins: null argument"
K_TEXT = "grid: basins keeps 1 to 8 basins per pixel, not %d"
FLAGS_TEXT = "grid: basins takes UMPA_HIP_F_DEVICE_IO, UMPA_HIP_F_USE_STAGED and no other flag"


def test_c_abi_refusals_come_before_any_device_work():
    """No device, no model: a pointer that is never followed stands for one.  Every refusal has its code and its full text;
    of two faults the first in the header's order (null pointers, K, flags) is the one reported."""
    _build()
    from umpa_amd import _lib
    g = _lib.grid()
    fake = ctypes.create_string_buffer(64)
    bufs = [np.zeros(8) for _ in range(6)] + [np.zeros(8, np.int32) for _ in range(4)]

    def call(model=ctypes.addressof(fake), K=4, flags=0, drop=None):
        ptrs = [None if q == drop else a.ctypes.data for q, a in enumerate(bufs)]
        return g.basins(model, 0, 1, 1, 0, 1, 1, K, *ptrs, flags, None), g.error()

    assert call(model=None) == (E_ARG, NULL_TEXT)
    for q in (0, 1, 2, 3, 4, 6, 7, 8, 9):                             # every array but df (index 5) is needed
        assert call(drop=q) == (E_ARG, NULL_TEXT), q
    for K in (0, -1, 9, 1 << 20):
        assert call(K=K) == (E_ARG, K_TEXT % K), K
    for flags in (_lib.F_FORCE_DIRECT, _lib.F_FORCE_TILED, _lib.F_PLANAR, _lib.F_REUSE_REF_MAPS, _lib.F_ASYNC, _lib.F_FORCE_PLAIN_DIRECT,
                  _lib.F_DEVICE_IO | _lib.F_PLANAR, _lib.F_USE_STAGED | _lib.F_ASYNC, 256):
        assert call(flags=flags) == (E_ARG, FLAGS_TEXT), flags
    # double refusals
    assert call(model=None, K=0) == (E_ARG, NULL_TEXT)
    assert call(drop=9, flags=_lib.F_PLANAR) == (E_ARG, NULL_TEXT)
    assert call(K=9, flags=_lib.F_PLANAR) == (E_ARG, K_TEXT % 9)
    assert all((a == 0).all() for a in bufs)


# ----------------------------------------------------------------------------- 4. the Python layer

class _HipLib:
    is_hip = True


def _stub(cls, **kw):
    """a model object that has what the checks in front of the native call read, and no device"""
    from umpa_amd import model
    m = object.__new__(getattr(model, cls))
    m._lib, m._mask, m._force = _HipLib(), None, 0
    m._pos_list, m._shape_list = [(0, 0)] * 3, [(40, 48)] * 3
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def test_python_refusals():
    from umpa_amd import _lib, model
    tail = " (grid search / cost volume): "
    for cls in ("UMPAModelDF", "UMPAModelNoDF"):
        for k in (0, 9, -1, 2.0, 2.5, "4", None, True):
            with pytest.raises(ValueError) as e:
                _stub(cls).basins(k=k)
            assert str(e.value) == "basins: k must be an integer from 1 to 8, not %r" % (k,)
        cases = [(dict(_mask=np.ones((3, 40, 48))), "masked models are not supported (their table holds finished costs)"),
                 (dict(_pos_list=[(0, 0), (2, 1), (1, 3)]), "frames at different positions (pos_list) or of different shapes are not supported"),
                 (dict(_shape_list=[(40, 48), (40, 48), (40, 50)]), "frames at different positions (pos_list) or of different shapes are not supported"),
                 (dict(_force=_lib.F_FORCE_DIRECT), "the model is forced onto the direct kernel")]
        for kw, why in cases:
            with pytest.raises(RuntimeError) as e:
                _stub(cls, **kw).basins()
            assert str(e.value) == "basins" + tail + why
            with pytest.raises(RuntimeError) as e:                    # the model's refusal comes before k's
                _stub(cls, **kw).basins(k=0)
            assert str(e.value) == "basins" + tail + why
    assert not hasattr(model.UMPAModelDFKernel, "basins")
    with pytest.raises(RuntimeError) as e:
        _stub("UMPAModelDFKernel")._grid_check("basins")
    assert str(e.value) == "basins" + tail + "the kernel dark-field model has no shift table"


def _hand_dict():
    """k = 3, 2 x 2 pixels: (0,0) three basins, (0,1) two, (1,0) one, (1,1) none"""
    count = np.array([[5, 2], [1, 0]], np.int32)
    err = np.array([[[1, 1], [0, -1]], [[0, 1], [-1, -1]], [[1, -1], [-1, -1]]], np.int32)
    live = err >= 0
    shift = np.zeros((3, 2, 2, 2), np.int32)
    shift[:, 0][live] = [1, -2, 3, 0, 2, -3]                          # rank-major: (r0: px00, px01, px10), (r1: px00, px01), (r2: px00)
    shift[:, 1][live] = [0, 1, -3, -2, 2, 3]
    b = {"count": count, "err": err, "shift": shift}
    for q, n in enumerate(("dx", "dy", "f", "T", "df", "cost")):
        b[n] = np.where(live, 10.0 * (q + 1) + np.arange(12).reshape(3, 2, 2), 0.0)
    b["cost"] = np.where(live, np.array([[[1.0, 2.0], [3.0, 0.0]], [[1.5, 2.0], [0.0, 0.0]], [[4.0, 0.0], [0.0, 0.0]]]), 0.0)
    return b


def test_helpers_on_a_hand_made_dictionary():
    import umpa_amd
    from umpa_amd import basins as B
    assert umpa_amd.basins is B and "basins" in umpa_amd.__all__ and B.__all__ == ["select", "nearest", "start_shifts", "ambiguity"]
    b = _hand_dict()
    # select: a scalar rank, a rank per pixel, empty slots
    s0 = B.select(b, 0)
    for n in ("dx", "dy", "f", "T", "df", "cost"):
        np.testing.assert_array_equal(s0[n], b[n][0])
    np.testing.assert_array_equal(s0["err"], [[1, 1], [0, 0]])
    assert s0["err"].dtype == np.int32
    np.testing.assert_array_equal(s0["shift"], b["shift"][0])
    idx = np.array([[2, 1], [0, 2]])
    s = B.select(b, idx)
    np.testing.assert_array_equal(s["dx"], [[b["dx"][2, 0, 0], b["dx"][1, 0, 1]], [b["dx"][0, 1, 0], 0.0]])
    np.testing.assert_array_equal(s["err"], [[1, 1], [0, 0]])
    np.testing.assert_array_equal(s["shift"][:, 0, 0], b["shift"][2, :, 0, 0])
    np.testing.assert_array_equal(s["shift"][:, 1, 1], [0, 0])
    for bad in (3, -1, np.full((2, 2), 3), np.zeros((2, 3), int), np.zeros(4, int), 1.0):
        with pytest.raises(ValueError):
            B.select(b, bad)
    # nearest: by the integer shift, (prior_dy rows, prior_dx columns); the lower rank among equally close; empty slots never
    near = B.nearest(b, np.array([[3.1, 0.9], [100.0, 7.0]]), np.array([[-2.8, -2.1], [-100.0, 7.0]]))
    np.testing.assert_array_equal(near, [[2, 0], [0, 0]])
    np.testing.assert_array_equal(B.nearest(b, -2.0, 0.0), [[1, 0], [0, 0]])      # scalars; px (0,0): (0,-2) at rank 1
    np.testing.assert_array_equal(B.nearest(b, NAN, 0.0), np.zeros((2, 2), int))
    tie = {"err": np.zeros((2, 1, 1), np.int32), "shift": np.array([[[[1]], [[0]]], [[[-1]], [[0]]]], np.int32)}
    assert B.nearest(tie, 0.0, 0.0)[0, 0] == 0                        # (1, 0) and (-1, 0) are equally far from (0, 0)
    # start_shifts: row shift first, float64, (0, 0) for an empty slot
    d0, d1 = B.start_shifts(b, near)
    assert d0.dtype == d1.dtype == np.float64
    np.testing.assert_array_equal(d0, [[-3.0, -2.0], [3.0, 0.0]])
    np.testing.assert_array_equal(d1, [[3.0, 1.0], [-3.0, 0.0]])
    # ambiguity
    np.testing.assert_array_equal(B.ambiguity(b), [[0.5, 0.0], [INF, INF]])
    with pytest.raises(ValueError):
        B.ambiguity({k: v[:1] if k != "count" else v for k, v in b.items()})
