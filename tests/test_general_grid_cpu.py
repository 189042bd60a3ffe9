"""
The grid consumers on the general table (model.general_grid, umpa_grid_set_general), what can be checked without a GPU: the
library exports the switch and holds the general_table_kernel instantiations, each claimed by a GPU test; the switch in Python
is off by default, leaves every refusal text as it was and lifts the refusals it is there to lift; the inputs of the GPU tests
(tests/general_expect.py) meet the conditions the expectations rest on, and the expected side agrees with the CPU oracle.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import REPO

import general_expect as G
import grid_expect as GE
from nativelibs import assert_claimed, build_all as _build, declared, exported, kernel_keys

GRID_LIB = os.path.join(REPO, "umpa_amd", "libumpa_grid.so")
FAMILY = "general_table_kernel"
WANT = ["%s<%d, %s>" % (FAMILY, kind, mask) for kind in (0, 1) for mask in ("false", "true")]
TEXTS = {
    "mask": "masked models are not supported (their table holds finished costs)",
    "pos": "frames at different positions (pos_list) or of different shapes are not supported",
    "force": "the model is forced onto the direct kernel",
    "dfkernel": "the kernel dark-field model has no shift table",
}
FINISHED = "a finished cost is not linear in the windowed sums, so a box average of costs is not the cost under a wider window"


# ----------------------------------------------------------------------------- 1. the library

def test_set_general_is_declared_exported_and_refuses_a_null_model():
    g = _build()
    from umpa_amd import _lib
    assert "umpa_grid_set_general" in declared("umpa_grid.h", "umpa_grid_")
    assert "set_general" in _lib.GRID_SYMBOLS and _lib._GRID_ABI["set_general"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
    assert declared("umpa_grid.h", "umpa_grid_") == sorted("umpa_grid_" + s for s in _lib.GRID_SYMBOLS)
    assert sorted(n for n in exported(GRID_LIB) if n.startswith("umpa")) == declared("umpa_grid.h", "umpa_grid_")
    lib = _lib.grid()
    for on in (0, 1, 3):
        assert lib.set_general(None, on) == -1                        # UMPA_HIP_E_ARG, before anything touches a device
        assert lib.error() == "grid: set_general: null model"
    # the main library: the hook, no new public symbol; what the satellite needs of it is not in the public header
    names = exported(g.HIP_LIB)
    assert "umpa_hipx_set_general_consumer" in names
    public = sorted(n for n in names if n.startswith("umpa_hip_"))
    assert public == sorted("umpa_hip_" + s for s in _lib.HIP_SYMBOLS)
    hdr = open(os.path.join(REPO, "include", "umpa_hip.h")).read()
    assert "umpa_hipx" not in hdr and "general_consumer" not in hdr


def test_the_general_table_kernels_exist_and_are_claimed():
    g = _build()
    keys = kernel_keys(GRID_LIB)
    syms = [k for k in keys if k.split("<", 1)[0] == FAMILY]
    assert sorted(syms) == sorted(WANT), sorted(set(syms) ^ set(WANT))
    # tests/test_hip_general_grid.py's REACHES names these and the masked_* consumers they feed, and nothing else
    assert_claimed(syms + [k for k in keys if k.startswith("masked_")], "general_grid")
    # the family is no masked_ one, and the main library holds none of it
    assert not [k for k in keys if k.startswith("masked_") and "general" in k]
    assert not [k for k in kernel_keys(g.HIP_LIB) if "general_table" in k]


# ----------------------------------------------------------------------------- 2. the switch in Python

class _HipLib:
    is_hip = True


def _stub(cls="UMPAModelNoDF", **kw):
    """a model the way the CPU tests of the siblings build one: no native handle, only what _grid_check reads"""
    from umpa_amd import model
    m = object.__new__(type("Stub", (getattr(model, cls),), {"__del__": lambda self: None}))
    m._lib, m._mask, m._force, m._device = _HipLib(), None, 0, 0
    m._pos_list, m._shape_list, m._padding, m._max_shift = [(0, 0)] * 3, [(40, 48)] * 3, 6, 3
    m._ROI = ((0, 28, 1), (0, 36, 1))
    for k, v in kw.items():
        setattr(m, k, v)
    return m


MASK = [np.ones((40, 48))] * 3
REFUSED = [("mask", dict(_mask=MASK)), ("pos", dict(_pos_list=[(0, 0), (2, 1), (1, 3)])),
           ("pos", dict(_shape_list=[(40, 48), (40, 48), (40, 50)])), ("force", dict(_force=2))]
WHATS = ["search='grid'", "cost_volume", "basins", "track", "sequence"]


def test_switch_off_keeps_every_text_and_on_lifts_the_refusals():
    from umpa_amd import _lib, levels, model, widen
    assert _lib.F_FORCE_DIRECT == 2
    for cls in ("UMPAModelNoDF", "UMPAModelDF"):
        assert isinstance(getattr(model, cls).general_grid, property) and _stub(cls).general_grid is False
        for why, kw in REFUSED:
            off = _stub(cls, **kw)
            assert "_general_grid" not in off.__dict__
            on = _stub(cls, _general_grid=True, **kw)
            assert on.general_grid is True and on._goes_general()
            for what in WHATS:
                with pytest.raises(RuntimeError) as e:
                    off._grid_check(what)
                assert str(e.value) == "%s (grid search / cost volume): %s" % (what, TEXTS[why]), (what, why)
                on._grid_check(what)                                  # admitted
            # window widening and scale space on a model that goes the general way: refused by name, and the text says why
            for name, call in (("cost_volume, widen=2", lambda: on.cost_volume(widen=2)), ("basins, widen=2", lambda: on.basins(k=2, widen=2)),
                               ("track, widen=2", lambda: on.track(0.0, 0.0, widen=2)),
                               ("search='grid', widen=2", lambda: on.match(quiet=True, search="grid", widen=2)),
                               ("coarse_to_fine", lambda: widen.coarse_to_fine(on, levels=(2, 1, 0))),
                               ("scale_space", lambda: levels.scale_space(on, levels=(2, 1, 0)))):
                with pytest.raises(RuntimeError) as e:
                    call()
                assert FINISHED in str(e.value) and name in str(e.value) and "general" in str(e.value), (name, str(e.value))
        # a plain model with the switch on still goes tiled: widening is not refused by this rule, no coverage key
        plain = _stub(cls, _general_grid=True)
        assert not plain._goes_general() and not plain._marks_covered()
        plain._no_masked_widening("widen")
        # where coverage is not trivial the consumers mark the covered pixels; a forced plain model's coverage is trivial
        assert _stub(cls, _general_grid=True, _mask=MASK)._marks_covered()
        assert _stub(cls, _general_grid=True, _pos_list=[(0, 0), (2, 1), (1, 3)])._marks_covered()
        assert not _stub(cls, _general_grid=True, _force=2)._marks_covered()
        # an admitted masked model on one frame box keeps going down the masked path: its own refusal of widening
        adm = _stub(cls, _general_grid=True, _mask=MASK, _masked_grid=True)
        assert not adm._goes_general() and adm._marks_covered()
        with pytest.raises(RuntimeError) as e:
            adm._no_masked_widening("widen")
        assert "masked model" in str(e.value)
    # the kernel dark-field model has no table, whatever a switch says: the setter refuses, and so does the check
    k = _stub("UMPAModelDFKernel")
    with pytest.raises(RuntimeError, match="general_grid: the kernel dark-field model has no shift table"):
        k.general_grid = True
    assert k.general_grid is False
    k._general_grid = True
    with pytest.raises(RuntimeError) as e:
        k._grid_check("search='grid'")
    assert str(e.value) == "search='grid' (grid search / cost volume): " + TEXTS["dfkernel"]


# ----------------------------------------------------------------------------- 3. the inputs are admissible

def test_D_has_the_frame_sets_the_issue_counted():
    sets = G.D_sets()
    assert sets.shape == (62, 72)
    assert len(np.unique(sets)) == G.D_SETS
    assert (sets == 0).sum() == G.D_DEAD
    assert sum((sets == 1 << k).sum() for k in range(4)) == G.D_SINGLE
    xi, xj = G.D_sample()
    assert 40 <= xi.size <= 80 and set(np.unique(sets)) == set(sets[xi, xj])
    masks = G.D_masks()
    assert all(set(np.unique(m)) == {0.0, 1.0} and 0.93 < m.mean() < 0.97 for m in masks)


@pytest.mark.parametrize("kind,assign,masked", G.D_CASES, ids=G.D_IDS)
def test_D_near_tie_share_and_finite_costs(kind, assign, masked):
    """The cap is a condition on the inputs, not on the device: recomputed here from the extended-precision volumes."""
    v = G.D_hp(kind, assign, masked)
    fin = np.isfinite(v["cost"].astype(np.float64))
    dead = v["sets"] == 0
    assert not fin[:, :, dead].any() and fin[:, :, ~dead].all() and (~dead).sum() == 4428
    share, near = G.near_tie_share(v)
    print("D kind %d %s masked %d: near-tie %d" % (kind, assign, masked, near.sum()))
    assert share <= GE.NEAR_TIE_CAP and near.sum() == 0
    with np.errstate(invalid="ignore"):
        assert np.all(v["bound"][fin] < np.abs(v["cost"][fin]))       # every cost is well above its fp64 bound


@pytest.mark.parametrize("Nw,ms,Na,N1,kind,assign,masked", G.EDGE_CASES, ids=G.EDGE_IDS)
def test_edge_stacks_near_tie_share(Nw, ms, Na, N1, kind, assign, masked):
    sam, _, pos, _ = G.edge_inputs(Nw, ms, Na, N1)
    assert G.extent_of([f.shape for f in sam], pos, Nw + ms) == (G.EDGE_ROWS, N1) and G.EDGE_ROWS % 16
    v = G.edge_hp(Nw, ms, Na, N1, kind, assign, masked)
    share, near = G.near_tie_share(v)
    print("edge Nw %d ms %d Na %d w %d: near-tie %d, frame sets %d" % (Nw, ms, Na, N1, near.sum(), len(np.unique(v["sets"]))))
    assert share <= GE.NEAR_TIE_CAP
    if Na > 1:
        assert len(np.unique(v["sets"])) > 1                          # the border has pixels only some frames contribute to


@pytest.mark.parametrize("kind,assign", G.MODES, ids=["%s-%s" % ("DF" if k else "NoDF", a) for k, a in G.MODES])
def test_P_near_tie_share(kind, assign):
    sam, ref, c = GE.stack(G.P_NAME)
    v = GE.hp_volumes(kind, sam, ref, GE.window(c["Nw"]), c["ms"], c["Nw"] + c["ms"], assign)
    assert GE.near_tie(v["cost"], v["bound"]).mean() <= GE.NEAR_TIE_CAP


@pytest.mark.parametrize("kind,assign,masked", [(0, "sam", False), (1, "ref", True), (1, "sam", False), (0, "ref", True)],
                         ids=["NoDF-sam-plain", "DF-ref-mask", "DF-sam-plain", "NoDF-ref-mask"])
def test_expected_side_agrees_with_the_cpu_oracle(port_ns, kind, assign, masked):
    """The frame-set grouping, the canvas and the |S| / Na scale against the CPU oracle's own cost() on the pixel sample of D,
    which touches every frame set: within the a-priori bound at every shift, NaN where no frame contributes."""
    sam, ref, pos, Nw, ms = G.D()
    kw = dict(window_size=Nw, max_shift=ms, pos_list=[np.array(p) for p in pos])
    if masked:
        kw["mask_list"] = list(G.D_masks())
    m = (port_ns.UMPAModelDF if kind else port_ns.UMPAModelNoDF)(list(sam), list(ref), **kw)
    m.assign_coordinates = assign
    xi, xj = G.D_sample()
    v = G.D_hp(kind, assign, masked)
    pad = Nw + ms
    worst = 0.0
    for a, b in zip(xi, xj):
        got = np.array([[m.cost(int(a) + pad, int(b) + pad, float(si), float(sj))[0] for sj in range(1 - ms, ms)] for si in range(1 - ms, ms)])
        want, bound = v["cost"][:, :, a, b], v["bound"][:, :, a, b]
        if v["sets"][a, b] == 0:
            assert np.isnan(got).all() and np.isnan(want.astype(np.float64)).all()
            continue
        ratio = np.abs(got.astype(np.longdouble) - want) / bound
        worst = max(worst, float(ratio.max()))
    print("oracle against the expected side, kind %d %s masked %d: max |oracle - hp| / bound %.4f" % (kind, assign, masked, worst))
    assert worst <= 1.0
