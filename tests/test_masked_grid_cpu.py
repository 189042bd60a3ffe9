"""
The masked grid consumers (model.masked_grid, umpa_grid_set_masked), what can be checked without a GPU: the inputs of the GPU
tests (tests/masked_grid_expect.py) meet the conditions the expectations rest on, the switch is off by default and the
refusals around it come before any device work, the library exports the switch and holds the five masked kernel families, each
claimed by a GPU test.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import REPO

import grid_expect as GE
import masked_grid_expect as ME
from nativelibs import assert_claimed, build_all as _build, declared, exported, kernel_keys

GRID_LIB = os.path.join(REPO, "umpa_amd", "libumpa_grid.so")
TODAY = "masked models are not supported (their table holds finished costs)"
FAMILIES = ("masked_min_kernel", "masked_volume_kernel", "masked_basins_kernel", "masked_track_kernel", "masked_sequence_kernel")


# ----------------------------------------------------------------------------- 1. the inputs

def test_masks_are_the_issue_s():
    for name, c in GE.STACKS.items():
        m = ME.masks(name)
        rng = np.random.default_rng(100 + c["seed"])
        shape = (c["K"], c["H"], c["W"])
        binary = (rng.random(shape) >= 0.10).astype(np.float64)
        real = 0.2 + 0.8 * rng.random(shape)
        for a in (binary, real):
            a[:, 20:34, 24:40] = 0
        np.testing.assert_array_equal(m["binary"], binary)
        np.testing.assert_array_equal(m["real"], real)
        assert set(np.unique(m["binary"])) == {0.0, 1.0}
        live = m["real"][m["real"] != 0]
        assert live.min() >= 0.2 and live.max() <= 1.0 and len(np.unique(live)) > 1000


@pytest.mark.parametrize("name,which,kind,assign", ME.CASES, ids=ME.IDS)
def test_near_tie_shares_and_nan_pixel_counts(name, which, kind, assign):
    """The cap is a condition on the inputs, not on the device: recomputed here from the extended-precision volumes."""
    v = ME.hp(name, which, kind, assign)
    none, some, whole = ME.pixel_classes(v)
    near = ME.near_tie(v)
    share = near.sum() / float((~none).sum())
    print("%s %s kind %d %s: no finite cost %d, some NaN %d, near-tie %.3f %% of %d, deficient cells %d" % (
        name, which, kind, assign, none.sum(), some.sum(), 100.0 * share, (~none).sum(), v["deficient"].sum()))
    assert none.sum() == ME.NO_FINITE[name]
    assert some.sum() == ME.SOME_NAN[name]
    assert whole.sum() == none.size - ME.NO_FINITE[name] - ME.SOME_NAN[name]
    assert share <= GE.NEAR_TIE_CAP
    if which == "real":
        assert near.sum() == 0
    # a dead cell (wt = 0) is NaN in all three volumes; any other NaN is a window whose fit is singular: rank-deficient
    for k in ("cost", "T", "df"):
        if v[k] is not None:
            nan = np.isnan(v[k].astype(np.float64))
            assert nan[v["dead"]].all() and not (nan & ~v["dead"] & ~v["deficient"]).any(), k
    if kind == 0:
        assert np.array_equal(np.isnan(v["cost"].astype(np.float64)), v["dead"])
    # the pixels match() skips are among those the consumers mark: the dead block's centre is below the coverage threshold
    cov = ME.covered(name, which)
    assert not cov.all() and cov.mean() > 0.9
    assert not cov[none].any()


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
CALLS = ["search='grid'", "cost_volume", "basins", "track", "sequence"]


def _call(m, what, **kw):
    if what == "search='grid'":
        return m.match(quiet=True, search="grid", **kw)
    if what == "cost_volume":
        return m.cost_volume(**kw)
    if what == "basins":
        return m.basins(k=2, **kw)
    if what == "track":
        return m.track(0.0, 0.0, **kw)
    return m.sequence(lam=0.0)


def test_switch_defaults_to_off_and_a_stub_without_it_gives_today_s_text():
    from umpa_amd import model
    for cls in ("UMPAModelNoDF", "UMPAModelDF"):
        assert isinstance(getattr(model, cls).masked_grid, property) and _stub(cls).masked_grid is False
        m = _stub(cls, _mask=MASK)
        assert "_masked_grid" not in m.__dict__ and m.masked_grid is False
        for what in CALLS:
            with pytest.raises(RuntimeError) as e:
                _call(m, what)
            assert str(e.value) == "%s (grid search / cost volume): %s" % (what, TODAY), what
        # a stub of the base class's making, which has no such attribute at all, counts as off
        bare = object.__new__(type("Bare", (model.UMPAModelBase,), {"__del__": lambda self: None, "_kind": 0}))
        bare._lib, bare._mask, bare._force, bare._device = _HipLib(), MASK, 0, 0
        with pytest.raises(RuntimeError) as e:
            bare._grid_check("cost_volume")
        assert str(e.value) == "cost_volume (grid search / cost volume): " + TODAY
    assert not hasattr(model.UMPAModelDFKernel, "masked_grid")


def test_refusals_with_the_switch_on():
    from umpa_amd import levels, widen
    why = "a finished cost is not linear in the windowed sums, so a box average of costs is not the cost under a wider window"
    for cls in ("UMPAModelNoDF", "UMPAModelDF"):
        m = _stub(cls, _mask=MASK, _masked_grid=True)
        assert m.masked_grid is True
        m._grid_check("cost_volume")                                  # admitted
        # window widening and scale space: refused, and the text says why
        for what in CALLS[:4]:
            with pytest.raises(RuntimeError) as e:
                _call(m, what, widen=2)
            assert why in str(e.value) and "widen=2" in str(e.value), (what, str(e.value))
        with pytest.raises(RuntimeError) as e:
            widen.coarse_to_fine(m, levels=(2, 1, 0))
        assert why in str(e.value) and "coarse_to_fine" in str(e.value)
        with pytest.raises(RuntimeError) as e:
            levels.scale_space(m, levels=(2, 1, 0))
        assert why in str(e.value) and "scale_space" in str(e.value)
        # positions and shapes are tested on their own: behind a mask they used to hide
        pos = "frames at different positions (pos_list) or of different shapes are not supported"
        for kw in (dict(_pos_list=[(0, 0), (2, 1), (1, 3)]), dict(_shape_list=[(40, 48), (40, 48), (40, 50)])):
            s = _stub(cls, _mask=MASK, _masked_grid=True, **kw)
            for what in CALLS:
                with pytest.raises(RuntimeError) as e:
                    _call(s, what)
                assert str(e.value) == "%s (grid search / cost volume): %s" % (what, pos), what
        # a forced direct kernel, as on a plain model
        f = _stub(cls, _mask=MASK, _masked_grid=True, _force=2)
        with pytest.raises(RuntimeError, match="forced onto the direct kernel"):
            f.cost_volume()
    # the kernel dark-field model has no table, whatever a switch says
    k = _stub("UMPAModelDFKernel", _mask=MASK, _masked_grid=True)
    with pytest.raises(RuntimeError) as e:
        k._grid_check("search='grid'")
    assert str(e.value) == "search='grid' (grid search / cost volume): the kernel dark-field model has no shift table"
    # a model without masks: the widened calls are not refused by this rule
    plain = _stub(_masked_grid=True)
    plain._no_masked_widening("widen")


# ----------------------------------------------------------------------------- 3. the library

def test_set_masked_is_declared_exported_and_refuses_a_null_model():
    g = _build()
    from umpa_amd import _lib
    assert "umpa_grid_set_masked" in declared("umpa_grid.h", "umpa_grid_")
    assert "set_masked" in _lib.GRID_SYMBOLS and "set_masked" in _lib._GRID_ABI
    assert _lib._GRID_ABI["set_masked"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
    assert declared("umpa_grid.h", "umpa_grid_") == sorted("umpa_grid_" + s for s in _lib.GRID_SYMBOLS)
    assert "umpa_grid_set_masked" in exported(GRID_LIB)
    assert sorted(n for n in exported(GRID_LIB) if n.startswith("umpa")) == declared("umpa_grid.h", "umpa_grid_")
    lib = _lib.grid()
    for on in (0, 1):
        assert lib.set_masked(None, on) == -1                         # UMPA_HIP_E_ARG, before anything touches a device
        assert lib.error() == "grid: set_masked: null model"
    # the main library: no new public symbol; what the satellite needs of it is not in the public header
    public = sorted(n for n in exported(g.HIP_LIB) if n.startswith("umpa_hip_"))
    assert public == sorted("umpa_hip_" + s for s in _lib.HIP_SYMBOLS)
    hdr = open(os.path.join(REPO, "include", "umpa_hip.h")).read()
    assert "masked_consumer" not in hdr and "umpa_hipx" not in hdr


def test_the_five_masked_families_exist_and_are_claimed():
    g = _build()
    keys = kernel_keys(GRID_LIB)
    syms = [k for k in keys if k.startswith("masked_")]
    want = ["%s<%d>" % (f, kind) for f in FAMILIES for kind in (0, 1)]
    assert sorted(syms) == sorted(want), sorted(set(syms) ^ set(want))
    assert_claimed(syms, "masked_grid")
    # the sibling families keep their instantiations
    family = lambda f: [k for k in keys if k.split("<", 1)[0] == f]
    for f in ("grid_min_kernel", "cost_volume_kernel", "grid_basins_kernel", "grid_track_kernel", "grid_sequence_kernel"):
        assert len(family(f)) == 26, f
    # the main library holds none of them
    assert not [k for k in kernel_keys(g.HIP_LIB) if k.startswith("masked_")]
