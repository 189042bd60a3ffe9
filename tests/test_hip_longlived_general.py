"""
Long-lived models on the general shift table (``general_grid``; libumpa_grid.so's general_table_kernel): every consumer call on
one model that lives through frame swaps, geometry changes, the switch and the force bit, each against a fresh twin.

``general()`` (umpa_grid.hip) reads ``m->dev()``: the front sample buffer and the descriptor table that ``adopt_staged``
rewrites in stream order; ``general_always`` is library state in the handle that the next consumer call re-derives from the
model's forced path; with ``masked_grid`` and ``general_grid`` both on, what the masked path refuses goes to the general
table.  A stale piece of any of it faults nothing: it returns a plausible table of the wrong frames or by the wrong path.

The harness is ``test_hip_longlived.py``'s: equal bit for bit, NaN for NaN, ``last_path`` and ``ROI`` included; no tolerance
appears in this file.  The stacks are tests/general_expect.py's: E (2 x 2 stepping, equal shapes), D (unequal shapes), P (one
frame box, forced direct).  Each trajectory prints its report line.

  G1  frames swapped on a stepping stack under every consumer
  G2  geometry over time: Nw, assign_coordinates, sub_pixel_mode, ROIs and steps either side of the LDS limit, the table budget
  G3  the switch and the force bit on a one-box model: tiled (path 2), general (path 5) and back
  G4  both switches on a masked model: what the masked path refuses goes the general way
  G5  unequal shapes: update_frames, and what stage_sample does
  G6  Tracker and Sequence used more than once
  G7  borrowed device frames rewritten in place between the consumers
"""
import numpy as np
import pytest

import general_expect as G
import grid_expect as GE

from test_hip_longlived import LongLived, _counts, _device_frames, _download, hip_ns   # noqa: F401  (hip_ns: the fixture)
from test_hip_longlived_consumers import _differ, _kw, _object_step, _priors, _run

pytestmark = pytest.mark.gpu

CLS = ["UMPAModelDF", "UMPAModelNoDF"]
GENERAL_PATH = 5
P = G.E_PAR
E_EXTENT = (P["H"] - 2 * (P["Nw"] + P["ms"]), P["W"] - 2 * (P["Nw"] + P["ms"]))        # 46 x 54
FULL = ((0, E_EXTENT[0], 1), (0, E_EXTENT[1], 1))
SMALL, LARGER, STEPPED = ((10, 26, 1), (12, 32, 1)), ((4, 40, 1), (6, 50, 1)), ((3, E_EXTENT[0], 2), (5, E_EXTENT[1], 3))
POS = "frames at different positions (pos_list) or of different shapes are not supported"
KEY = dict(grid="dx", volume="cost", basins="dx", track="dx", sequence="dx")


def _E(seed=0):
    sam, ref, pos = G.E(seed)
    return np.ascontiguousarray(sam), np.ascontiguousarray(ref), pos


def _live(hip_ns, cls, label, sam=None, mask=None, general=True, **kw):
    s, ref, pos = _E()
    t = LongLived(hip_ns, cls, s if sam is None else sam, ref, P["Nw"], P["ms"], mask=mask, pos=pos, label=label, **kw)
    if general:
        t.set_general(True)
    return t


def _saw(t, *paths):
    assert set(paths) <= set(t.paths), "%s: paths seen %r, expected %r among them" % (t.label, sorted(set(t.paths)), paths)


# ----------------------------------------------------------------------------- G1. frames swapped on a stepping stack

@pytest.mark.parametrize("consumer", ["grid", "volume", "basins", "track", "sequence"])
@pytest.mark.parametrize("cls", CLS)
def test_frames_swapped_on_a_stepping_stack(hip_ns, cls, consumer):
    """the script of test_frames_swapped_under_the_consumers on E: the consumer is the first reader of every staged stack"""
    samA, refA, _ = _E()
    samB, samC = _E(1)[0], _E(2)[0]
    rng = np.random.default_rng(3)
    refB = np.ascontiguousarray(refA + 0.002 * rng.standard_normal(refA.shape))
    dark = 100.0 + rng.uniform(0, 2, size=samA.shape)
    flat = 20000.0 * (1.0 + 0.05 * rng.standard_normal(samA.shape))
    d_dark, d_flat = _device_frames(dark), _device_frames(flat)
    t = _live(hip_ns, cls, "G1 swapped %s %s" % (consumer, cls))
    go = lambda what, roi=FULL, device=False: _run(hip_ns, t, consumer, roi, what, device=device)
    first = go("as built")
    t.update(sam=samB)
    after = go("update_frames(sam)")
    assert _differ(first, after, KEY[consumer])                       # (the stacks differ: a stale one would show)
    t.stage(np.ascontiguousarray(samA))
    back = go("first after stage_sample float64", device=True)
    assert not t.live._use_staged and not _differ(first, back, KEY[consumer])
    t.stage(_counts(samC, flat, dark), dark=d_dark, flat=d_flat)
    go("first after stage_sample uint16 with device dark and flat")
    assert not t.live._use_staged
    t.stage(np.ascontiguousarray(samA))
    t.stage(np.ascontiguousarray(0.5 * samB))
    go("two stage_sample calls, the second wins")
    t.stage(np.ascontiguousarray(samC))
    t.update(sam=samB)
    assert not t.live._use_staged
    won = go("stage_sample, update_frames(sam): the update wins", device=True)
    assert not _differ(won, after, KEY[consumer])
    t.update(ref=refB)
    moved = go("update_frames(ref)")
    assert _differ(moved, after, KEY[consumer])
    t.match("the walk between the consumers", ROI=FULL)
    go("a small ROI", SMALL)
    go("a larger ROI after it", LARGER, device=True)
    go("a stepped ROI", STEPPED)
    t.match("the walk afterwards", ROI=FULL)
    t.report()
    _saw(t, GENERAL_PATH)


# ----------------------------------------------------------------------------- G2. geometry over time

@pytest.mark.parametrize("cls", CLS)
def test_geometry_over_time(hip_ns, cls, monkeypatch):
    monkeypatch.delenv("UMPA_HIP_TABLE_MB", raising=False)
    t = _live(hip_ns, cls, "G2 geometry " + cls)
    go = lambda name, what, roi=FULL, device=False: _run(hip_ns, t, name, roi, what, device=device)
    w2 = go("volume", "as built")
    t.set(Nw=1)
    w1 = go("volume", "Nw 1: padding stays, footprints shrink")
    go("basins", "Nw 1")
    t.set(Nw=P["Nw"])
    back = go("volume", "Nw 2 again")
    assert _differ(w1, w2, "cost") and not _differ(back, w2, "cost")
    t.set(assign="ref")
    as_ref = go("volume", "reference coordinates")
    go("track", "reference coordinates", device=True)
    assert _differ(as_ref, w2, "cost")
    for subpx in (0, 1):
        t.set(subpx=subpx)
        go("grid", "sub_pixel_mode %d" % subpx)
        go("basins", "sub_pixel_mode %d" % subpx, SMALL)
    t.set(subpx=-1)
    go("sequence", "a (2, 3)-step ROI with an offset", ((3, E_EXTENT[0], 2), (5, E_EXTENT[1], 3)))
    # either side of the LDS limit at Nw 2, max_shift 3: general_expect.lds_geometry, the restatement the CPU module holds to
    # the host sweep program's list
    assert G.lds_geometry(P["Nw"], P["ms"], 3, 4, False, 1)[0] == "staged" and G.lds_geometry(P["Nw"], P["ms"], 4, 4, False, 1)[0] == "fallback"
    staged = go("volume", "step (3, 4): the last that is staged", ((1, E_EXTENT[0], 3), (2, E_EXTENT[1], 4)))
    fallback = go("volume", "step (4, 4): just past LDS, the fallback", ((1, E_EXTENT[0], 4), (2, E_EXTENT[1], 4)))
    assert np.array_equal(staged["cost"][:, :, ::4, :], as_ref["cost"][:, :, 1::12, 2::4], equal_nan=True)
    assert np.array_equal(fallback["cost"], as_ref["cost"][:, :, 1::4, 2::4], equal_nan=True)
    go("track", "unit steps again")
    t.set(assign="sam")
    go("basins", "sample coordinates again")
    t.report()
    _saw(t, GENERAL_PATH)


@pytest.mark.parametrize("cls", CLS)
def test_table_budget_over_time_on_the_general_table(hip_ns, cls, monkeypatch):
    """The sizing argument of test_hip_general_grid.py's _chunk_model: 65 columns, max_shift 8, so that a row of the table is
    225 x NV x 65 doubles and the smallest budget (16 MiB) holds 47 rows with dark-field (NV = 3) and 71 without (NV = 2) -- 32
    and 64 after rounding to the workgroup's 16.  53 rows with dark-field and 85 without: two row chunks under 16 MiB, one
    under the default budget.  One chunk, two, one again, the consumers in between."""
    from umpa_amd.synth import make_stack
    monkeypatch.delenv("UMPA_HIP_TABLE_MB", raising=False)
    NV, rows = (3, 53) if cls == "UMPAModelDF" else (2, 85)
    per_row = 225 * NV * 65 * 8
    chunk = max(16, (16 << 20) // per_row // 16 * 16)
    assert chunk < rows <= 2 * chunk, (chunk, rows)
    sam, ref, _ = make_stack(rows + 2 * 9 - 3, 65 + 2 * 9 - 5, 3, 8, df=True, seed=77, amplitude=3.0, order=1)
    pos = [(0, 0), (3, 5), (0, 5)]
    t = LongLived(hip_ns, cls, sam, ref, 1, 8, pos=pos, label="G2 budget " + cls)
    t.set_general(True)
    assert t.live.extent == (rows, 65)
    full = ((0, rows, 1), (0, 65, 1))
    kept = {}
    for tag, mb in (("default budget", None), ("16 MiB: two chunks", "16"), ("default budget again", None)):
        if mb:
            monkeypatch.setenv("UMPA_HIP_TABLE_MB", mb)
        else:
            monkeypatch.delenv("UMPA_HIP_TABLE_MB", raising=False)
        kept[tag] = t.basins("basins, " + tag, k=2, ROI=full)
        t.volume("cost_volume, " + tag, with_fit=True, ROI=full)
        pdx, pdy = _priors(t, full)
        t.track(pdx, pdy, "track, " + tag, device=mb is not None, lam=0.02, radius=3.0, ROI=full)
    assert not _differ(kept["default budget"], kept["16 MiB: two chunks"], "dx")
    t.report()
    _saw(t, GENERAL_PATH)


# ----------------------------------------------------------------------------- G3. the switch and the force bit

@pytest.mark.parametrize("cls", CLS)
def test_the_switch_and_the_force_bit(hip_ns, cls):
    """P, one frame box: with the switch on and nothing forced the consumers stay on the tiled table (path 2); forced onto the
    direct kernel they go the general way (path 5, general_always in the handle); the force gone, the NEXT call is back on
    path 2 with the first result's bits."""
    from umpa_amd import _lib
    sam, ref, c = GE.stack(G.P_NAME)
    t = LongLived(hip_ns, cls, sam, ref, c["Nw"], c["ms"], label="G3 switch and force " + cls)
    t.set_general(True)
    n0, n1 = t.live.extent
    full = ((0, n0, 1), (0, n1, 1))
    kw = _kw(hip_ns)
    pdx, pdy = _priors(t, full)

    def consumers(what, path):
        out = [t.grid("grid, " + what, expect_path=path, ROI=full), t.volume("cost_volume, " + what, with_fit=True, ROI=full),
               t.basins("basins, " + what, k=3, ROI=full),
               t.track(pdx, pdy, "track, " + what, lam=kw["lam"], radius=kw["radius"], ROI=full)]
        assert t.paths[-4:] == [path] * 4, (what, t.paths[-4:])
        return out

    tiled = consumers("switch on, unforced", 2)
    walk = t.match("the walk", ROI=full)
    t.set_force(_lib.F_FORCE_DIRECT)
    forced = consumers("forced direct", GENERAL_PATH)
    t.set_force(0)
    again = consumers("the force gone", 2)
    for a, b in zip(tiled, again):
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), k
    t.set_force(_lib.F_FORCE_DIRECT)
    forced2 = consumers("forced again", GENERAL_PATH)
    assert not _differ(forced[1], forced2[1], "cost")
    t.set_general(False)
    m = t.live
    for what, call in (("search='grid'", lambda: m.match(quiet=True, search="grid")), ("cost_volume", lambda: m.cost_volume()),
                       ("basins", lambda: m.basins()), ("track", lambda: m.track(0.0, 0.0)), ("sequence", lambda: m.sequence(lam=0.0))):
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == "%s (grid search / cost volume): the model is forced onto the direct kernel" % what, what
    t.match("switch off, forced: the walk")
    t.set_force(0)
    w2 = t.match("switch off, unforced: the walk", ROI=full)
    assert not _differ(walk, w2, "dx") and not _differ(walk, w2, "f")
    t.set_general(True)
    t.set_force(_lib.F_FORCE_DIRECT)
    consumers("switch on again, forced", GENERAL_PATH)
    t.report()
    _saw(t, 2, GENERAL_PATH)


@pytest.mark.parametrize("cls", CLS)
def test_the_switch_off_and_on_around_the_refusals(hip_ns, cls):
    """E with the switch off: every refusal text of test_switch_on_off_and_the_refusals_around_it, verbatim, and the walk
    unchanged; on again, the consumers equal a fresh twin's"""
    t = _live(hip_ns, cls, "G3 refusals " + cls)
    kw = _kw(hip_ns)
    on = t.basins("basins, switch on", k=3, ROI=FULL)
    before = t.match("the walk", ROI=FULL)
    t.set_general(False)
    m = t.live
    for what, call in (("search='grid'", lambda: m.match(quiet=True, search="grid")), ("cost_volume", lambda: m.cost_volume()),
                       ("basins", lambda: m.basins()), ("track", lambda: m.track(0.0, 0.0)), ("sequence", lambda: m.sequence(lam=0.0))):
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == "%s (grid search / cost volume): %s" % (what, POS), what
    after = t.match("the walk after the refusals", ROI=FULL)
    assert not _differ(before, after, "dx") and not _differ(before, after, "f")
    t.set_general(True)
    again = t.basins("basins, switch on again", k=3, ROI=FULL)
    assert not _differ(on, again, "dx")
    t.sequence("sequence, switch on again", lam=kw["lam"], trunc=kw["trunc"], ROI=FULL)
    t.report()
    _saw(t, GENERAL_PATH)


# ----------------------------------------------------------------------------- G4. both switches on a masked model

def _masks(kind, shape, seed=5):
    rng = np.random.default_rng(seed)
    if kind == "binary":
        return (rng.random(shape) < 0.9).astype(np.float64)
    return rng.uniform(0.0, 1.0, size=shape) * (rng.random(shape) < 0.95)


def _past_limit(cls):
    """the smallest step product above the masked step limit (16 dense pixels per requested one without dark-field, 5 with it,
    at up to 81 shifts): 17 = 1 x 17, 6 = 2 x 3"""
    return (1, 17) if cls == "UMPAModelNoDF" else (2, 3)


@pytest.mark.parametrize("kind", ["binary", "weights"])
@pytest.mark.parametrize("cls", CLS)
def test_both_switches_on_a_masked_stepping_stack(hip_ns, cls, kind):
    samA, refA, pos = _E()
    mask = _masks(kind, samA.shape)
    t = _live(hip_ns, cls, "G4 both switches, E %s %s" % (cls, kind), mask=mask, general=False)
    t.set_masked(True)
    t.set_general(True)
    unit = t.volume("unit steps, both switches", with_fit=True, ROI=FULL)
    unit_path = t.paths[-1]
    s0, s1 = _past_limit(cls)
    roi = ((1, E_EXTENT[0], s0), (2, E_EXTENT[1], s1))
    stepped = t.volume("a step past the masked limit", with_fit=True, ROI=roi)
    assert t.paths[-1] == GENERAL_PATH
    plain = _live(hip_ns, cls, "twin, masked_grid off", mask=mask)       # (a fresh model, the masked switch off)
    dense = _download(plain.live.cost_volume(with_fit=True, ROI=FULL))
    for k in ("cost", "T") + (("df",) if cls == "UMPAModelDF" else ()):
        assert np.array_equal(stepped[k], dense[k][:, :, 1::s0, 2::s1], equal_nan=True), k
    t.basins("basins past the limit", k=3, ROI=roi)
    t.set_masked(False)
    t.volume("masked_grid off: still the general way", with_fit=True, ROI=roi)
    assert t.paths[-1] == GENERAL_PATH
    t.set_masked(True)
    t.update(sam=_E(1)[0])
    t.grid("update_frames(sam), both switches", ROI=FULL)
    t.report()
    print("[long-lived] %s: the unit-step call went path %d" % (t.label, unit_path))
    _saw(t, GENERAL_PATH)


@pytest.mark.parametrize("kind", ["binary", "weights"])
@pytest.mark.parametrize("cls", CLS)
def test_both_switches_on_a_masked_frame_box(hip_ns, cls, kind):
    """A masked model on ONE frame box is the model the masked path takes of its own accord: with both switches on, unit steps
    stay on it (path 2) and only what masked_consumer_refusal refuses goes to the general table (run_match's second general
    branch).  With general_grid off the refusal is the masked path's own text."""
    sam, ref, c = GE.stack(G.P_NAME)
    Nw, ms = c["Nw"], c["ms"]
    mask = _masks(kind, sam.shape)
    t = LongLived(hip_ns, cls, sam, ref, Nw, ms, mask=mask, label="G4 both switches, one box %s %s" % (cls, kind))
    t.set_masked(True)
    t.set_general(True)
    n0, n1 = t.live.extent
    full = ((0, n0, 1), (0, n1, 1))
    t.volume("unit steps: the masked path", with_fit=True, ROI=full)
    unit_path = t.paths[-1]
    s0, s1 = _past_limit(cls)
    roi = ((1, n0, s0), (2, n1, s1))
    stepped = t.volume("a step past the masked limit: the general table", with_fit=True, ROI=roi)
    assert t.paths[-1] == GENERAL_PATH
    plain = LongLived(hip_ns, cls, sam, ref, Nw, ms, mask=mask, label="twin, masked_grid off")
    plain.set_general(True)
    dense = _download(plain.live.cost_volume(with_fit=True, ROI=full))
    assert plain._path(plain.live) == GENERAL_PATH
    for k in ("cost", "T") + (("df",) if cls == "UMPAModelDF" else ()):
        assert np.array_equal(stepped[k], dense[k][:, :, 1::s0, 2::s1], equal_nan=True), k
    t.basins("basins past the limit", k=3, ROI=roi)
    t.set_masked(False)
    t.volume("masked_grid off: still the general way", with_fit=True, ROI=roi)
    assert t.paths[-1] == GENERAL_PATH
    t.set_masked(True)
    t.set_general(False)
    lim, base = (16, 16) if cls == "UMPAModelNoDF" else (5, 5)
    with pytest.raises(RuntimeError) as e:
        t.live.cost_volume(ROI=roi)
    assert ("steps %d x %d: the masked table is filled on the dense grid, its step limit is %d dense pixels per requested one "
            "(%d at up to 81 shifts, fewer beyond)" % (s0, s1, lim, base)) in str(e.value), str(e.value)
    t.volume("general_grid off, unit steps: the masked path", with_fit=True, ROI=full)
    t.set_general(True)
    t.volume("on again, past the limit", with_fit=True, ROI=roi)
    t.report()
    print("[long-lived] %s: the unit-step call went path %d" % (t.label, unit_path))
    _saw(t, GENERAL_PATH)
    assert unit_path == 2


@pytest.mark.parametrize("which", ["exact fit", "no configuration"])
@pytest.mark.parametrize("cls", CLS)
def test_the_other_two_refusals_go_the_general_way(hip_ns, cls, which):
    """One frame with Nw 1 and masks (exact fit: 1 x 9 <= 9), and window half-width 9, for which masked_supported
    (umpa_tiled.h: configurations for 1 to 8) is false.  Both switches on: path 5, the volume within the a-priori bound of
    extended precision and equal to model.cost bit for bit on a pixel sample.  The exact fit leaves run_match through its
    second general branch; Nw 9 through the first, since tiled_applicable refuses it before (no tiled path takes it whole)."""
    kind = int(cls == "UMPAModelDF")
    sam, ref, mask, Nw, ms = G.refused_inputs(which)
    pad, rows, N1 = Nw + ms, G.EDGE_ROWS, G.REFUSED[which][3]
    t = LongLived(hip_ns, cls, sam, ref, Nw, ms, mask=mask, label="G4 %s %s" % (which, cls))
    t.set_masked(True)
    t.set_general(True)
    vol = t.volume(which, with_fit=True)
    assert t.paths[-1] == GENERAL_PATH and vol["cost"].shape == (3, 3, rows, N1)
    worst = G.within_bound(vol["cost"], G.refused_hp(which, kind), which)
    m = t.live
    for a, b in ((0, 0), (0, N1 - 1), (rows - 1, 0), (rows - 1, N1 - 1), (15, 15), (16, 16), (10, 31)):
        want = np.array([[m.cost(a + pad, b + pad, float(si), float(sj)) for sj in range(1 - ms, ms)] for si in range(1 - ms, ms)])
        for q, k in enumerate(("cost", "T") + (("df",) if kind else ())):
            np.testing.assert_array_equal(vol[k][:, :, a, b], want[:, :, q], err_msg="%s at (%d, %d)" % (k, a, b))
    t.basins("basins", k=2)
    t.report()
    print("[long-lived] %s: max |gpu - hp| / bound %.4f" % (t.label, worst))


# ----------------------------------------------------------------------------- G5. unequal shapes

@pytest.mark.parametrize("cls", CLS)
def test_frames_swapped_on_unequal_shapes(hip_ns, cls):
    """D: update_frames with D's own shapes; stage_sample takes a stack of the model's shapes too and is held to the twin"""
    sam, ref, pos, Nw, ms = G.D()
    rng = np.random.default_rng(21)
    samB = [f + 0.002 * rng.standard_normal(f.shape) for f in sam]
    refB = [f + 0.002 * rng.standard_normal(f.shape) for f in ref]
    t = LongLived(hip_ns, cls, list(sam), list(ref), Nw, ms, pos=pos, label="G5 unequal shapes " + cls)
    t.set_general(True)
    kw = _kw(hip_ns)
    n0, n1 = t.live.extent
    full = ((0, n0, 1), (0, n1, 1))
    pdx, pdy = _priors(t, full)
    first = t.basins("basins, as built", k=3, ROI=full)
    t.update(sam=samB)
    after = t.basins("basins, update_frames(sam)", k=3, ROI=full)
    assert _differ(first, after, "dx")
    t.track(pdx, pdy, "track, update_frames(sam)", device=True, lam=kw["lam"], radius=kw["radius"], ROI=full)
    t.update(ref=refB)
    t.track(pdx, pdy, "track, update_frames(ref)", lam=kw["lam"], radius=kw["radius"], ROI=full)
    moved = t.basins("basins, update_frames(ref)", k=3, ROI=full)
    assert _differ(moved, after, "dx")
    t.stage([np.ascontiguousarray(f) for f in sam])
    assert t.live._use_staged
    back = t.basins("basins, first after stage_sample", k=3, ROI=full)
    assert not t.live._use_staged and _differ(back, moved, "dx")
    t.stage([np.ascontiguousarray(f.astype(np.float32)) for f in samB])
    t.volume("cost_volume, first after stage_sample float32", with_fit=True, ROI=full)
    t.report()
    _saw(t, GENERAL_PATH)


# ----------------------------------------------------------------------------- G6. Tracker and Sequence used more than once

def _projections():
    return [_E(seed)[0] for seed in (1, 2, 3, 4)]


@pytest.mark.parametrize("cls", CLS)
def test_sequence_object_on_a_stepping_stack(hip_ns, cls):
    from umpa_amd import Sequence
    Pj = _projections()
    kw = _kw(hip_ns)
    t = _live(hip_ns, cls, "G6 Sequence " + cls, sam=Pj[0])
    t.set(ROI=FULL)
    seq = Sequence(t.live, kw["lam"], trunc=kw["trunc"])
    need = t._fit() + ("state", "cost", "total", "cost0", "shift", "moved", "covered")
    results = []
    for p in range(4):
        prev = None if seq.state is None else seq.state.cpu().numpy()
        assert (p == 0) == (prev is None)
        results.append(_object_step(t, seq, Pj[p], lambda m: m.sequence(state=prev, lam=kw["lam"], trunc=kw["trunc"]), "projection %d" % p, need))
    assert _differ(_download(results[1]), _download(results[2]), "dx")
    seq.reset()
    _object_step(t, seq, Pj[2], lambda m: m.sequence(state=None, lam=kw["lam"], trunc=kw["trunc"]), "after reset(): a series starts", need)
    t.report()
    _saw(t, GENERAL_PATH)


@pytest.mark.parametrize("cls", CLS)
def test_tracker_object_on_a_stepping_stack(hip_ns, cls):
    from umpa_amd import Tracker
    Pj = _projections()
    kw = _kw(hip_ns)
    t = _live(hip_ns, cls, "G6 Tracker " + cls, sam=Pj[0])
    t.set(ROI=FULL)
    tr = Tracker(t.live, lam=kw["lam"], radius=kw["radius"])
    need = t._fit() + ("cost", "cost0", "shift", "count", "found", "covered")
    results = []
    for p in range(4):
        prior = [np.full(t.live.sh, np.nan)] * 2 if tr.prior is None else [a.cpu().numpy() for a in tr.prior]
        results.append(_object_step(t, tr, Pj[p], lambda m: m.track(prior[0], prior[1], lam=kw["lam"], radius=kw["radius"]), "projection %d" % p, need))
    assert _differ(_download(results[1]), _download(results[2]), "dx")
    t.report()
    _saw(t, GENERAL_PATH)


# ----------------------------------------------------------------------------- G7. borrowed device frames

@pytest.mark.parametrize("cls", CLS)
def test_borrowed_frames_rewritten_between_the_consumers(hip_ns, cls):
    """a model on borrowed device frames takes pos_list; the stacks are rewritten where they lie between the consumers"""
    samA, refA, pos = _E()
    samB = _E(1)[0]
    refB = np.ascontiguousarray(refA + 0.002 * np.random.default_rng(3).standard_normal(refA.shape))
    t = LongLived(hip_ns, cls, samA, refA, P["Nw"], P["ms"], pos=pos, label="G7 borrowed " + cls, borrowed=True)
    t.set_general(True)
    first = _run(hip_ns, t, "basins", FULL, "as built")
    t.write(sam=samB)
    second = _run(hip_ns, t, "basins", FULL, "the sample stack rewritten in place")
    assert _differ(first, second, "dx")
    _run(hip_ns, t, "track", FULL, "the same stack", device=True)
    t.write(ref=refB)
    _run(hip_ns, t, "volume", STEPPED, "the reference stack rewritten in place, a stepped ROI")
    _run(hip_ns, t, "sequence", FULL, "a series", series=True)
    t.write(sam=samA, ref=refA)
    back = _run(hip_ns, t, "basins", FULL, "both stacks as built again")
    assert not _differ(first, back, "dx")
    t.report()
    _saw(t, GENERAL_PATH)
