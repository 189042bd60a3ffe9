"""
Long-lived models, the table's later consumers: ``basins``, ``track``, ``sequence``, window widening, the level chains, the
``masked_grid`` switch, ``uncertainty(resident=True)``, ``Tracker`` and ``Sequence`` -- each against a fresh model.

``test_hip_longlived.py`` drives one model through many calls and holds every answer, bit for bit, to a twin that has only
ever been in the recorded state.  The consumers named above read the same surviving state as the walk -- the reference-side
maps and ``TiledState::ref_rect``, the grow-only map and table scratch, the two sample buffers, the one-shot staged flag, the
table consumer hook, the on-demand stages -- and their own modules test one transition each.  The trajectories here put them
in front of and behind the histories in which stale state has lived before:

  A  a ROI that left ``ref_rect`` a strict subset of what the consumer needs, a ROI covered by a larger rectangle that a
     consumer (not the walk) computed, an ``Nw`` change, ``assign_coordinates`` and ``sub_pixel_mode`` flipped between calls;
  B  ``widen=b``, whose pooling reads tiles outside the rectangle the preceding call left (the geometry test restates which),
     ``b`` going down and up, ``Nw`` and the reference stack changed between widened calls;
  C  the table budget changed between calls: one chunk, four chunks with a carry of ``2b`` rows, one chunk again;
  D  frames swapped under each consumer: ``update_frames``, both kinds of ``stage_sample``, even and odd numbers of buffer
     swaps, a staged stack that is pending while ``uncertainty(resident=True)`` reads the adopted one;
  E  a masked model with the switch turned on, off and on again around the walk, whose on-demand stages must come back;
  F  one ``Sequence`` and one ``Tracker`` over many steps, resets, ROI changes and a match behind the object's back.

No tolerance appears in this file: every comparison is the harness's -- equal bit for bit, NaN for NaN, ``last_path`` and
``ROI`` included.  Each trajectory asserts once that a mutation changed the answer (a twin in the wrong state would have
failed) and prints its report line.

35 cases, 13 s on an MI355X host when the module runs alone -- 11 s of them are the first use of HIP tensors in the process,
which falls to whichever test comes first; behind it no case takes more than half a second (the stacks are small: what costs
is the twins and the host copies, not the kernels).  In the whole suite no case of this module is among the slowest 40.
"""
import ctypes

import numpy as np
import pytest

from test_hip_longlived import (FULL, H1, K1, MS1, ROI_IN, ROI_OUT, W1, WS1, LongLived, _counts, _device_frames, _download,
                                _prep_rect, _smooth_kw, _stack, hip_ns)          # noqa: F401  (hip_ns: the fixture)

pytestmark = pytest.mark.gpu

CLS = ["UMPAModelDF", "UMPAModelNoDF"]


def _kw(hip_ns):
    """lam and trunc of every call of this file, from the cost scale of test_hip_longlived's _smooth_kw; the radius is a
    distance in pixels.  No step depends on a default."""
    p = _smooth_kw(hip_ns)
    return dict(lam=p["lam"], trunc=p["trunc"], radius=3.0)


def _shape(t, roi, b=0):
    """the pixels a call on `roi` widened by `b` returns"""
    from umpa_amd import widen
    r = widen.valid_region(t.live, b, ROI=roi)
    return len(range(*r[0])), len(range(*r[1]))


def _priors(t, roi, b=0, seed=1):
    """(prior_dx, prior_dy) of the region a call returns: a seeded field within the search range, a few pixels blind"""
    rng = np.random.default_rng(seed)
    shape = _shape(t, roi, b)
    pdx, pdy = rng.uniform(-3.0, 3.0, shape), rng.uniform(-3.0, 3.0, shape)
    pdx[rng.random(shape) < 0.03] = np.nan
    return pdx, pdy


def _state(hip_ns, t, roi, seed=2):
    """a state for sequence(): accumulated costs on the scale of one projection's"""
    rng = np.random.default_rng(seed)
    U = 2 * t.rec["max_shift"] - 1
    return np.ascontiguousarray(_kw(hip_ns)["trunc"] * rng.random((U, U) + _shape(t, roi)))


KEY = dict(basins="dx", track="dx", sequence="dx", grid_widen="dx", volume_widen="cost", grid="dx", volume="cost",
           scale_space="sel.dx", coarse_to_fine="sel.dx", resident="unit")


def _run(hip_ns, t, name, roi, what, device=False, series=False, b=1):
    """one call of the consumer `name` on `roi`, as a step of `t`; series: sequence() starts a series and goes on with the
    state it returned (two steps)"""
    kw = _kw(hip_ns)
    if name == "basins":
        return t.basins("basins, " + what, k=3, ROI=roi)
    if name == "track":
        pdx, pdy = _priors(t, roi)
        return t.track(pdx, pdy, "track, " + what, device=device, lam=kw["lam"], radius=kw["radius"], ROI=roi)
    if name == "sequence":
        if series:
            first = t.sequence("sequence, a series starts, " + what, lam=kw["lam"], trunc=kw["trunc"], ROI=roi)
            state = first["state"]
        else:
            state = _state(hip_ns, t, roi)
        return t.sequence("sequence with a state, " + what, state=state, device=device, lam=kw["lam"], trunc=kw["trunc"], ROI=roi)
    if name == "grid":
        return t.grid("grid search, " + what, ROI=roi)
    if name == "volume":
        return t.volume("cost_volume, " + what, ROI=roi, with_fit=True)
    if name == "grid_widen":
        return t.grid("grid search widen=%d, %s" % (b, what), ROI=roi, widen=b)
    if name == "volume_widen":
        return t.volume("cost_volume widen=%d, %s" % (b, what), ROI=roi, widen=b)
    if name == "scale_space":
        return t.scale_space("scale_space, " + what, levels=(2, 1, 0), tol=0.5, lam=kw["lam"], radius=kw["radius"], ROI=roi)
    if name == "resident":
        return t.resident(dict(ROI=roi), "uncertainty(resident=True), " + what)
    raise KeyError(name)


def _differ(a, b, key):
    """the two answers are different numbers: a comparison against a twin in the other state would have failed"""
    return a[key].shape != b[key].shape or not np.array_equal(a[key], b[key], equal_nan=True)


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


# ----------------------------------------------------------------------------- the tiles a widened call needs

def _grown(E, roi, b):
    """the region a widened call is made on (model.widen_region, unit steps): the requested one grown by b pixels on every
    side, or by as many as stay inside the extent E"""
    out = []
    for n, (a, e, s) in zip(E, roi):
        assert s == 1
        out.append((a - min(b, a), e + min(b, n - e), 1))
    return tuple(out)


def test_a_widened_call_reads_tiles_past_the_rectangle_of_its_region():
    """The pooled table of a widen=b call is built from the raw table of the region grown by b (umpa_widen_geom.h: a pooled row
    r needs the raw rows r - b .. r + b; model.widen_region grows the call's region accordingly), and the raw table of a region
    reads the maps of prep_rect's tiles.  At Nw = 4 ROI_IN alone reads tx [1, 3) x ty [1, 2): its last row 55 reads the maps
    up to tile (55 + pad + max_shift - Nw) / 32 = 1.  Grown by 1, 3 or 8 pixels its last row is 56, 58 or 63, which reads tile
    row 2: the widened call reads ty [1, 3), one tile row that the walk on ROI_IN did not prepare -- and one below ROI_OUT's
    ty [0, 2).  At Nw = 3 ROI_IN's own rectangle has that tile row already."""
    from umpa_amd import model as M
    pad = WS1 + MS1
    E = (H1 - 2 * pad, W1 - 2 * pad)
    for b in (1, 3, 8):                                               # the restatement above is widen_region's
        native = M.widen_region(E, ROI_IN[0], ROI_IN[1], 16, 20, b)[0]
        assert (native[0], native[1]) == _grown(E, ROI_IN, b), (b, native)
        assert M.widen_region(E, ROI_IN[0], ROI_IN[1], 16, 20, b)[2] == ROI_IN      # ... and every requested pixel is kept
    assert _grown(E, ROI_IN, 8) == ((32, 64, 1), (32, 68, 1)) and _grown(E, FULL, 3) == FULL
    inner, outer = _prep_rect(H1, W1, 4, MS1, pad, ROI_IN), _prep_rect(H1, W1, 4, MS1, pad, ROI_OUT)
    assert (inner, outer) == ((1, 3, 1, 2), (1, 4, 0, 2))
    for b in (1, 3, 8):
        wide = _prep_rect(H1, W1, 4, MS1, pad, _grown(E, ROI_IN, b))
        assert wide == (1, 3, 1, 3), (b, wide)
        assert wide[0] <= inner[0] and wide[1] >= inner[1] and wide[2] <= inner[2] and wide[3] > inner[3]     # strictly larger
    assert _prep_rect(H1, W1, 4, MS1, pad, _grown(E, ROI_IN, 8))[3] > outer[3]                                # past ROI_OUT's below
    for b in (1, 3, 8):
        assert _prep_rect(H1, W1, 3, MS1, pad, _grown(E, ROI_IN, b)) == _prep_rect(H1, W1, 3, MS1, pad, ROI_IN) == (1, 3, 1, 3)


# ----------------------------------------------------------------------------- A. the cached rectangle under every consumer

@pytest.mark.parametrize("consumer", ["basins", "track", "sequence", "grid_widen", "volume_widen", "scale_space"])
@pytest.mark.parametrize("cls", CLS)
def test_cached_rectangle_under_every_consumer(hip_ns, cls, consumer):
    """A new window drops every map, so the walk on ROI_IN leaves ref_rect a strict subset of the tiles; the consumer then
    outgrows it (ROI_OUT at Nw 3, the whole region at Nw 4), the walk returns to ROI_IN, and the consumer on ROI_IN finds
    itself covered by the larger rectangle that a consumer computed."""
    sam, ref = _stack(5)
    t = LongLived(hip_ns, cls, sam, ref, WS1, MS1, label="A rectangle %s %s" % (consumer, cls))
    b = 2 if consumer == "grid_widen" else 1
    inside = {}
    for nw, large in ((3, ROI_OUT), (4, FULL)):
        t.set(Nw=nw)
        t.match("Nw %d, the walk on ROI_IN: a strict subset of the tiles" % nw, expect_path=2, ROI=ROI_IN)
        _run(hip_ns, t, consumer, large, "past the walk's rectangle", series=True, device=nw == 4, b=b)
        t.match("the walk on ROI_IN again", expect_path=2, ROI=ROI_IN)
        inside[nw] = _run(hip_ns, t, consumer, ROI_IN, "covered by the consumer's rectangle", series=True, device=nw == 3, b=b)
    assert _differ(inside[3], inside[4], KEY[consumer])               # (the windows differ: maps of the other one would show)
    t.set(assign="ref")
    as_ref = _run(hip_ns, t, consumer, ROI_OUT, "reference coordinates", b=b)
    t.set(assign="sam")
    as_sam = _run(hip_ns, t, consumer, ROI_OUT, "sample coordinates again", b=b)
    assert _differ(as_ref, as_sam, KEY[consumer])
    for subpx in (0, 1, -1):
        t.set(subpx=subpx)
        _run(hip_ns, t, consumer, ROI_IN if subpx == 0 else ROI_OUT, "sub_pixel_mode %d" % subpx, b=b)
    t.report()


# ----------------------------------------------------------------------------- B. widening reaches past the rectangle

@pytest.mark.parametrize("cls", CLS)
def test_widening_reaches_past_the_rectangle(hip_ns, cls):
    """the tiles: test_a_widened_call_reads_tiles_past_the_rectangle_of_its_region"""
    samA, refA = _stack(5)
    _, refB = _stack(9, amplitude=2.0)
    kw = _kw(hip_ns)
    t = LongLived(hip_ns, cls, samA, refA, WS1, MS1, label="B widening " + cls)
    t.match("the walk on ROI_IN: tiles ty [1, 2)", expect_path=2, ROI=ROI_IN)
    w1 = t.grid("widen=1 on ROI_IN: tile row 2 was not prepared", expect_path=2, ROI=ROI_IN, widen=1)
    w0 = t.grid("widen=0", expect_path=2, ROI=ROI_IN, widen=0)
    assert _differ(w1, w0, "dx")
    t.match("the walk on ROI_IN", expect_path=2, ROI=ROI_IN)
    by_b = {}
    for b in (8, 1, 3):
        by_b[b] = t.grid("widen going down and up: %d" % b, ROI=ROI_IN, widen=b)
    assert _differ(by_b[8], by_b[1], "dx") and _differ(by_b[1], by_b[3], "dx") and not _differ(by_b[1], w1, "dx")
    t.volume("cost_volume widen=8", ROI=ROI_IN, widen=8)
    t.basins("basins widen=1", k=3, ROI=ROI_IN, widen=1)
    pdx, pdy = _priors(t, ROI_IN, 3)
    t.track(pdx, pdy, "track widen=3, device priors", device=True, lam=kw["lam"], radius=kw["radius"], ROI=ROI_IN, widen=3)
    # at the border of the extent two half-widths keep two different regions
    f3 = t.grid("the whole region, widen=3", ROI=FULL, widen=3)
    f1 = t.grid("the whole region, widen=1", ROI=FULL, widen=1)
    assert f3["region"].tolist() == [[3, 101, 1], [3, 121, 1]] and f1["region"].tolist() == [[1, 103, 1], [1, 123, 1]]
    assert f3["dx"].shape == (98, 118) and f1["dx"].shape == (102, 122)
    t.match("the walk on ROI_IN", expect_path=2, ROI=ROI_IN)
    t.set(Nw=3)
    n3 = t.grid("Nw 3, widen=1", ROI=ROI_IN, widen=1)
    t.set(Nw=4)
    n4 = t.volume("Nw 4, cost_volume widen=1", ROI=ROI_IN, widen=1)
    t.grid("Nw 4, widen=3", ROI=ROI_IN, widen=3)
    assert _differ(n3, w1, "dx") and n4["region"].tolist() == [list(ROI_IN[0]), list(ROI_IN[1])]
    t.match("the walk on ROI_IN", expect_path=2, ROI=ROI_IN)
    t.update(ref=refB)
    r3 = t.basins("update_frames(ref), then basins widen=3 at once", k=3, ROI=ROI_IN, widen=3)
    t.update(ref=refA)
    t.grid("update_frames(ref), then widen=1 at once", ROI=ROI_IN, widen=1)
    r3a = t.basins("basins widen=3 on the first reference", k=3, ROI=ROI_IN, widen=3)
    assert _differ(r3, r3a, "dx")
    t.set(ROI=ROI_OUT)
    t.coarse_to_fine("coarse_to_fine over ROI_OUT", levels=(2, 1, 0), lam=kw["lam"], radius=kw["radius"])
    t.match("the walk afterwards", expect_path=2, ROI=ROI_IN)
    t.report()


# ----------------------------------------------------------------------------- C. table budget and chunk carry

def test_table_budget_and_chunk_carry_under_the_consumers(hip_ns, monkeypatch):
    """the 400 x 300 x 4 stack of test_table_budget_and_grid_consumer_on_one_model: one chunk under the default budget, four
    under 16 MB (a stepped ROI is computed on its dense grid, so it is chunked like the whole region); widen and scale_space
    then carry 2b rows from chunk to chunk"""
    from umpa_amd.synth import make_stack
    sam, ref, _ = make_stack(400, 300, 4, 4, df=True, seed=77, amplitude=1.5, order=1)
    monkeypatch.delenv("UMPA_HIP_TABLE_MB", raising=False)
    kw = _kw(hip_ns)
    t = LongLived(hip_ns, "UMPAModelDF", sam, ref, 3, 4, label="C budget")
    t.set(debug="ncalls")
    full = ((0, 386, 1), (0, 286, 1))
    thin = ((0, 386, 1), (0, 286, 3))
    coarse = ((0, 386, 4), (0, 286, 4))
    pdx, pdy = _priors(t, full)
    state = _state(hip_ns, t, thin)
    chunks, kept = {}, {}

    def five(tag, levels, device):
        kept[tag], seen = _launches(t.live, lambda: t.basins("basins, " + tag, k=2, ROI=full))
        chunks[tag] = [seen.get("table_consumer")]
        t.track(pdx, pdy, "track, " + tag, device=device, lam=kw["lam"], radius=kw["radius"], ROI=full)
        t.sequence("sequence with a state, " + tag, state=state, device=not device, lam=kw["lam"], trunc=kw["trunc"], ROI=thin)
        _, seen = _launches(t.live, lambda: t.volume("cost_volume widen=2, " + tag, ROI=coarse, widen=2))
        chunks[tag].append(seen.get("table_consumer"))
        _, seen = _launches(t.live, lambda: t.scale_space("scale_space %r, %s" % (levels, tag), levels=levels, tol=0.5, lam=kw["lam"],
                                                          radius=kw["radius"], ROI=full))
        chunks[tag].append(seen.get("table_consumer"))

    t.match("default budget: one chunk", expect_path=2, ROI=full)
    five("one chunk", (4, 2, 1, 0), False)
    monkeypatch.setenv("UMPA_HIP_TABLE_MB", "16")
    five("16 MB", (4, 2, 1, 0), True)
    t.match("the walk between the consumers, chunked", expect_path=2, ROI=full)
    t.scale_space("scale_space (8, 1), 16 MB", levels=(8, 1), tol=0.5, lam=kw["lam"], radius=kw["radius"], ROI=full)
    t.basins("basins on a stepped ROI, 16 MB", k=2, ROI=((17, 300, 2), (5, 280, 3)))
    monkeypatch.delenv("UMPA_HIP_TABLE_MB")
    five("default budget again", (8, 1), False)
    t.match("the walk afterwards", expect_path=2, ROI=full)
    print("\n[long-lived] C budget: table_consumer launches (basins, cost_volume widen=2, scale_space) %r" % (chunks,))
    assert chunks["one chunk"] == [1, 1, 1] and chunks["default budget again"] == [1, 1, 1], chunks
    assert all(n is not None and n > 1 for n in chunks["16 MB"]) and chunks["16 MB"][0] == 4, chunks
    # the answers do not depend on the chunking, and they do depend on the stack
    assert not _differ(kept["one chunk"], kept["16 MB"], "dx")
    t.update(sam=np.ascontiguousarray(sam[::-1]))
    other = t.basins("basins after update_frames(sam)", k=2, ROI=full)
    assert _differ(other, kept["one chunk"], "dx")
    t.report()


# ----------------------------------------------------------------------------- D. frames swapped under the consumers

@pytest.mark.parametrize("consumer", ["basins", "track", "sequence", "grid_widen", "scale_space", "resident"])
@pytest.mark.parametrize("cls", CLS)
def test_frames_swapped_under_the_consumers(hip_ns, cls, consumer):
    """the stacks, dark and flat of test_frames_swapped_under_the_caches.  The consumer is the FIRST reader of every staged
    stack: it adopts it and spends the one-shot bit.  uncertainty(resident=True) adopts through the match of its step; where
    a stack is staged and nothing has adopted it, it still reads the adopted one -- after one swap and after two."""
    samA, refA = _stack(5)
    samB, refB = _stack(9, amplitude=2.0)
    samC, _ = _stack(13)
    rng = np.random.default_rng(3)
    dark = 100.0 + rng.uniform(0, 2, size=samA.shape)
    flat = 20000.0 * (1.0 + 0.05 * rng.standard_normal(samA.shape))
    d_dark, d_flat = _device_frames(dark), _device_frames(flat)
    t = LongLived(hip_ns, cls, samA, refA, WS1, MS1, label="D swapped %s %s" % (consumer, cls))
    go = lambda what, roi=FULL, device=False: _run(hip_ns, t, consumer, roi, what, device=device)

    def pending(what):
        """(resident only) the walk, a staged stack that stays pending, and the maps of the stack adopted before it"""
        if consumer != "resident":
            return
        res = t.match("the walk before " + what, ROI=FULL)
        t.stage(np.ascontiguousarray(0.75 * samC))
        assert t.live._use_staged
        t.resident(dict(ROI=FULL), "staged and not adopted, " + what, result=res, pending=True)
        assert t.live._use_staged                                     # still pending: the next reader adopts it

    first = go("as built")
    t.update(sam=samB)
    after = go("update_frames(sam)")
    assert _differ(first, after, KEY[consumer])                       # (the stacks differ: a stale one would show)
    t.stage(np.ascontiguousarray(samA))
    back = go("first after stage_sample float64: one swap", device=True)
    assert not t.live._use_staged and not _differ(first, back, KEY[consumer])
    pending("after one swap")
    t.stage(_counts(samC, flat, dark), dark=d_dark, flat=d_flat)
    go("first after stage_sample uint16 with dark and flat")
    assert not t.live._use_staged
    pending("after the flat-corrected stack")
    t.stage(np.ascontiguousarray(samA))
    t.stage(np.ascontiguousarray(0.5 * samB))
    go("two stage_sample calls, the second wins")
    t.stage(np.ascontiguousarray(samC))
    t.update(sam=samB)
    assert not t.live._use_staged
    won = go("stage_sample, update_frames(sam): the update wins", device=True)
    assert not _differ(won, after, KEY[consumer])
    t.stage(_counts(samA, flat, dark), dark=d_dark, flat=d_flat)
    go("one more swap, on a ROI", ROI_IN)
    t.update(ref=refB)
    go("update_frames(ref), then a ROI the previous rectangle covers", ROI_IN)
    # (only match() carries F_REUSE_REF_MAPS: the other consumers compute the reference side anew and leave it to the walk)
    t.match("the walk on that ROI: the reference side is the consumer's", expect_path=2, ROI=ROI_IN)
    go("... then a ROI past the tiles just computed", ROI_OUT)
    t.match("the walk afterwards", ROI=FULL)
    t.report()


# ----------------------------------------------------------------------------- E. a masked model with the switch over time

@pytest.mark.parametrize("kind", ["binary", "weights"])
@pytest.mark.parametrize("cls", CLS)
def test_a_masked_model_with_the_switch_over_time(hip_ns, cls, kind):
    """the configuration and the masks of test_masked_models_on_the_tiled_path; unit steps only, within the masked step limit"""
    from umpa_amd import _lib
    H, W, K, Nw, ms = 120, 131, 3, 3, 4
    samA, refA = _stack(77, H, W, K, ms, 2.0)
    samB, refB = _stack(78, H, W, K, ms, 2.0)
    rng = np.random.default_rng(5)
    if kind == "binary":
        mask = (rng.random(samA.shape) < 0.9).astype(np.float64)
    else:
        mask = rng.uniform(0.0, 1.0, size=samA.shape) * (rng.random(samA.shape) < 0.95)
    full = ((0, H - 2 * (Nw + ms), 1), (0, W - 2 * (Nw + ms), 1))
    small, larger = ((40, 56, 1), (40, 60, 1)), ((10, 56, 1), (40, 100, 1))
    kw = _kw(hip_ns)
    t = LongLived(hip_ns, cls, samA, refA, Nw, ms, mask=mask, force=_lib.F_FORCE_TILED, label="E masked %s %s" % (cls, kind))
    go = lambda name, what, roi=full, device=False: _run(hip_ns, t, name, roi, what, device=device)
    w0 = t.match("the walk", expect_path=2, ROI=full)
    t.set_masked(True)
    go("grid", "switch on")
    go("volume", "switch on", small)
    b0 = go("basins", "switch on")
    assert b0["covered"].dtype == np.bool_ and b0["covered"].shape == b0["dx"].shape[1:]
    go("track", "switch on", device=True)
    go("sequence", "switch on")
    w1 = t.match("the walk again: the on-demand stages are back", expect_path=2, ROI=full)
    assert not _differ(w0, w1, "dx") and not _differ(w0, w1, "f")
    t.update(sam=samB)
    b1 = go("basins", "update_frames(sam)")
    assert _differ(b0, b1, "dx")
    go("sequence", "update_frames(sam)", device=True)
    t.update(ref=refB)
    go("track", "update_frames(ref), small ROI", small)
    go("track", "a larger ROI after the smaller one", larger)
    t.update(ref=refA)
    go("grid", "update_frames(ref), small ROI", small)
    go("basins", "a larger ROI after the smaller one", larger)
    t.set(Nw=2)
    go("sequence", "Nw 2, small ROI", small)
    go("volume", "Nw 2, a larger ROI", larger)
    t.match("Nw 2, the walk", expect_path=2, ROI=full)
    t.set_masked(False)
    today = "masked models are not supported (their table holds finished costs)"
    m = t.live
    for name, call in (("search='grid'", lambda: m.match(quiet=True, search="grid")), ("cost_volume", lambda: m.cost_volume(ROI=small)),
                       ("basins", lambda: m.basins(k=3)), ("track", lambda: m.track(0.0, 0.0, lam=kw["lam"], radius=kw["radius"])),
                       ("sequence", lambda: m.sequence(lam=kw["lam"], trunc=kw["trunc"]))):
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == "%s (grid search / cost volume): %s" % (name, today), name
    t.match("switch off: the walk", expect_path=2, ROI=full)
    t.set_masked(True)
    go("track", "switch on again")
    go("grid", "switch on again", larger)
    t.set(Nw=Nw)
    res = t.match("the constructor's window, the walk", expect_path=2, ROI=full)
    go("basins", "in front of the uncertainty maps", larger)
    after_consumer = t.resident(dict(ROI=full), "uncertainty(resident=True) after a consumer", result=res)
    after_walk = t.resident(dict(ROI=full), "uncertainty(resident=True) after the walk")
    assert not _differ(after_consumer, after_walk, "unit") and after_walk["valid"].any()
    t.report()


# ----------------------------------------------------------------------------- F. Tracker and Sequence used more than once

def _projections():
    return [np.ascontiguousarray(s) for s in (_stack(5)[0], _stack(9, amplitude=2.0)[0], _stack(13)[0], 0.5 * _stack(9, amplitude=2.0)[0])]


def _object_step(t, obj, raw, twin_call, what, need):
    """obj.step(raw) on the live model, against a fresh model that stages the same projection and makes `twin_call`"""
    res = obj.step(list(raw))
    assert all(v.is_cuda for k, v in res.items() if hasattr(v, "data_ptr")) and not t.live._use_staged
    t.rec["sam"] = ("staged", (raw, None, None))
    t._check(_download(res), t._path(t.live), t.live.ROI, lambda m: _download(twin_call(m)), what, need=need)
    return res


def test_sequence_object_used_more_than_once(hip_ns):
    from umpa_amd import Sequence
    P = _projections()
    kw = _kw(hip_ns)
    t = LongLived(hip_ns, "UMPAModelDF", P[0], _stack(5)[1], WS1, MS1, label="F Sequence")
    t.set(ROI=FULL)
    seq = Sequence(t.live, kw["lam"], trunc=kw["trunc"])
    need = t._fit() + ("state", "cost", "total", "cost0", "shift", "moved")
    host = lambda a: a.cpu().numpy()

    def step(p, what, starts=False):
        """starts: the object reads no state (a series starts); else the twin gets a host copy of the state the object holds"""
        prev = None if starts else host(seq.state)
        assert starts or seq.state is not None
        return _object_step(t, seq, P[p], lambda m: m.sequence(state=prev, lam=kw["lam"], trunc=kw["trunc"]), what, need)

    r1 = step(0, "a series starts", starts=True)
    keep1 = host(r1["state"])
    r2 = step(1, "second step")
    assert np.array_equal(host(r1["state"]), keep1, equal_nan=True)   # a returned state is unchanged by the next step ...
    keep2 = host(r2["state"])
    r3 = step(2, "third step")
    assert np.array_equal(host(r2["state"]), keep2, equal_nan=True)
    assert not np.array_equal(host(r1["state"]), keep1, equal_nan=True)                # ... and overwritten by the one after
    ptrs = [r["state"].data_ptr() for r in (r1, r2, r3)]
    assert ptrs[0] == ptrs[2] != ptrs[1]
    assert _differ(_download(r2), _download(r3), "dx")
    seq.reset()
    assert seq.state is None
    r4 = step(2, "after reset(): a series starts", starts=True)
    assert np.array_equal(host(r4["dx"]), t.grid("(the grid search of the same stack)")["dx"], equal_nan=True)
    r5 = step(3, "second step after reset()")
    ptrs += [r4["state"].data_ptr(), r5["state"].data_ptr()]
    assert len(set(ptrs)) == 2 and ptrs[3] != ptrs[4]                 # the two tensors were kept
    t.set(ROI=ROI_IN)
    r6 = step(0, "the model's ROI changed: new buffers, the state is dropped", starts=True)
    assert tuple(r6["state"].shape) == (7, 7, 16, 20)
    t.stage(P[2])
    t.match("a plain match on another staged stack, behind the object's back")
    r7 = step(1, "second step on the ROI, after that match")
    assert r6["state"].data_ptr() != r7["state"].data_ptr()
    t.set(ROI=FULL)
    r8 = step(3, "the ROI back: the state is dropped again", starts=True)
    r9 = step(2, "second step on the whole region")
    assert tuple(r9["state"].shape) == (7, 7) + (FULL[0][1], FULL[1][1]) and r8["state"].data_ptr() != r9["state"].data_ptr()
    t.report()


def test_tracker_object_used_more_than_once(hip_ns):
    """Tracker keeps its prior across a ROI change, where Sequence drops its state: the step is then refused by name (the
    projection it uploaded stays staged), and reset() starts anew"""
    from umpa_amd import Tracker
    P = _projections()
    kw = _kw(hip_ns)
    t = LongLived(hip_ns, "UMPAModelDF", P[0], _stack(5)[1], WS1, MS1, label="F Tracker")
    t.set(ROI=FULL)
    tr = Tracker(t.live, lam=kw["lam"], radius=kw["radius"])
    need = t._fit() + ("cost", "cost0", "shift", "count", "found")

    def step(p, what):
        if tr.prior is None:
            prior = [np.full(t.live.sh, np.nan)] * 2
        else:
            prior = [a.cpu().numpy() for a in tr.prior]
        return _object_step(t, tr, P[p], lambda m: m.track(prior[0], prior[1], lam=kw["lam"], radius=kw["radius"]), what, need)

    r1 = step(0, "the first step: the grid search")
    r2 = step(1, "second step")
    r3 = step(2, "third step")
    assert all(p.is_cuda for p in tr.prior) and _differ(_download(r2), _download(r3), "dx")
    tr.reset()
    assert tr.prior is None
    r4 = step(2, "after reset(): the grid search")
    assert np.array_equal(r4["dx"].cpu().numpy(), t.grid("(the grid search of the same stack)")["dx"], equal_nan=True)
    assert _differ(_download(r3), _download(r4), "dx")                 # (the prior of the third step told)
    step(3, "second step after reset()")
    t.set(ROI=ROI_IN)
    with pytest.raises(ValueError, match=r"track: a prior must be a scalar or of shape \(16, 20\), not \(104, 124\)"):
        tr.step(list(P[0]))
    assert t.live._use_staged                                         # uploaded, not adopted
    tr.reset()
    step(0, "the model's ROI changed, reset(): the grid search")
    t.stage(P[2])
    t.match("a plain match on another staged stack, behind the object's back")
    step(1, "second step on the ROI, after that match")
    t.set(ROI=FULL)
    tr.reset()
    step(3, "the ROI back, reset()")
    step(2, "second step on the whole region")
    assert r1["dx"].shape == (FULL[0][1], FULL[1][1])
    t.report()
