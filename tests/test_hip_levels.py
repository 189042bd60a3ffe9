"""
Scale-space search on the GPU: umpa_amd.levels.scale_space (umpa_grid_levels_track, libumpa_grid.so).  The main check is
equality bit for bit: every level of the one call against umpa_amd.widen.coarse_to_fine and against the chain of separate
track() calls, under every list of levels, table layout, row chunking, region, prior mode and input side; the selection
against the numpy statement of its rule applied to the device's own per-level maps.

REACHES names, per test, the levels kernels of libumpa_grid.so it is there for (tests/test_levels_cpu.py checks on the CPU
that every levels_* kernel symbol of the built library is claimed here, and that no claim is stale).
"""
import numpy as np
import pytest

import grid_expect as GE
import levels_expect as LE
from test_hip_widen import _chunk_stack, _launches, _model, _np

pytestmark = pytest.mark.gpu

REACHES = {
    "tests/test_hip_levels.py::test_every_level_subset_on_either_table_layout": LE.TABLE_KERNELS,
    "tests/test_hip_levels.py::test_levels_equal_coarse_to_fine": ["levels_prior_kernel"],
    "tests/test_hip_levels.py::test_selection_is_the_rule_on_the_device_maps": ["levels_select_kernel"],
}
NAN = float("nan")
INF = float("inf")


@pytest.fixture(scope="module")
def hip_ns():
    from umpa_amd import _lib, model
    if _lib.hip().device_count() < 1:
        pytest.fail("no HIP device: the GPU tests cannot run (there is no CPU fallback)")
    return model


def _levels_equal(every, want, levels, what, keys=None):
    """every level of scale_space's list against a list of separate results: equal on the level's own region, the values of
    a pixel without a basin in the rest of the call's region"""
    assert len(every) == len(want) == len(levels)
    for l, (got, exp, b) in enumerate(zip(every, want, levels)):
        names = [k for k in exp if k != "region" and k in got] if keys is None else keys
        assert len(names) >= 5 and {"dx", "dy", "f", "T", "err"} <= set(names), names
        for k in names:
            np.testing.assert_array_equal(LE.cut(_np(got[k]), got["region"], exp["region"]), _np(exp[k]),
                                          err_msg="%s: level %d (b %d) %s" % (what, l, b, k))
        ring = np.ones(_np(got["dx"]).shape, bool)
        LE.cut(ring, got["region"], exp["region"])[...] = False
        assert (_np(got["found"])[ring] == 0).all() and (_np(got["err"])[ring] == 0).all() and (_np(got["count"])[ring] == 0).all(), (what, l)
        for k in ("f", "T", "dx", "dy", "cost", "cost0") + (("df",) if "df" in got else ()):
            assert (_np(got[k])[ring] == 0).all(), (what, l, k)
        assert (_np(got["shift"])[:, ring] == 0).all(), (what, l)


def _same_call(a, b, what):
    """two results of scale_space, (selected, all), bit for bit"""
    for n, (x, y) in enumerate(zip([a[0]] + a[1], [b[0]] + b[1])):
        assert sorted(x) == sorted(y)
        for k in x:
            if k == "region":
                assert tuple(x[k]) == tuple(y[k]), (what, n)
            else:
                np.testing.assert_array_equal(_np(x[k]), _np(y[k]), err_msg="%s: result %d %s" % (what, n, k))


def _selection_holds(sel, every, levels, tol, what):
    from umpa_amd import levels as LV
    want = LV.select_levels(every, tol, levels=levels)
    assert sorted(want) == sorted(sel), (sorted(want), sorted(sel))
    for k in want:
        if k != "region":
            assert _np(sel[k]).dtype == want[k].dtype, k
            np.testing.assert_array_equal(_np(sel[k]), want[k], err_msg="%s: selected %s" % (what, k))
    return want


# ----------------------------------------------------------------------------- 1. the levels are coarse_to_fine's

@pytest.mark.parametrize("levels", [(4, 2, 1, 0), (8, 1), (2,), (4, 2, 0)], ids=str)
@pytest.mark.parametrize("kind", [0, 1], ids=["NoDF", "DF"])
def test_levels_equal_coarse_to_fine(hip_ns, kind, levels):
    from umpa_amd import levels as LV, widen
    sam, ref, c = GE.stack("64x72x3")
    for assign, subpx in (("sam", -1), ("ref", 1)):
        m = _model(hip_ns, kind, sam, ref, c["Nw"], c["ms"], assign, subpx)
        sel, every = LV.scale_space(m, levels=levels)
        assert all(tuple(r["region"]) == tuple(widen.valid_region(m, levels[-1])) for r in every + [sel])
        assert sorted(every[0]) == sorted(["f", "T", "dx", "dy", "cost", "cost0", "count", "found", "shift", "err", "region"] + (["df"] if kind else []))
        assert sorted(sel) == sorted(list(every[0]) + ["level", "halfwidth"])
        last, want = widen.coarse_to_fine(m, levels=levels)
        m.ROI = None
        # the first level of coarse_to_fine is a match() result: its maps are compared, the later ones have every key
        _levels_equal(every, want, levels, "%s subpx %d" % (assign, subpx))
        assert all(sorted(k for k in w if k in g) == sorted(w) for g, w in zip(every[1:], want[1:]))
        _levels_equal(every, LE.chain(m, levels), levels, "%s subpx %d, chain" % (assign, subpx), keys=[k for k in every[0] if k != "region"])


@pytest.mark.parametrize("levels", [(0,), (1, 0)], ids=str)
def test_lists_without_a_pooling_pass_or_with_a_single_one(hip_ns, levels):
    """the model's own window alone (no pooling, no lag, no carry) and one widened level above it (widen_table_kernel's pass)"""
    from umpa_amd import levels as LV
    sam, ref, c = GE.stack("64x72x3")
    for kind in (0, 1):
        m = _model(hip_ns, kind, sam, ref, c["Nw"], c["ms"], "sam", -1)
        (sel, every), seen = _launches(m, lambda: LV.scale_space(m, levels=levels, tol=0.5))
        assert seen.get("table_consumer") == 1 and seen.get("corr_volume") == 1, seen
        _levels_equal(every, LE.chain(m, levels), levels, str(levels), keys=[k for k in every[0] if k != "region"])
        _selection_holds(sel, every, levels, 0.5, str(levels))


# ----------------------------------------------------------------------------- 2. every pooling kernel

@pytest.mark.parametrize("strip", [False, True], ids=["plain", "strip-blocked"])
@pytest.mark.parametrize("levels", LE.SUBSETS, ids=str)
def test_every_level_subset_on_either_table_layout(hip_ns, levels, strip):
    from umpa_amd import levels as LV
    from umpa_amd.synth import make_stack
    if strip:
        sam, ref, _ = make_stack(66, 92, 3, 3, df=True, seed=77, order=1)
        m = _model(hip_ns, 1, sam, ref, 6, 3, "sam", 0)
    else:
        sam, ref, c = GE.stack("64x72x3")
        m = _model(hip_ns, 1, sam, ref, c["Nw"], c["ms"], "sam", 0)
    (sel, every), seen = _launches(m, lambda: LV.scale_space(m, levels=levels))
    assert ("corr_march" in seen) == strip and ("corr_volume" in seen) != strip and seen.get("table_consumer") == 1, seen
    _levels_equal(every, LE.chain(m, levels), levels, "%s strip %d" % (levels, strip), keys=[k for k in every[0] if k != "region"])
    assert (_np(every[-1]["found"]) >= 1).all()


# ----------------------------------------------------------------------------- 3. the selection

@pytest.mark.parametrize("tol", [0.0, 0.25, INF, (1.5, 0.5, 0.0, 7.0)], ids=str)
def test_selection_is_the_rule_on_the_device_maps(hip_ns, tol):
    from umpa_amd import levels as LV
    sam, ref, c = GE.stack("64x72x3")
    levels = (4, 2, 1, 0)
    seen = set()
    for kind, subpx in ((0, -1), (1, 1), (1, 0)):
        m = _model(hip_ns, kind, sam, ref, c["Nw"], c["ms"], "sam", subpx)
        sel, every = LV.scale_space(m, levels=levels, tol=tol)
        want = _selection_holds(sel, every, levels, tol, "kind %d subpx %d tol %s" % (kind, subpx, tol))
        dx, dy, err = (np.stack([_np(r[k]) for r in every]) for k in ("dx", "dy", "err"))
        np.testing.assert_array_equal(want["level"], LE.brute_select(dx, dy, err, LV.check_tol(tol, len(levels))))
        hw = np.asarray(levels + (-1,), np.int32)[_np(sel["level"])]
        np.testing.assert_array_equal(_np(sel["halfwidth"]), hw)
        seen |= set(np.unique(_np(sel["level"])).tolist())
    assert len(levels) - 1 in seen, seen


# ----------------------------------------------------------------------------- 4. one table pass

def test_one_table_pass(hip_ns):
    from umpa_amd import levels as LV, widen
    sam, ref, c = GE.stack("64x72x3")
    levels = (4, 2, 1, 0)
    m = _model(hip_ns, 1, sam, ref, c["Nw"], c["ms"])
    _, one = _launches(m, lambda: LV.scale_space(m, levels=levels))
    _, four = _launches(m, lambda: widen.coarse_to_fine(m, levels=levels))
    assert one.get("corr_volume") == 1 and one.get("table_consumer") == 1 and "replay_walk" not in one, one
    assert four.get("corr_volume") == 4 and four.get("table_consumer") == 4, four


# ----------------------------------------------------------------------------- 5. row chunks

@pytest.mark.parametrize("levels", [(8, 2, 0), (4, 1), (0,)], ids=str)
def test_row_chunks_change_nothing(hip_ns, monkeypatch, levels):
    from umpa_amd import levels as LV
    sam, ref = _chunk_stack()
    res = {}
    for mb in (None, "16"):
        if mb:
            monkeypatch.setenv("UMPA_HIP_TABLE_MB", mb)
        else:
            monkeypatch.delenv("UMPA_HIP_TABLE_MB", raising=False)
        m = _model(hip_ns, 1, sam, ref, 3, 5, subpx=-1)
        res[mb], seen = _launches(m, lambda: LV.scale_space(m, levels=levels, tol=0.5))
        assert seen.get("table_consumer") == (4 if mb else 1), (mb, seen)
    _same_call(res[None], res["16"], "four chunks")
    b = levels[-1]
    assert _np(res[None][0]["dx"]).shape == (128 - 2 * b, 512 - 2 * b)
    assert (_np(res[None][1][-1]["found"]) >= 1).all()


# ----------------------------------------------------------------------------- 6. regions, prior modes

def test_regions_are_slices_of_the_full_result(hip_ns):
    from umpa_amd import levels as LV, widen
    sam, ref, c = GE.stack("64x72x3")
    levels = (4, 1, 0)
    for kind in (0, 1):
        m = _model(hip_ns, kind, sam, ref, c["Nw"], c["ms"], subpx=-1)
        full = LV.scale_space(m, levels=levels, tol=0.5)
        N0, N1 = m.extent
        for region in (dict(step=2), dict(ROI=((5, N0 - 6, 2), (6, N1 - 7, 3))), dict(ROI=((0, 20, 1), (N1 - 9, N1, 1)))):
            part = LV.scale_space(m, levels=levels, tol=0.5, **region)
            assert tuple(part[0]["region"]) == tuple(widen.valid_region(m, levels[-1], **region))
            both = None
            for l, b in enumerate(levels):
                # where this level has numbers in both calls AND the same prior: the pixels every level so far keeps in the
                # smaller call (with steps its dense grid may end before the extent does; a level without a pixel leaves
                # the next one a NaN prior there, in coarse_to_fine as here)
                v = widen.valid_region(m, b, **region)
                both = v if both is None else tuple((max(p[0], q[0]), min(p[1], q[1]), p[2]) for p, q in zip(both, v))
                for k in part[1][l]:
                    if k != "region":
                        got = LE.cut(_np(part[1][l][k]), part[1][l]["region"], both)
                        s0, s1 = (slice(t[0] - f[0], t[1] - f[0], t[2]) for t, f in zip(both, full[1][l]["region"]))
                        np.testing.assert_array_equal(got, _np(full[1][l][k])[..., s0, s1], err_msg="%s level %d %s" % (region, l, k))
            _selection_holds(part[0], part[1], levels, 0.5, str(region))


def test_prior_modes_are_forwarded(hip_ns):
    from umpa_amd import levels as LV
    sam, ref, c = GE.stack("64x72x3")
    levels = (4, 2, 0)
    for kind in (0, 1):
        m = _model(hip_ns, kind, sam, ref, c["Nw"], c["ms"], subpx=-1)
        for lam, radius in ((0.02, 4.0), (None, 1.5), (0.3, None)):
            sel, every = LV.scale_space(m, levels=levels, lam=lam, radius=radius)
            _levels_equal(every, LE.chain(m, levels, lam=lam, radius=radius), levels, "lam %r radius %r" % (lam, radius),
                          keys=[k for k in every[0] if k != "region"])


# ----------------------------------------------------------------------------- 7. special pixels

@pytest.mark.parametrize("bad", ["nan", "+inf", "zero"])
@pytest.mark.parametrize("where", ["sam", "ref"])
def test_special_pixels(hip_ns, bad, where):
    import regimes
    from umpa_amd import levels as LV
    sam, ref, c = GE.stack("64x72x3")
    ms, Nw = c["ms"], c["Nw"]
    cfg = dict(H=c["H"], W=c["W"], K=c["K"], Nw=Nw, ms=ms)
    pos = [p for p in regimes.bad_positions(cfg) if p[1] < c["H"] and p[2] < c["W"]]
    assert len(pos) >= 3
    sam, ref = regimes.bad_pixels(sam, ref, bad, where, pos)
    levels = (4, 1, 0)
    for kind in (0, 1):
        m = _model(hip_ns, kind, sam, ref, Nw, ms, subpx=-1)
        sel, every = LV.scale_space(m, levels=levels)
        # each level's footprint of the bad pixels is the sibling's: the chain of separate calls, NaN for NaN
        _levels_equal(every, LE.chain(m, levels), levels, "%s in %s" % (bad, where), keys=[k for k in every[0] if k != "region"])
        want = _selection_holds(sel, every, levels, None, "%s in %s" % (bad, where))
        ok = [(_np(r["err"]) == 1) & np.isfinite(_np(r["dx"])) & np.isfinite(_np(r["dy"])) for r in every]
        level = _np(sel["level"])
        # no tolerance: the narrowest level that matched, whatever the wider ones did
        expect = np.full(level.shape, -1)
        for l in range(len(levels)):
            expect[ok[l]] = l
        np.testing.assert_array_equal(level, expect)
        if bad != "zero" and where == "sam":
            inner = np.zeros(level.shape, bool)
            inner[4:-4, 4:-4] = True                                  # (where the widest level's window fits)
            # around a hole the wide windows fail first: pixels the last level still matches and the widest does not, and
            # the hole itself, which no level matches
            assert (inner & ~ok[0] & (level == len(levels) - 1)).any() and (level == -1).any()
            assert (_np(every[-1]["found"])[level == -1] == 0).any()


# ----------------------------------------------------------------------------- 8. repeats, HIP tensors on a side stream

def test_repeats_and_device_models_on_a_side_stream(hip_ns):
    import torch
    from umpa_amd import levels as LV
    sam, ref, c = GE.stack("64x72x3")
    levels = (4, 2, 1, 0)
    for kind in (0, 1):
        m = _model(hip_ns, kind, sam, ref, c["Nw"], c["ms"], subpx=-1)
        host = LV.scale_space(m, levels=levels, tol=0.25)
        assert not hasattr(host[0]["dx"], "data_ptr")
        _same_call(LV.scale_space(m, levels=levels, tol=0.25), host, "second call")
        dev = torch.device("cuda", m._device)
        ts, tr = ([torch.as_tensor(np.ascontiguousarray(f), device=dev) for f in s] for s in (sam, ref))
        md = _model(hip_ns, kind, ts, tr, c["Nw"], c["ms"], subpx=-1)
        on_dev = LV.scale_space(md, levels=levels, tol=0.25)
        stream = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(stream):
            side = LV.scale_space(md, levels=levels, tol=0.25)
        stream.synchronize()
        assert all(hasattr(r["dx"], "data_ptr") and hasattr(r["err"], "data_ptr") for r in [on_dev[0], side[0]] + on_dev[1] + side[1])
        _same_call(on_dev, host, "HIP-tensor model")
        _same_call(side, host, "HIP-tensor model on a side stream")


# ----------------------------------------------------------------------------- 9. the use case

def test_the_use_case_returns_the_true_shift_at_the_narrowest_level(hip_ns):
    from umpa_amd import levels as LV
    u, sam, ref, known, sure = LE.use_case()
    ty, tx = u["true"]
    levels = LE.USE_LEVELS
    m = _model(hip_ns, 0, sam, ref, u["Nw"], u["ms"], "sam", 0)       # sub-pixel mode 0: dx, dy are the integer shifts
    assert sure.shape == tuple(m.extent)
    sel, every = LV.scale_space(m, levels=levels, tol=0.0)
    print("use: %d of %d pixels are sure at every level, %d of them among the %d known" % (sure.sum(), sure.size, (sure & known).sum(), known.sum()))
    assert sure.any() and (sure & known).any()
    np.testing.assert_array_equal(sel["dy"][sure], ty)
    np.testing.assert_array_equal(sel["dx"][sure], tx)
    np.testing.assert_array_equal(sel["halfwidth"][sure], min(levels))
    np.testing.assert_array_equal(sel["level"][sure], len(levels) - 1)
    # the plain grid search takes the alias at the known pixels: the scale space is what finds the true shift there
    plain = m.match(quiet=True, search="grid")
    np.testing.assert_array_equal(plain["dx"][known], tx - u["period"])
