"""
Long-lived models: what the libraries remember between calls, against a fresh model.

A production run keeps one model alive for thousands of projections: frames are swapped under it (``update_frames``,
``stage_sample``), the region, the window, the coordinate convention and the table budget change, matches run
asynchronously, the grid search borrows the table.  Every one of these leans on state that survives a call -- the
reference-side maps and the tile rectangle they were computed for (``TiledState::ref_maps_ok`` / ``ref_rect``), the grow-only
map and table scratch, the two sample buffers and the descriptor lists that point into them, the two output sets, the
unwarp attachment, the streaming matcher's current reference.  A stale piece of it faults nothing: it returns plausible
maps computed from the wrong frames.

A trajectory here is a list of steps applied to ONE model; beside it the harness keeps a plain record of what the model
should now be.  After every match a fresh twin is built from that record, matched once with the same arguments under the
same environment, and the two results must be equal bit for bit, ``last_path`` included.  No tolerance appears in this file.

Every consumer of a live model is a step: ``match()`` (walk and grid search), ``cost_volume()``, ``smooth.match_smooth(model)``
and ``model.uncertainty(result)``.  Trajectories 9 to 13 put the later three behind staged, updated and rewritten stacks: a
staged stack is adopted by the FIRST call that reads the sample stack, whichever it is, and the last stack given wins.
The table's later consumers are steps of the harness too -- ``basins()``, ``track()``, ``sequence()``, ``widen=b`` on the grid
search, the volume, ``basins`` and ``track``, ``widen.coarse_to_fine``, ``levels.scale_space``, ``uncertainty(resident=True)`` --
and the ``masked_grid`` switch is a mutation of the record; their trajectories, and those of ``Tracker`` and ``Sequence``, are
in ``test_hip_longlived_consumers.py``.  The ``general_grid`` switch and the forced path are mutations of the record as well
(``set_general``, ``set_force``): the trajectories of the consumers on the general shift table are in
``test_hip_longlived_general.py``.  Where such a call takes HIP tensors (priors, states, ``out=``) the live model is given
tensors, the twin the same numbers as host arrays, and the downloaded maps are compared.

Each trajectory prints one line (steps compared, paths seen) for the record.
"""
import os
import re

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip_ns():
    from umpa_amd import _lib, model
    if _lib.hip().device_count() < 1:
        pytest.fail("no HIP device: the GPU tests cannot run (there is no CPU fallback)")
    return model


def _copy(res):
    return {k: np.array(v) for k, v in res.items() if isinstance(v, np.ndarray)}


def _download(res, prefix=""):
    """_copy for the table consumers' results: HIP tensors are downloaded, and `region` -- two (start, end, step) triples -- is
    kept as an int array, so that it is compared like a map"""
    out = {}
    for k, v in res.items():
        if k == "region":
            out[prefix + k] = np.array(v, dtype=np.int64)
        elif hasattr(v, "data_ptr"):
            out[prefix + k] = v.cpu().numpy()
        elif isinstance(v, np.ndarray):
            out[prefix + k] = np.array(v)
    return out


def _levels(pair):
    """(result, all) of coarse_to_fine / scale_space as one dictionary: `sel.<key>` and `L<n>.<key>`"""
    sel, every = pair
    out = _download(sel, "sel.")
    for n, r in enumerate(every):
        out.update(_download(r, "L%d." % n))
    return out


def _to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _device_frames(a):
    import torch
    return list(torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0"))


def _assert_same(got, want, need, what):
    """bit for bit, on every array both results carry; the arrays in `need` must be among them"""
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    assert set(need) <= set(got), (what, sorted(got))
    for k in sorted(got):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        if not np.array_equal(got[k], want[k], equal_nan=True):
            bad = ~((got[k] == want[k]) | ((got[k] != got[k]) & (want[k] != want[k])))
            first = tuple(int(x) for x in np.argwhere(bad)[0])
            raise AssertionError("%s: %s differs from the fresh model's at %d of %d elements, first at %r: %r != %r" % (
                what, k, int(bad.sum()), bad.size, first, got[k][first], want[k][first]))


def _frames(x):
    """a stack as the record keeps it: one array, or a list of arrays where the frames' shapes differ"""
    if isinstance(x, np.ndarray):
        return np.ascontiguousarray(x)
    x = [np.ascontiguousarray(f) for f in x]
    return np.ascontiguousarray(x) if len({f.shape for f in x}) == 1 else x


class LongLived:
    """One model that stays alive, and the record a fresh twin is built from.

    The record: model class, the sample stack -- a host array, or what was staged (raws, dark, flat: the twin stages the same
    into its own sample buffer, so no host arithmetic stands in for the flat-correction kernel) --, the reference stack,
    masks, positions, the window_size of the constructor (padding and extent are fixed there) and the Nw set since,
    assign_coordinates, sub_pixel_mode, debug, the ROI, the forced path and the attached unwarp map."""

    def __init__(self, hip_ns, cls, sam, ref, window_size, max_shift, mask=None, pos=None, force=0, label="", borrowed=False):
        """borrowed: the model borrows device frames (the planes of one tensor per stack), `write` rewrites them in place, and
        the twin is a fresh borrowed model on device copies of the record"""
        self.ns, self.label, self.borrowed = hip_ns, label or cls, borrowed
        self.rec = dict(cls=cls, sam=("host", _frames(sam)), ref=_frames(ref), mask=mask, pos=pos,
                        window_size=window_size, max_shift=max_shift, Nw=None, assign="sam", subpx=-1, debug=True, ROI=None,
                        force=force, unwarp=None, masked_grid=False, general_grid=False)
        self.adopted = self.rec["sam"]                                # the stack the library matches: a staged one is not, yet
        self.live = self._construct()
        self.steps, self.paths = 0, []

    # -- a model that has only ever been in the recorded state
    def _construct(self, sam=None):
        """sam: this sample-stack entry in place of the record's (the stack last adopted, while another is staged)"""
        r = self.rec if sam is None else dict(self.rec, sam=sam)
        kw = dict(window_size=r["window_size"], max_shift=r["max_shift"])
        if r["mask"] is not None:
            kw["mask_list"] = r["mask"]
        if r["pos"] is not None:
            kw["pos_list"] = [np.array(p) for p in r["pos"]]
        kind, payload = r["sam"]
        if self.borrowed:
            m = getattr(self.ns, r["cls"])(_device_frames(np.array(payload)), _device_frames(np.array(r["ref"])), **kw)
        else:
            blank = [np.zeros_like(f) for f in r["ref"]] if isinstance(r["ref"], list) else np.zeros_like(r["ref"])
            m = getattr(self.ns, r["cls"])(payload if kind == "host" else blank, r["ref"], **kw)
        m._force = r["force"]
        if r["Nw"] is not None:
            m.Nw = r["Nw"]
        m.assign_coordinates = r["assign"]
        m.sub_pixel_mode = r["subpx"]
        m.debug = r["debug"]
        if r["ROI"] is not None:
            m.ROI = r["ROI"]
        if r["masked_grid"]:
            m.masked_grid = True
        if r["general_grid"]:
            m.general_grid = True
        if kind == "staged":
            raw, dark, flat = payload
            if r["unwarp"] is not None:
                m.set_unwarp(r["unwarp"])
            m.stage_sample(list(raw), dark=dark, flat=flat)
        return m

    # -- mutations: the live model and the record together
    def set(self, **attrs):
        names = dict(Nw="Nw", assign="assign_coordinates", subpx="sub_pixel_mode", debug="debug", ROI="ROI")
        for k, v in attrs.items():
            setattr(self.live, names[k], v)
            self.rec[k] = v

    def set_masked(self, on):
        """the masked_grid switch of a model with masks"""
        self.live.masked_grid = on
        assert self.live.masked_grid is bool(on)
        self.rec["masked_grid"] = bool(on)

    def set_general(self, on):
        """the general_grid switch: the grid consumers of what no tiled path takes whole run on the general table"""
        self.live.general_grid = on
        assert self.live.general_grid is bool(on)
        self.rec["general_grid"] = bool(on)

    def set_force(self, flags):
        """the forced path (F_FORCE_DIRECT, F_FORCE_TILED, 0); the next consumer call re-derives the library's state from it"""
        self.live._force = flags
        self.rec["force"] = flags

    def update(self, sam=None, ref=None):
        self.live.update_frames(sam_list=sam, ref_list=ref)
        if sam is not None:
            self.rec["sam"] = self.adopted = ("host", _frames(sam))
        if ref is not None:
            self.rec["ref"] = _frames(ref)

    def stage(self, raw, dark=None, flat=None):
        """float64 raws without dark / flat and without a map are copied as they are: the twin is BUILT with them (exact);
        anything else goes through a kernel, and the twin stages the same raws into its own fresh model"""
        self.live.stage_sample(list(raw), dark=dark, flat=flat)
        plain = all(f.dtype == np.float64 for f in raw) and dark is None and flat is None and self.rec["unwarp"] is None
        self.rec["sam"] = ("host", _frames(raw)) if plain else ("staged", (raw, dark, flat))

    def write(self, sam=None, ref=None):
        """a borrowed model's stacks rewritten where they lie: the addresses stay, the contents change"""
        import torch
        for key, frames, new in (("sam", self.live._sam, sam), ("ref", self.live._ref, ref)):
            if new is not None:
                for d, x in zip(frames, new):
                    d.copy_(torch.from_numpy(np.array(x)))
                self.rec[key] = ("host", np.ascontiguousarray(new)) if key == "sam" else np.ascontiguousarray(new)
        torch.cuda.synchronize()

    def unwarp(self, umap):
        self.live.set_unwarp(umap)
        self.rec["unwarp"] = umap

    # -- matches: each against a twin that did only this call
    def _path(self, m):
        return m._lib.last_path(m._handle)

    def _check(self, got, path, roi, call, what, expect_path=None, need=None, pending=False):
        """got, path, roi: the live model's maps, last_path and ROI after its call; `call(twin)` makes the same call.
        pending: the live call read the sample stack without adopting a staged one, and so does the twin's: it is built from
        the stack adopted last"""
        twin = self._construct(self.adopted if pending else None)
        if not pending:
            self.adopted = self.rec["sam"]
        want = _copy(call(twin))
        self.steps += 1
        self.paths.append(path)
        tag = "%s, step %d (%s)" % (self.label, self.steps, what)
        assert path == self._path(twin), "%s: last_path %d, the fresh model's %d" % (tag, path, self._path(twin))
        if expect_path is not None:
            assert path == expect_path, "%s: last_path %d, expected %d" % (tag, path, expect_path)
        _assert_same(got, want, self._maps() if need is None else need, tag)
        assert roi == twin.ROI, "%s: ROI %r, the fresh model's %r" % (tag, roi, twin.ROI)
        self.rec["ROI"] = twin.ROI
        return got

    def _maps(self):
        need = ("f", "T", "dx", "dy", "err") + (("df",) if self.rec["cls"] == "UMPAModelDF" else ())
        return need + (("debug_Ncalls",) if self.rec["debug"] else ())

    def match(self, what="", expect_path=None, **kw):
        got = _copy(self.live.match(quiet=True, **kw))
        return self._check(got, self._path(self.live), self.live.ROI, lambda m: m.match(quiet=True, **kw), what or repr(kw), expect_path)

    def match_async_pair(self, kw_a, kw_b):
        """two asynchronous matches in flight (one per device output set), compared after their waits"""
        ra = self.live.match_async(quiet=True, **kw_a)
        pa, roi_a = self._path(self.live), self.live.ROI
        rb = self.live.match_async(quiet=True, **kw_b)
        pb, roi_b = self._path(self.live), self.live.ROI
        self.live.wait()
        self.live.wait()
        ga, gb = _copy(ra), _copy(rb)
        self._check(ga, pa, roi_a, lambda m: m.match(quiet=True, **kw_a), "async, first in flight %r" % (kw_a,))
        self._check(gb, pb, roi_b, lambda m: m.match(quiet=True, **kw_b), "async, second in flight %r" % (kw_b,))

    def cost_volume(self, **kw):
        got = _copy(self.live.cost_volume(**kw))
        return self._check(got, self._path(self.live), self.live.ROI, lambda m: m.cost_volume(**kw), "cost_volume %r" % (kw,),
                           need=("cost",) + (("T", "df") if kw.get("with_fit") else ()))

    def smooth(self, what="", **kw):
        """smooth.match_smooth(model, lam=..., trunc=..., **kw): the start field, its margin and valid, and the maps"""
        from umpa_amd import smooth
        assert "lam" in kw and "trunc" in kw                          # stated by the caller: no step depends on the defaults
        got = _copy(smooth.match_smooth(self.live, **kw))
        return self._check(got, self._path(self.live), self.live.ROI, lambda m: smooth.match_smooth(m, **kw),
                           what or "match_smooth %r" % (kw,), need=self._maps() + ("start", "margin", "valid"))

    def uncertainty(self, result_kw, what="", smooth_kw=None, sam=None, **kw):
        """model.uncertainty(model.match(**result_kw), **kw) -- or of smooth.match_smooth(model, **smooth_kw) --: unit, s2, dof,
        valid.  `sam`: the stack handed to the live model as sam=; the twin gets it only where its own stack was staged
        through a kernel too (a twin BUILT on the stack needs none: that is the comparison)."""
        from umpa_amd import smooth

        def call(m, sam_kw):
            res = m.match(quiet=True, **result_kw) if smooth_kw is None else smooth.match_smooth(m, **smooth_kw)
            u = m.uncertainty(res, **sam_kw, **kw)
            return {"unit": u.unit, "s2": u.s2, "dof": u.dof, "valid": u.valid}

        given = {} if sam is None else {"sam": sam}
        got = _copy(call(self.live, given))
        twin_kw = given if self.rec["sam"][0] == "staged" else {}
        return self._check(got, self._path(self.live), self.live.ROI, lambda m: call(m, twin_kw),
                           what or "uncertainty %r %r" % (result_kw if smooth_kw is None else smooth_kw, kw), need=("unit", "s2", "dof", "valid"))

    # -- the table's other consumers: basins, track, sequence, widening, the level chains, the resident uncertainty maps.
    #    Every call states lam, trunc and radius itself; with device=True the live model is given HIP tensors and its maps are
    #    downloaded, the twin is given the same numbers as host arrays.
    def _fit(self):
        return ("f", "T", "dx", "dy", "err") + (("df",) if self.rec["cls"] == "UMPAModelDF" else ())

    def _goes_general(self):
        """from the record alone: with general_grid on, a model that no tiled path takes whole -- masks that masked_grid does
        not admit, frames at different positions or of different shapes, a forced direct kernel"""
        from umpa_amd import _lib
        r = self.rec
        return r["general_grid"] and ((r["mask"] is not None and not r["masked_grid"]) or not self._one_box()
                                      or bool(r["force"] & _lib.F_FORCE_DIRECT))

    def _one_box(self):
        if isinstance(self.rec["ref"], list):                         # (_frames: a list where the shapes differ)
            return False
        return self.rec["pos"] is None or all(int(p[0]) == 0 and int(p[1]) == 0 for p in self.rec["pos"])

    def _extra(self, kw):
        """`region` of a widened call; `covered` of a masked model with the switch on, and of a model that goes the general
        way with a coverage that is not trivial (masks, or frames at different positions)"""
        covered = self.rec["masked_grid"] or (self._goes_general() and (self.rec["mask"] is not None or not self._one_box()))
        return (("region",) if kw.get("widen") else ()) + (("covered",) if covered else ())

    def grid(self, what="", expect_path=None, **kw):
        """match(search='grid', **kw), `region` of a widened call included"""
        got = _download(self.live.match(quiet=True, search="grid", **kw))
        return self._check(got, self._path(self.live), self.live.ROI, lambda m: _download(m.match(quiet=True, search="grid", **kw)),
                           what or "grid %r" % (kw,), expect_path, need=self._maps() + (("region",) if kw.get("widen") else ()))

    def volume(self, what="", **kw):
        """cost_volume(**kw), `region` and `covered` included"""
        got = _download(self.live.cost_volume(**kw))
        fit = ("T",) + (("df",) if self.rec["cls"] == "UMPAModelDF" else ()) if kw.get("with_fit") else ()
        return self._check(got, self._path(self.live), self.live.ROI, lambda m: _download(m.cost_volume(**kw)),
                           what or "cost_volume %r" % (kw,), need=("cost",) + fit + self._extra(kw))

    def basins(self, what="", **kw):
        assert "k" in kw
        got = _download(self.live.basins(**kw))
        return self._check(got, self._path(self.live), self.live.ROI, lambda m: _download(m.basins(**kw)),
                           what or "basins %r" % (kw,), need=self._fit() + ("cost", "shift", "count") + self._extra(kw))

    def track(self, prior_dx, prior_dy, what="", device=False, **kw):
        assert "lam" in kw and "radius" in kw
        given = [_to_device(p) if device and isinstance(p, np.ndarray) else p for p in (prior_dx, prior_dy)]
        res = self.live.track(given[0], given[1], **kw)
        assert hasattr(res["dx"], "data_ptr") == (device and any(isinstance(p, np.ndarray) for p in (prior_dx, prior_dy)))
        return self._check(_download(res), self._path(self.live), self.live.ROI, lambda m: _download(m.track(prior_dx, prior_dy, **kw)),
                           what or "track %r" % (kw,), need=self._fit() + ("cost", "cost0", "shift", "count", "found") + self._extra(kw))

    def sequence(self, what="", state=None, device=False, **kw):
        """state: a host array, or None where a series starts; the twin gets exactly it.  device=True: the live model reads a
        HIP copy of it and writes the next state into a tensor given as out="""
        assert "lam" in kw and "trunc" in kw
        if device:
            import torch
            _, _, N0, N1 = self.live._region(kw.get("ROI"), kw.get("step"), ROI_wins=True)
            U = 2 * self.rec["max_shift"] - 1
            out = torch.empty((U, U, N0, N1), dtype=torch.float64, device="cuda:0")
            res = self.live.sequence(state=None if state is None else _to_device(state), out=out, **kw)
            assert res["state"].data_ptr() == out.data_ptr() and res["dx"].is_cuda
        else:
            res = self.live.sequence(state=state, **kw)
        keys = self._fit() + ("state", "cost", "total", "cost0", "shift", "moved") + self._extra(kw)
        return self._check(_download(res), self._path(self.live), self.live.ROI, lambda m: _download(m.sequence(state=state, **kw)),
                           what or "sequence %r" % (kw,), need=keys)

    def coarse_to_fine(self, what="", **kw):
        """widen.coarse_to_fine(model, **kw) over the remembered ROI: every level's maps and regions"""
        from umpa_amd import widen
        assert "levels" in kw and "lam" in kw and "radius" in kw
        got = _levels(widen.coarse_to_fine(self.live, **kw))
        keys = tuple("%s.%s" % (p, k) for p in ["sel"] + ["L%d" % n for n in range(len(kw["levels"]))] for k in ("dx", "dy", "err", "region"))
        return self._check(got, self._path(self.live), self.live.ROI, lambda m: _levels(widen.coarse_to_fine(m, **kw)),
                           what or "coarse_to_fine %r" % (kw,), need=keys)

    def scale_space(self, what="", **kw):
        """levels.scale_space(model, **kw): the selected maps, `level` and `halfwidth`, and every level's maps and regions"""
        from umpa_amd import levels
        assert "levels" in kw and "tol" in kw and "lam" in kw and "radius" in kw
        got = _levels(levels.scale_space(self.live, **kw))
        keys = tuple("%s.%s" % (p, k) for p in ["sel"] + ["L%d" % n for n in range(len(kw["levels"]))] for k in ("dx", "dy", "err", "found", "region"))
        return self._check(got, self._path(self.live), self.live.ROI, lambda m: _levels(levels.scale_space(m, **kw)),
                           what or "scale_space %r" % (kw,), need=keys + ("sel.level", "sel.halfwidth"))

    def resident(self, result_kw, what="", result=None, pending=False, **kw):
        """model.uncertainty(res, resident=True, **kw) with res = model.match(**result_kw): unit, s2, dof, valid.  The twin is
        always one that adopted the same stack by the same route -- built on it, or staged through the kernel and adopted by
        its own match(**result_kw).  result: the maps of an earlier step with result_kw, and then the live model makes no
        match here: it reads the buffer as the calls before left it.  pending: a stack is staged and not adopted, the live
        call reads the one adopted before it, and the twin is a model of THAT stack (result is then required)."""
        assert not pending or result is not None

        def call(m, res):
            res = m.match(quiet=True, **result_kw) if res is None else res
            u = m.uncertainty(res, resident=True, **({} if res is not result else {"ROI": result_kw.get("ROI")}), **kw)
            return {"unit": u.unit, "s2": u.s2, "dof": u.dof, "valid": u.valid}

        got = _copy(call(self.live, result))
        return self._check(got, self._path(self.live), self.live.ROI, lambda m: call(m, None), what or "uncertainty(resident=True) %r %r" % (result_kw, kw),
                           need=("unit", "s2", "dof", "valid"), pending=pending)

    def report(self):
        print("\n[long-lived] %s: %d match steps compared, last_path values %s" % (self.label, self.steps, sorted(set(self.paths))))


# ----------------------------------------------------------------------------- the tiles a region needs

def _tile():
    """PrepCfg<NW>::T as the source has it"""
    tiled = open(os.path.join(REPO, "umpa_amd", "csrc", "umpa_tiled.h")).read()
    corr = open(os.path.join(REPO, "umpa_amd", "csrc", "umpa_corr.h")).read()
    assert re.search(r"struct PrepCfg \{\s*static constexpr int T = UMPA_TILE,", tiled), "PrepCfg<NW>::T is no longer UMPA_TILE"
    return int(re.search(r"#define UMPA_TILE (\d+)", corr).group(1))


def _prep_rect(H, W, NW, ms, pad, roi):
    """prep_rect (umpa_tiled.h) restated: the tiles (tx0, tx1, ty0, ty1) of the maps a region reads"""
    T = _tile()
    ntx, nty = (W - 2 * NW + T - 1) // T, (H - 2 * NW + T - 1) // T
    lo = lambda x: 0 if x - ms - NW < 0 else (x - ms - NW) // T
    hi = lambda x, n: min(n, max(0, (x + ms - NW) // T + 1))
    (a0, b0, s0), (a1, b1, s1) = roi
    last0, last1 = a0 + s0 * ((b0 - a0 - 1) // s0), a1 + s1 * ((b1 - a1 - 1) // s1)
    ty0 = min(lo(pad + a0), nty)
    tx0 = min(lo(pad + a1), ntx)
    return tx0, max(tx0, hi(pad + last1, ntx)), ty0, max(ty0, hi(pad + last0, nty))


# 120 x 140 frames, window_size 4, max_shift 4: padding 8, 104 x 124 output pixels; T = 32 gives 5 x 4 tiles at Nw = 4 and 3.
# The whole region reads tiles tx [0, 5) x ty [0, 4).
#   ROI_IN   output rows 40..55, columns 40..59  -> tx [1, 3) x ty [1, 2) at Nw = 4, tx [1, 3) x ty [1, 3) at Nw = 3, 2:
#            a strict subset of the tiles
#   ROI_OUT  output rows 10..55, columns 40..99  -> tx [1, 4) x ty [0, 2) at Nw = 4, tx [1, 4) x ty [0, 3) at Nw = 3, 2:
#            one tile row above and one tile column to the right of ROI_IN's rectangle (`covered` is false after ROI_IN)
H1, W1, K1, WS1, MS1 = 120, 140, 6, 4, 4
FULL = ((0, H1 - 2 * (WS1 + MS1), 1), (0, W1 - 2 * (WS1 + MS1), 1))
ROI_IN = ((40, 56, 1), (40, 60, 1))
ROI_OUT = ((10, 56, 1), (40, 100, 1))


def test_the_two_rois_sit_on_the_tiles_as_described():
    pad = WS1 + MS1
    want = {4: ((1, 3, 1, 2), (1, 4, 0, 2)), 3: ((1, 3, 1, 3), (1, 4, 0, 3)), 2: ((1, 3, 1, 3), (1, 4, 0, 3))}
    for NW in (4, 3, 2):
        full = _prep_rect(H1, W1, NW, MS1, pad, FULL)
        inner = _prep_rect(H1, W1, NW, MS1, pad, ROI_IN)
        outer = _prep_rect(H1, W1, NW, MS1, pad, ROI_OUT)
        assert full == (0, 5, 0, 4) and (inner, outer) == want[NW], (NW, full, inner, outer)
        assert full[0] < inner[0] and inner[1] < full[1] and full[2] < inner[2] and inner[3] < full[3]     # strictly inside
        assert outer[1] > inner[1] and outer[2] < inner[2]                                                  # past it on two sides


_stacks = {}


def _stack(seed, H=H1, W=W1, K=K1, ms=MS1, amplitude=1.5):
    key = (seed, H, W, K, ms, amplitude)
    if key not in _stacks:
        from umpa_amd.synth import make_stack
        sam, ref, _ = make_stack(H, W, K, ms, df=True, seed=seed, amplitude=amplitude)
        sam.setflags(write=False)
        ref.setflags(write=False)
        _stacks[key] = (sam, ref)
    return _stacks[key]


# ----------------------------------------------------------------------------- 1. the plain tiled path

@pytest.mark.parametrize("cls", ["UMPAModelDF", "UMPAModelNoDF"])
def test_plain_tiled_path_over_regions_modes_and_windows(hip_ns, cls):
    sam, ref = _stack(5)
    t = LongLived(hip_ns, cls, sam, ref, WS1, MS1, label="1 plain " + cls)
    t.match("whole region", expect_path=2, ROI=FULL)
    t.match("the same again: the reference side is reused", expect_path=2, ROI=FULL)
    t.match("interior ROI: a strict subset of the tiles", expect_path=2, ROI=ROI_IN)
    t.match("ROI past that rectangle on two sides", expect_path=2, ROI=ROI_OUT)
    t.match("whole region again", expect_path=2, ROI=FULL)
    t.set(ROI=None)
    t.match("step 2", step=2)
    t.match("stepped ROI", ROI=((3, 100, 2), (5, 120, 3)))
    t.set(assign="ref")
    t.match("reference coordinates", ROI=FULL)
    t.set(assign="sam")
    t.match("sample coordinates again", ROI=FULL)
    for subpx in (0, 1, -1):                                          # the modes of the goldens
        t.set(subpx=subpx)
        t.match("sub_pixel_mode %d" % subpx, ROI=ROI_OUT if subpx == 0 else FULL)
    t.match("start shifts", ROI=FULL, dxdy=(1, -1))
    for debug in ("ncalls", False, True):
        t.set(debug=debug)
        t.match("debug %r" % (debug,), ROI=ROI_IN if debug is False else FULL)
    # a new window drops every map: the interior ROI then fills its own tiles only, and the larger one finds maps of the
    # OLD window around them
    for nw in (3, 2, 4, 3):
        t.set(Nw=nw)
        t.match("Nw %d, interior ROI" % nw, expect_path=2, ROI=ROI_IN)
        t.match("Nw %d, ROI past it" % nw, expect_path=2, ROI=ROI_OUT)
    t.match("whole region at the last window", expect_path=2, ROI=FULL)
    t.report()


# ----------------------------------------------------------------------------- 2. frames swapped under the caches

def _counts(sam, flat, dark):
    return np.ascontiguousarray(np.clip(np.rint(sam * flat + dark), 0, 65535).astype(np.uint16))


@pytest.mark.parametrize("cls", ["UMPAModelDF", "UMPAModelNoDF"])
def test_frames_swapped_under_the_caches(hip_ns, cls):
    samA, refA = _stack(5)
    samB, refB = _stack(9, amplitude=2.0)
    samC, refC = _stack(13)
    rng = np.random.default_rng(3)
    dark = 100.0 + rng.uniform(0, 2, size=samA.shape)
    flat = 20000.0 * (1.0 + 0.05 * rng.standard_normal(samA.shape))
    d_dark, d_flat = _device_frames(dark), _device_frames(flat)
    t = LongLived(hip_ns, cls, samA, refA, WS1, MS1, label="2 swapped " + cls)
    t.match("as built", expect_path=2, ROI=FULL)
    t.update(sam=samB)
    t.match("update_frames(sam)", ROI=FULL)
    t.update(ref=refB)
    t.match("update_frames(ref)", ROI=FULL)
    t.update(sam=samC, ref=refC)
    t.match("update_frames(both)", ROI=FULL)
    t.stage(np.ascontiguousarray(samA))
    t.match("stage_sample float64: the back blob is the front buffer now", ROI=FULL)
    t.update(sam=samB)
    t.match("update_frames(sam) into the back blob", ROI=FULL)
    t.stage(_counts(samC, flat, dark), dark=d_dark, flat=d_flat)
    t.match("stage_sample uint16 with dark and flat", ROI=FULL)
    t.update(ref=refA)
    t.match("update_frames(ref), then a ROI the previous rectangle covers", expect_path=2, ROI=ROI_IN)
    t.match("... then a ROI past the tiles just computed", expect_path=2, ROI=ROI_OUT)
    t.stage(np.ascontiguousarray(samA))
    t.stage(np.ascontiguousarray(0.5 * samB))
    t.match("two stage_sample calls, the second wins", ROI=FULL)
    t.stage(_counts(samA, flat, dark), dark=d_dark, flat=d_flat)
    t.match("stage_sample, then a ROI", ROI=ROI_IN)
    t.match("... then the whole region", ROI=FULL)
    t.update(sam=samC)
    t.match("update_frames(sam) after an even number of swaps", ROI=FULL)
    t.report()


# ----------------------------------------------------------------------------- 3. asynchronous matches

def test_asynchronous_matches_in_both_output_sets(hip_ns):
    sam, ref = _stack(5)
    t = LongLived(hip_ns, "UMPAModelDF", sam, ref, WS1, MS1, label="3 async")
    t.match_async_pair(dict(ROI=FULL), dict(ROI=ROI_IN))              # set 0 sized by the whole region, set 1 by the ROI
    t.match_async_pair(dict(ROI=ROI_IN), dict(ROI=FULL))              # ... and the other way round
    t.match_async_pair(dict(ROI=ROI_OUT), dict(ROI=((3, 100, 2), (5, 120, 3))))
    t.match("synchronous afterwards", ROI=FULL)
    t.match("and a ROI", ROI=ROI_IN)
    t.report()


# ----------------------------------------------------------------------------- 4. masked models

@pytest.mark.parametrize("kind", ["binary", "weights"])
@pytest.mark.parametrize("cls", ["UMPAModelDF", "UMPAModelNoDF"])
def test_masked_models_on_the_tiled_path(hip_ns, cls, kind):
    """the 120 x 131, K = 3, Nw = 3, max_shift = 4 configuration of test_masked_models_against_the_oracle, path forced as there"""
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
    t = LongLived(hip_ns, cls, samA, refA, Nw, ms, mask=mask, force=_lib.F_FORCE_TILED, label="4 masked %s %s" % (cls, kind))
    t.match("as built", expect_path=2, ROI=full)
    t.match("the same again: nothing is prepared", expect_path=2, ROI=full)
    t.update(sam=samB)
    t.match("update_frames(sam)", expect_path=2, ROI=full)
    t.update(ref=refB)
    t.match("update_frames(ref)", expect_path=2, ROI=full)
    t.update(ref=refA)
    t.match("update_frames(ref), small ROI", expect_path=2, ROI=((40, 56, 1), (40, 60, 1)))
    t.match("a larger ROI after the smaller one", expect_path=2, ROI=((10, 56, 1), (40, 100, 1)))
    t.set(Nw=2)
    t.match("Nw 2, small ROI", expect_path=2, ROI=((40, 56, 1), (40, 60, 1)))
    t.match("Nw 2, whole region", expect_path=2, ROI=full)
    t.report()


# ----------------------------------------------------------------------------- 5. sample stepping

def test_sample_stepping_with_cached_subset_descriptors(hip_ns):
    """Three frames at (0, 0), (2, 1), (1, 3).  Frame k contributes to the output rows pi .. pi + H - 2 pad and columns
    pj .. pj + W - 2 pad (run_stepping_cells), so the rectangles of the region with a constant set of contributing frames
    are the centre (every frame: rows 2 .. H - 2 pad, columns 3 .. W - 2 pad) and strips one or two pixels wide around
    it; only those of 1024 pixels (UMPA_STEP_CELL_MIN) and more run on the tiled path, with a cached descriptor list of
    their subset.  The column strips beside the centre are H - 11 rows tall: column 0 (frame 0), columns 1..2 (frames 0, 1),
    column W - 9 (frames 1, 2) and column W - 8 (frame 2).  One-column strips of 1024 pixels take frames 1035 rows tall --
    taller than the other trajectories', and narrow instead (1040 x 24: fewer pixels than 160 x 180)."""
    H, W, K, Nw, ms = 1040, 24, 3, 2, 3
    pos = ((0, 0), (2, 1), (1, 3))
    pad = Nw + ms
    assert H - 2 * pad - 1 >= 1024                                    # rows 2 .. H - 2 pad of a one-column strip
    samA, refA = _stack(21, H, W, K, ms, 1.0)
    samB, refB = _stack(22, H, W, K, ms, 1.0)
    t = LongLived(hip_ns, "UMPAModelDF", samA, refA, Nw, ms, pos=pos, label="5 stepping")
    N0, N1 = t.live.extent
    assert (N0, N1) == (H + 2 - 2 * pad, W + 3 - 2 * pad)
    full = ((0, N0, 1), (0, N1, 1))
    inside = ((10, 1000, 1), (4, 14, 1))                              # within rows 2 .. H - 2 pad, columns 3 .. W - 2 pad: every frame
    # the first match, with the library's timers: the centre and the four strips each launch the table kernel
    import ctypes
    lib, h = t.live._lib, t.live._handle
    lib.timing_enable(h, 1)
    t.match("whole region", expect_path=4, ROI=full)
    seen = {}
    for q in range(lib.timing_collect(h)):
        nm, tot, cnt = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_int()
        lib.timing_read(h, q, ctypes.byref(nm), ctypes.byref(tot), ctypes.byref(cnt))
        seen[nm.value.decode()] = cnt.value
    lib.timing_enable(h, 0)
    assert seen.get("corr_volume", 0) == 5, sorted(seen.items())
    t.match("the same again: cached descriptor lists", expect_path=4, ROI=full)
    t.stage(np.ascontiguousarray(samB))
    t.match("stage_sample: the cached lists hold the old sample pointers", expect_path=4, ROI=full)
    t.update(ref=refB)
    t.match("update_frames(ref)", expect_path=4, ROI=full)
    t.match("a ROI every frame covers", expect_path=2, ROI=inside)
    t.match("the whole region: subset planes over the all-frames planes", expect_path=4, ROI=full)
    t.match("that ROI again", expect_path=2, ROI=inside)
    t.stage(np.ascontiguousarray(samA))
    t.match("stage_sample back into the first buffer", expect_path=4, ROI=full)
    t.report()


# ----------------------------------------------------------------------------- 6. the table and its consumer

def test_table_budget_and_grid_consumer_on_one_model(hip_ns, monkeypatch):
    """the 400 x 300 x 4 stack of test_stepped_and_chunked_tiled_path_matches_direct: 49 planes of 288 doubles per dense row,
    so 16 MB hold 128 rows and the 386 rows fall into four chunks -- under a table the default budget allocated whole"""
    from umpa_amd.synth import make_stack
    sam, ref, _ = make_stack(400, 300, 4, 4, df=True, seed=77, amplitude=1.5, order=1)
    monkeypatch.delenv("UMPA_HIP_TABLE_MB", raising=False)
    t = LongLived(hip_ns, "UMPAModelDF", sam, ref, 3, 4, label="6 table")
    t.set(debug="ncalls")
    full = ((0, 386, 1), (0, 286, 1))
    roi = ((17, 300, 2), (5, 280, 3))
    t.match("default budget: one chunk", expect_path=2, ROI=full)
    t.match("grid search, one chunk", expect_path=2, ROI=full, search="grid")
    monkeypatch.setenv("UMPA_HIP_TABLE_MB", "16")
    t.match("16 MB: four chunks under the larger table", expect_path=2, ROI=full)
    t.cost_volume(ROI=((100, 140, 1), (50, 90, 1)), with_fit=True)
    t.match("stepped ROI, chunked", expect_path=2, ROI=roi)
    t.match("grid search, four chunks", expect_path=2, ROI=full, search="grid")
    t.match("the walk after the consumer", expect_path=2, ROI=full)
    monkeypatch.delenv("UMPA_HIP_TABLE_MB")
    t.cost_volume(ROI=((0, 386, 4), (0, 286, 4)))
    t.match("default budget again", expect_path=2, ROI=full)
    t.match("grid search on a ROI", expect_path=2, ROI=roi, search="grid")
    t.report()


# ----------------------------------------------------------------------------- 7. the unwarp attachment over time

def test_unwarp_attachment_over_time(hip_ns):
    import test_hip_unwarp as TU
    import unwarp_expect as UE
    from umpa_amd import UnwarpMap
    refs, flats, dark, raws = TU.series()
    map_a = UnwarpMap(*UE.radial_map(TU.MH, TU.MW), interp="cubic")
    map_b = UnwarpMap(*UE.radial_map(TU.MH, TU.MW, amplitude=2.0, seed=11), interp="linear")
    d_dark, d_flat = _device_frames(dark), _device_frames(flats[0])
    t = LongLived(hip_ns, "UMPAModelDF", np.zeros_like(refs[0]), refs[0], TU.Nw, TU.MS, label="7 unwarp")
    t.unwarp(map_a)
    t.stage(raws[0], dark=d_dark, flat=d_flat)
    a0 = t.match("map A")
    t.unwarp(map_b)
    t.stage(raws[0], dark=d_dark, flat=d_flat)
    b0 = t.match("map B attached over A")
    t.unwarp(None)
    t.stage(raws[0], dark=d_dark, flat=d_flat)
    n0 = t.match("detached")
    t.unwarp(map_a)
    t.stage(raws[2], dark=d_dark, flat=d_flat)
    t.match("map A again, another projection")
    t.stage(raws[0], dark=d_dark, flat=d_flat)
    a1 = t.match("map A, the first projection again")
    # the three states are three different answers, so the comparisons above could tell them apart
    assert not np.array_equal(a0["dx"], b0["dx"]) and not np.array_equal(a0["dx"], n0["dx"]) and not np.array_equal(b0["dx"], n0["dx"])
    assert np.array_equal(a0["dx"], a1["dx"])
    t.report()


# ----------------------------------------------------------------------------- 8. StreamingMatcher used more than once

@pytest.mark.parametrize("unwarp", [False, True], ids=["plain", "unwarp"])
def test_streaming_matcher_used_more_than_once(hip_ns, unwarp):
    """Projection numbers 0, 1, 0.25, 0.75 against references acquired at 0 and 1: the nearest reference alternates, as the
    flats of the series do.  The second run is left at its first yield -- the hand-out before the first reference switch,
    with projection 1 staged and not yet adopted."""
    import test_hip_unwarp as TU
    import unwarp_expect as UE
    from umpa_amd import UnwarpMap
    from umpa_amd.farm import StreamingMatcher
    refs, flats, dark, raws = TU.series()
    ids = [0.0, 1.0, 0.25, 0.75]
    umap = UnwarpMap(*UE.radial_map(TU.MH, TU.MW), interp="cubic") if unwarp else None

    def matcher():
        return StreamingMatcher(refs, TU.Nw, TU.MS, df=True, device=0, flats=flats, dark=dark, ref_nums=[0, 1], unwarp=umap)

    def items():
        return ((ids[p], raws[p]) for p in range(4))

    sm = matcher()
    first = [(pid, _copy(res)) for pid, res in sm.run(items())]
    gen = sm.run(items())
    pid, _res = next(gen)
    assert pid == ids[0] and sm.model._use_staged                     # the next projection is staged, its match not enqueued
    gen.close()
    third = [(pid, _copy(res)) for pid, res in sm.run(items())]
    want = [(pid, _copy(res)) for pid, res in matcher().run(items())]
    assert [p for p, _ in first] == [p for p, _ in third] == [p for p, _ in want] == ids
    for run, what in ((first, "first run"), (third, "run after an abandoned one")):
        for (pid, got), (_, exp) in zip(run, want):
            assert exp["err"].mean() > 0.5
            _assert_same(got, exp, ("f", "T", "dx", "dy", "df", "err"), "8 streaming %s, projection %r" % (what, pid))
    assert not np.array_equal(want[0][1]["dx"], want[2][1]["dx"])     # (the projections differ: a mix-up would show)
    print("\n[long-lived] 8 streaming %s: %d projections compared" % ("unwarp" if unwarp else "plain", 2 * len(want)))


# ----------------------------------------------------------------------------- 9. a staged stack and whoever reads it first

_penalties = {}


def _smooth_kw(hip_ns):
    """lam and trunc for every match_smooth step of this file: 0.3 and 2.5 times cost_scale of the first stack's volume on
    ROI_IN (the factors of test_match_smooth), computed once"""
    if not _penalties:
        from umpa_amd import smooth
        sam, ref = _stack(5)
        m = hip_ns.UMPAModelDF(sam, ref, window_size=WS1, max_shift=MS1)
        unit = smooth.cost_scale(m.cost_volume(ROI=ROI_IN)["cost"])
        assert unit > 0
        _penalties.update(lam=0.3 * unit, trunc=2.5 * unit)
    return dict(_penalties)


def _consume(hip_ns, t, name, what):
    """the calls that read the sample stack besides the walk"""
    if name == "cost_volume":
        return t.cost_volume(ROI=ROI_IN)
    if name == "grid_search":
        return t.match("grid search, " + what, ROI=FULL, search="grid")
    return t.smooth("match_smooth, " + what, ROI=FULL, **_smooth_kw(hip_ns))


@pytest.mark.parametrize("consumer", ["cost_volume", "grid_search", "match_smooth"])
@pytest.mark.parametrize("raws", ["float64", "uint16"])
@pytest.mark.parametrize("cls", ["UMPAModelDF", "UMPAModelNoDF"])
def test_a_staged_stack_is_adopted_by_whoever_reads_the_sample_stack_first(hip_ns, cls, raws, consumer):
    """The consumer on a fresh live model: stage, the consumer, match(), the consumer again.  float64 raws
    without dark and flat are copied as they are, so the twin is BUILT on them; uint16 counts with dark and flat go through the
    flat-correction kernel, and the twin stages the same.  (Where cost_volume() does not adopt the staged stack, the first
    step of "cost_volume" and of "match_smooth" returns the constructor's stack's volume / start field.)"""
    samA, refA = _stack(5)
    samB, _ = _stack(9, amplitude=2.0)
    if raws == "uint16":
        rng = np.random.default_rng(3)
        dark = 100.0 + rng.uniform(0, 2, size=samA.shape)
        flat = 20000.0 * (1.0 + 0.05 * rng.standard_normal(samA.shape))
        staged = dict(raw=_counts(samB, flat, dark), dark=_device_frames(dark), flat=_device_frames(flat))
    else:
        staged = dict(raw=np.ascontiguousarray(samB))
    t = LongLived(hip_ns, cls, samA, refA, WS1, MS1, label="9 staged %s, %s first, %s" % (raws, consumer, cls))
    t.stage(**staged)
    _consume(hip_ns, t, consumer, "first after stage_sample")
    assert not t.live._use_staged                                     # adopted: the one-shot bit is spent
    t.match("the walk after it", ROI=FULL)
    _consume(hip_ns, t, consumer, "again")
    t.report()


# ----------------------------------------------------------------------------- 10. the last stack wins

@pytest.mark.parametrize("cls", ["UMPAModelDF", "UMPAModelNoDF"])
def test_the_last_stack_wins_between_stage_sample_and_update_frames(hip_ns, cls):
    from umpa_amd import _lib
    samA, refA = _stack(5)
    samB, refB = _stack(9, amplitude=2.0)
    samC, _ = _stack(13)
    t = LongLived(hip_ns, cls, samA, refA, WS1, MS1, label="10 last stack wins " + cls)
    t.match("as built", ROI=FULL)
    t.stage(np.ascontiguousarray(samB))
    t.update(sam=samC)                                                # the record's sample stack is samC now
    t.match("stage_sample, update_frames(sam): the update is the later stack", ROI=FULL)
    # the library's own rule, past the Python bookkeeping: the dropped stack cannot be asked for
    t.live._use_staged = True
    with pytest.raises(_lib.NativeError, match="UMPA_HIP_F_USE_STAGED without a staged sample stack"):
        t.live.match(quiet=True, ROI=FULL)
    assert not t.live._use_staged
    t.match("the same again after the refused flag", ROI=FULL)
    t.stage(np.ascontiguousarray(samA))
    t.match("one more stage_sample: a first swap, the dropped stack's buffer is overwritten", ROI=FULL)
    t.stage(np.ascontiguousarray(0.5 * samB))
    t.match("... and a second swap: the dropped stack does not come back", ROI=FULL)
    t.stage(np.ascontiguousarray(samB))
    t.update(ref=refB)                                                # the reference alone: the staged stack stays pending
    assert t.live._use_staged
    t.match("stage_sample, update_frames(ref): the staged stack with the new reference", ROI=FULL)
    t.stage(np.ascontiguousarray(samC))
    t.match("one more stage_sample", ROI=ROI_OUT)
    t.stage(np.ascontiguousarray(samB))
    t.update(sam=samA, ref=refA)
    t.cost_volume(ROI=ROI_IN)                                         # the same rule for the volume
    t.match("stage_sample, update_frames(both), cost_volume: the walk after them", ROI=FULL)
    t.report()


# ----------------------------------------------------------------------------- 11. uncertainty() over time

@pytest.mark.parametrize("cls", ["UMPAModelDF", "UMPAModelNoDF"])
def test_uncertainty_over_time(hip_ns, cls):
    samA, refA = _stack(5)
    samB, refB = _stack(9, amplitude=2.0)
    samC, refC = _stack(13)
    t = LongLived(hip_ns, cls, samA, refA, WS1, MS1, label="11 uncertainty " + cls)
    first = t.uncertainty(dict(ROI=FULL), "as built")
    assert first["valid"].mean() > 0.5                                # (the maps are there to be compared)
    t.update(sam=samB)
    after_sam = t.uncertainty(dict(ROI=FULL), "update_frames(sam)")
    assert not np.array_equal(after_sam["unit"], first["unit"], equal_nan=True)     # (the stacks differ: a stale one would show)
    t.update(ref=refB)
    t.uncertainty(dict(ROI=FULL), "update_frames(ref)")
    t.update(sam=samC, ref=refC)
    t.uncertainty(dict(ROI=FULL), "update_frames(both)")
    # the default region is the ROI the match left behind
    part = t.uncertainty(dict(ROI=ROI_IN), "default region after match(ROI=ROI_IN)")
    assert part["unit"].shape == (3, 16, 20)
    whole = t.uncertainty(dict(ROI=FULL), "default region after match(ROI=FULL)")
    assert whole["unit"].shape == (3,) + (FULL[0][1], FULL[1][1])
    t.uncertainty(None, "after match_smooth(ROI=ROI_OUT)", smooth_kw=dict(ROI=ROI_OUT, **_smooth_kw(hip_ns)))
    t.uncertainty(None, "after match_smooth on a stepped ROI", smooth_kw=dict(ROI=((3, 100, 2), (5, 120, 3)), **_smooth_kw(hip_ns)))
    # a narrower window is refused by name; back at the constructor's window the maps are a fresh model's
    t.set(Nw=3)
    res = t.match("Nw 3", ROI=FULL)
    with pytest.raises(RuntimeError, match="uncertainty: a window narrower than the one the model was built with is not supported"):
        t.live.uncertainty(res)
    t.set(Nw=WS1)
    t.uncertainty(dict(ROI=FULL), "Nw back at the constructor's window")
    t.report()


@pytest.mark.parametrize("cls", ["UMPAModelDF", "UMPAModelNoDF"])
def test_uncertainty_under_a_borrowed_stack_rewritten_in_place(hip_ns, cls):
    """the pattern of test_hip_borrowed.py::test_stacks_rewritten_in_place_under_one_borrowed_model: the frame addresses of the
    live model never change, their contents do; uncertainty() reads the planes where they lie"""
    from umpa_amd import sigma
    samA, refA = _stack(5)
    samB, refB = _stack(9, amplitude=2.0)
    t = LongLived(hip_ns, cls, samA, refA, WS1, MS1, label="12 uncertainty, borrowed " + cls, borrowed=True)
    base = t.live._sam[0].data_ptr()
    assert sigma._stack(t.live._sam).data_ptr() == base               # borrowed as it lies, not stacked into a copy
    first = t.uncertainty(dict(ROI=FULL), "as built")
    t.write(sam=samB)
    after_sam = t.uncertainty(dict(ROI=FULL), "sample stack overwritten in place")
    assert not np.array_equal(after_sam["unit"], first["unit"], equal_nan=True)
    t.write(ref=refB)
    t.uncertainty(dict(ROI=FULL), "reference stack overwritten in place")
    t.uncertainty(dict(ROI=ROI_IN), "a ROI")
    t.write(sam=samA, ref=refA)
    back = t.uncertainty(dict(ROI=FULL), "the first stacks again")
    _assert_same(back, first, ("unit", "s2", "dof", "valid"), "12 borrowed %s: the first data gives the first maps again" % cls)
    assert t.live._sam[0].data_ptr() == base
    t.report()


# ----------------------------------------------------------------------------- 13. uncertainty() after stage_sample

@pytest.mark.parametrize("cls", ["UMPAModelDF", "UMPAModelNoDF"])
def test_uncertainty_after_stage_sample_takes_the_stack_as_an_argument(hip_ns, cls):
    """The model keeps no host copy of a staged stack (it exists flat-corrected in the library's buffer only), so
    uncertainty() refuses by name until it is given the stack -- a host array or a HIP tensor -- or update_frames(sam_list=...)
    gives the model one again.  (Without the refusal the call reads the constructor's stack: finite maps of the wrong frames.)"""
    import torch
    from umpa_amd import sigma
    samA, refA = _stack(5)
    samB, _ = _stack(9, amplitude=2.0)
    samC, _ = _stack(13)
    refusal = re.escape("uncertainty: the sample stack was staged (stage_sample); pass it as sam=")
    t = LongLived(hip_ns, cls, samA, refA, WS1, MS1, label="13 uncertainty, staged " + cls)
    t.uncertainty(dict(ROI=FULL), "as built")
    t.stage(np.ascontiguousarray(samB))
    res = t.match("stage_sample float64", ROI=FULL)
    with pytest.raises(RuntimeError, match=refusal):
        t.live.uncertainty(res)
    on_host = t.uncertainty(dict(ROI=FULL), "sam= a host array, against a model built on it", sam=np.ascontiguousarray(samB))
    on_dev = t.uncertainty(dict(ROI=FULL), "sam= a HIP tensor", sam=torch.from_numpy(np.array(samB)).to("cuda:0"))
    _assert_same(on_dev, on_host, ("unit", "s2", "dof", "valid"), "13 %s: device and host sam=" % cls)
    # ... and the library call on the same shift field
    kind = int(cls == "UMPAModelDF")
    reg = (0, 1, FULL[0][1], 0, 1, FULL[1][1])
    direct = sigma.region(np.ascontiguousarray(samB), refA, t.live.window, MS1, kind, reg, sigma.shift_field(res, MS1))
    for k in ("unit", "s2", "dof"):
        assert np.array_equal(on_host[k], direct[k], equal_nan=True), k
    # the argument is checked by name
    with pytest.raises(ValueError, match=r"sam must be \[K, H, W\] = \(6, 120, 140\)"):
        t.live.uncertainty(res, sam=np.ascontiguousarray(samB[:, :-1]))
    with pytest.raises(ValueError, match=r"sam must be \[K, H, W\]"):
        t.live.uncertainty(res, sam=torch.zeros((K1 - 1, H1, W1), dtype=torch.float64, device="cuda:0"))
    with pytest.raises(ValueError, match="sam must be float64"):
        t.live.uncertainty(res, sam=samB.astype(np.float32))
    # a second staged stack, not adopted yet: still refused
    t.stage(np.ascontiguousarray(samA))
    with pytest.raises(RuntimeError, match=refusal):
        t.live.uncertainty(res)
    t.update(sam=samC)                                                # the model holds its sample stack again
    t.uncertainty(dict(ROI=FULL), "update_frames(sam) after stage_sample: no argument needed")
    # uint16 counts with dark and flat: the twin stages the same and is refused the same; both take the same sam=
    rng = np.random.default_rng(3)
    dark = 100.0 + rng.uniform(0, 2, size=samA.shape)
    flat = 20000.0 * (1.0 + 0.05 * rng.standard_normal(samA.shape))
    counts = _counts(samB, flat, dark)
    t.stage(counts, dark=_device_frames(dark), flat=_device_frames(flat))
    res = t.match("stage_sample uint16 with dark and flat", ROI=FULL)
    with pytest.raises(RuntimeError, match=refusal):
        t.live.uncertainty(res)
    t.uncertainty(dict(ROI=FULL), "sam= after a flat-corrected stage_sample", sam=(counts - dark) / flat)
    t.report()
