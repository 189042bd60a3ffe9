"""
The reference-side maps are reused by default for frames the model owns: umpa_hip_match_region through the raw C ABI, WITHOUT
UMPA_HIP_F_REUSE_REF_MAPS, once on host arrays and once on UMPA_HIP_F_DEVICE_IO tensors.

Frames of 45 x 61, Nw 2, max_shift 3: a region of 35 x 51, two tile rows and two tile columns with partial tiles on both
edges.  Three models: dark-field with 10 frames, no dark field with 3, dark-field with a 95 % mask.  Every match is compared
bit for bit (NaNs included) with the first match of a model created for the occasion on the same stacks, window and
coordinate mode.  On the masked model the tiled path reads only the reference means, so a match that reuses them launches
no prep_maps at all: there the launch count of umpa_hip_timing_read is asserted as well (results cannot show a reuse, by
design).  The models without masks always launch one prep_maps, for the sample side.
"""
import ctypes

import numpy as np
import pytest

from conftest import Case

pytestmark = pytest.mark.gpu

H, W, NW, MS = 45, 61, 2, 3
WHOLE = (0, 35, 0, 51)
ONE_TILE = (2, 12, 3, 15)                 # image rows and columns below 32 - max_shift + Nw: tile (0, 0) alone
MODELS = {"df": ("UMPAModelDF", 10, False), "nodf": ("UMPAModelNoDF", 3, False), "masked": ("UMPAModelDF", 10, True)}


@pytest.fixture(scope="module")
def hip_ns():
    from umpa_amd import _lib, model
    if _lib.hip().device_count() < 1:
        pytest.fail("no HIP device: the GPU tests cannot run (there is no CPU fallback)")
    return model


_stacks = {}


def _stack(name, seed):
    """(sam, ref) of a model's shape; seed 0 and 1 are two unrelated stacks"""
    from umpa_amd.synth import make_stack
    cls, K, _ = MODELS[name]
    key = (K, cls, seed)
    if key not in _stacks:
        sam, ref, _ = make_stack(H, W, K, MS, df=cls == "UMPAModelDF", seed=40 + seed, amplitude=1.2)
        _stacks[key] = (sam, ref)
    return _stacks[key]


def _mask(name):
    K = MODELS[name][1]
    return (np.random.default_rng(7).uniform(size=(K, H, W)) < 0.95).astype(np.float64) if MODELS[name][2] else None


def _window(power):
    """a separable window that is not the model's own for power != 1"""
    h = np.hamming(2 * NW + 1) ** power
    w = np.multiply.outer(h, h)
    return np.ascontiguousarray(w / w.sum())


class State:
    """What a model is made of at this moment: the stacks, the window, the coordinate mode."""

    def __init__(self, name, sam, ref, mask=None, pos=None, Nw=NW, ms=MS):
        self.name, self.sam, self.ref, self.mask, self.pos, self.Nw, self.ms = name, sam, ref, mask, pos, Nw, ms
        self.window, self.ref_shift = None, 0

    def build(self, hip_ns, borrowed=False):
        import torch
        conv = (lambda fr: None if fr is None else [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in fr]) if borrowed else (lambda fr: fr)
        kw = dict(window_size=self.Nw, max_shift=self.ms)
        if self.pos is not None:
            kw["pos_list"] = self.pos
        frames = (conv(self.sam), conv(self.ref), conv(self.mask))
        m = getattr(hip_ns, MODELS[self.name][0])(frames[0], frames[1], mask_list=frames[2], **kw)
        m._borrowed = frames                                          # (kept alive, and written in place by the borrowed test)
        lib, h = m._lib, m._handle
        if self.window is not None:
            lib.check(lib.set_window(h, self.window.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), self.Nw), "set_window")
        lib.check(lib.set_reference_shift(h, self.ref_shift), "set_reference_shift")
        lib.check(lib.timing_enable(h, 1), "timing_enable")
        return m


def _launches(m):
    lib, h = m._lib, m._handle
    out = {}
    for q in range(lib.timing_collect(h)):
        nm, tot, cnt = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_int()
        lib.timing_read(h, q, ctypes.byref(nm), ctypes.byref(tot), ctypes.byref(cnt))
        out[nm.value.decode()] = cnt.value
    return out


def _raw_match(m, io, region=None, flags=0):
    """umpa_hip_match_region as a C host calls it: ({map: host array}, launches per kernel, last_path)"""
    import torch
    from umpa_amd import _lib
    lib, h = m._lib, m._handle
    r0, r1, c0, c1 = region or (0, m.extent[0], 0, m.extent[1])
    N0, N1, nparam = r1 - r0, c1 - c0, m.Nparam
    if io == "device":
        dev = torch.device("cuda", torch.cuda.current_device())
        arrays = dict(values=torch.zeros((N0, N1, nparam), dtype=torch.float64, device=dev),
                      err=torch.zeros((N0, N1), dtype=torch.int32, device=dev), ncalls=torch.zeros((N0, N1), dtype=torch.int32, device=dev))
        ptr = {k: v.data_ptr() for k, v in arrays.items()}
        flags, stream = flags | _lib.F_DEVICE_IO, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    else:
        arrays = dict(values=np.zeros((N0, N1, nparam)), err=np.zeros((N0, N1), dtype=np.int32), ncalls=np.zeros((N0, N1), dtype=np.int32))
        ptr = {k: v.ctypes.data for k, v in arrays.items()}
        stream = None
    assert not flags & _lib.F_REUSE_REF_MAPS or getattr(m, "_vouched", False)
    rc = lib.match_region(h, r0, 1, N0, c0, 1, N1, ptr["values"], nparam, None, ptr["err"], None, 0.0, None, None, ptr["ncalls"], flags, stream)
    lib.check(rc, "match_region")
    if io == "device":
        torch.cuda.synchronize()
        arrays = {k: v.cpu().numpy() for k, v in arrays.items()}
    return arrays, _launches(m), lib.last_path(h)


def _same_bits(got, want, label):
    for k in want:
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), "%s: %s differs from a fresh model's" % (label, k)


class Live:
    """One long-lived model; every match is held to the first match of a fresh twin."""

    def __init__(self, hip_ns, state, io, borrowed=False):
        self.ns, self.state, self.io, self.borrowed = hip_ns, state, io, borrowed
        self.m = state.build(hip_ns, borrowed)
        self.counted = MODELS[state.name][2]                          # the masked model: a reuse launches no prep_maps

    def match(self, what, prep, region=WHOLE, flags=0, path=2):
        """`prep`: prep_maps launches of the masked model (None: equality only)"""
        label = "%s, %s arrays: %s" % (self.state.name, self.io, what)
        got, fam, p = _raw_match(self.m, self.io, region, flags)
        twin = self.state.build(self.ns, self.borrowed)
        want, fam_twin, p_twin = _raw_match(twin, self.io, region)
        assert p == p_twin and (path is None or p == path), (label, p, p_twin)
        assert np.isfinite(want["values"]).any() and (want["err"] == 1).any(), label
        _same_bits(got, want, label)
        if path == 2:
            assert fam_twin.get("prep_maps", 0) == 1, (label, fam_twin)   # a fresh model pays both sides
            if self.counted and prep is not None:
                assert fam.get("prep_maps", 0) == prep, (label, fam)
            elif not self.counted:
                assert fam.get("prep_maps", 0) == 1, (label, fam)         # the sample side, every time
        return got

    # what a C host does to a model between matches
    def update(self, sam=None, ref=None):
        from umpa_amd import _lib
        lib = self.m._lib
        fs = [None if a is None else _lib.FrameSet([np.ascontiguousarray(f) for f in a]) for a in (sam, ref)]
        lib.check(lib.update_frames(self.m._handle, fs[0].table if fs[0] else None, fs[1].table if fs[1] else None), "update_frames")
        if sam is not None:
            self.state.sam = sam
        if ref is not None:
            self.state.ref = ref

    def set_window(self, win):
        lib = self.m._lib
        lib.check(lib.set_window(self.m._handle, win.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), self.state.Nw), "set_window")
        self.state.window = win

    def set_reference_shift(self, v):
        self.m._lib.check(self.m._lib.set_reference_shift(self.m._handle, v), "set_reference_shift")
        self.state.ref_shift = v

    def stage(self, sam):
        lib = self.m._lib
        frames = [np.ascontiguousarray(f) for f in sam]
        table = (ctypes.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
        lib.check(lib.stage_sample(self.m._handle, table, 0, None, None), "stage_sample")
        self.state.sam = sam
        self._staged = frames                                         # (pageable memory: the upload has read it when the call returns; kept anyway)


@pytest.mark.parametrize("io", ["host", "device"])
@pytest.mark.parametrize("name", list(MODELS))
def test_a_models_life_without_the_flag(hip_ns, name, io):
    """match, match: 1, 0.  A new sample stack: 0.  A new reference stack: 1.  A new window: 1.  Whole region, one-tile ROI,
    whole region: 1, 0, 0 (a sample-only pass over fewer tiles leaves the covered rectangle alone).  A staged stack adopted
    with UMPA_HIP_F_USE_STAGED: 0.  The coordinate mode toggled: equality.  A fresh model, ROI then whole region: 1, 1."""
    from umpa_amd import _lib
    samA, refA = _stack(name, 0)
    samB, refB = _stack(name, 1)
    t = Live(hip_ns, State(name, samA, refA, _mask(name)), io)
    assert tuple(t.m.extent) == (WHOLE[1], WHOLE[3])
    first = t.match("the first match", 1)
    t.match("the same again", 0)
    t.update(sam=samB)
    moved = t.match("update_frames(sam)", 0)
    assert moved["values"].tobytes() != first["values"].tobytes()
    t.update(ref=refB)
    other = t.match("update_frames(ref)", 1)
    assert other["values"].tobytes() != moved["values"].tobytes()      # (stale reference maps would show)
    t.match("... and again", 0)
    t.set_window(_window(1.5))
    t.match("set_window", 1)
    t.update(ref=refA)
    t.match("whole region after a new reference", 1)
    t.match("a one-tile ROI", 0, region=ONE_TILE)
    t.match("the whole region after the ROI", 0)
    t.stage(samA)
    t.match("a staged stack, UMPA_HIP_F_USE_STAGED", 0, flags=_lib.F_USE_STAGED)
    t.set_reference_shift(1)
    t.match("reference coordinates", None)
    t.set_reference_shift(0)
    t.match("sample coordinates again", None)
    t.match("... twice", 0)

    u = Live(hip_ns, State(name, samA, refA, _mask(name)), io)
    u.match("fresh model: the ROI first", 1, region=ONE_TILE)
    u.match("fresh model: the whole region, which the ROI's tiles do not cover", 1)
    u.match("fresh model: the ROI again", 0, region=ONE_TILE)


@pytest.mark.parametrize("io", ["host", "device"])
def test_stepping_stacks_matched_twice(hip_ns, io):
    """The D_stepping golden stack (frames of unequal shapes at four positions) and the same frames cropped to one shape, which
    the tiled path takes in rectangles of frame subsets (last_path 4: each subset fills the map planes with its own frames and
    drops the record): two matches each, equal to a fresh model's."""
    c = Case("D_stepping")
    pos = [np.array(p) for p in c.pos]
    for what, crop, path in (("as recorded", None, None), ("cropped to 60 x 72", (60, 72), 4)):
        cut = (lambda fr: [np.ascontiguousarray(f) for f in fr]) if crop is None else (lambda fr: [np.ascontiguousarray(f[:crop[0], :crop[1]]) for f in fr])
        t = Live(hip_ns, State("df", cut(c.sam), cut(c.ref), pos=pos, Nw=c.Nw, ms=c.max_shift), io)
        region = (0, t.m.extent[0], 0, t.m.extent[1])
        for n in (1, 2, 3):
            t.match("D_stepping %s, match %d" % (what, n), None, region=region, path=path)


@pytest.mark.parametrize("name", list(MODELS))
def test_a_grid_consumer_called_twice(hip_ns, name):
    """umpa_grid_cost_volume (masked_grid on for the masked model) goes through the same decision: 1, 0, and the second
    volume is the first bit for bit; then a walk on the same model reuses what the consumer left: 0."""
    from umpa_amd import _lib
    sam, ref = _stack(name, 0)
    grid = _lib.grid()

    def volume(m):
        h, U = m._handle, 2 * MS - 1
        if MODELS[name][2]:
            grid.check(grid.set_masked(h, 1), "grid set_masked")
        cost = np.full((U, U, WHOLE[1], WHOLE[3]), -1.0)
        T = np.full_like(cost, -1.0)
        grid.check(grid.cost_volume(h, 0, 1, WHOLE[1], 0, 1, WHOLE[3], cost.ctypes.data, T.ctypes.data, None, 0, None), "grid cost_volume")
        return dict(cost=cost, T=T), _launches(m)

    state = State(name, sam, ref, _mask(name))
    live = state.build(hip_ns)
    want, fam0 = volume(state.build(hip_ns))
    assert np.isfinite(want["cost"]).any() and fam0.get("prep_maps", 0) == 1, fam0
    for n, prep in ((1, 1), (2, 0), (3, 0)):
        got, fam = volume(live)
        _same_bits(got, want, "%s cost volume %d" % (name, n))
        assert fam.get("prep_maps", 0) == (prep if MODELS[name][2] else 1), (name, n, fam)
    t = Live(hip_ns, state, "host")
    t.m = live
    t.match("a walk after the volumes", 0)


@pytest.mark.parametrize("name", list(MODELS))
def test_borrowed_frames_stay_opt_in(hip_ns, name):
    """Frames the model borrows (UMPA_HIP_F_DEVICE_FRAMES) can be overwritten behind the library's back: without the flag
    every match computes both sides (1, 1, with the reference tensors overwritten in place in between: the maps are those of
    a fresh model on the new reference); with the flag, the reference untouched, the second match reuses (0)."""
    import torch
    from umpa_amd import _lib
    samA, refA = _stack(name, 0)
    _, refB = _stack(name, 1)
    t = Live(hip_ns, State(name, samA, refA, _mask(name)), "device", borrowed=True)
    before = t.match("borrowed, as built", 1)
    for d, s in zip(t.m._borrowed[1], refB):
        d.copy_(torch.from_numpy(np.ascontiguousarray(s)))
    torch.cuda.synchronize()
    t.state.ref = refB
    after = t.match("borrowed, reference overwritten in place, no flag", 1)
    assert after["values"].tobytes() != before["values"].tobytes()
    t.match("borrowed, no flag, nothing changed: the library cannot know", 1)
    t.m._vouched = True
    t.match("borrowed, the owner vouches", 0, flags=_lib.F_REUSE_REF_MAPS)
    t.match("borrowed, a ROI with the flag", 0, region=ONE_TILE, flags=_lib.F_REUSE_REF_MAPS)
    t.match("borrowed, the whole region with the flag: still covered", 0, flags=_lib.F_REUSE_REF_MAPS)
