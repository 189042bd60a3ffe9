"""
Borrowed device frames (UMPA_HIP_F_DEVICE_FRAMES) and device outputs (UMPA_HIP_F_DEVICE_IO) on every matching path.

The rest of the suite builds its models from host arrays and reads host arrays back; the sharded matcher, the multi-GPU
benchmark leg and KernelSearch run on the other interface.  What differs there is host logic and addresses, not arithmetic,
so every comparison in this file is bit for bit -- against the same match of a model that owns its frames, against the same
model in another memory layout, against a fresh model -- with one exception, the sample-stepping slivers (a. below).

The frames and the output arrays live inside larger tensors of the test's own (tests/guarded.py): a read of the bytes around
a frame changes a result (the guards hold NaN, or 1e300), a store outside an array changes a guard, a store into the stack
changes a frame, and all three are seen as DATA.  Nothing here relies on a fault or can cause one: the guards are at least two
rows and a wavefront long.

 a. borrowed = owned, on the twenty configurations of tests/regimes.py (CONFIGS and STEPPING_EXTRA);
 b. four layouts of the borrowed stack (tight, NaN guards, 1e300 guards, odd element offsets: bases at 8 mod 16) give one
    result, and no match writes to the stack or the guards;
 c. device outputs between canaries, interleaved and planar, owned and borrowed, ROIs, a coverage map that skips pixels,
    row pieces with a callback;
 d. one borrowed model whose stacks change in place, step by step against a fresh model.
"""
import ctypes

import numpy as np
import pytest

import guarded as G
import regimes as R
from conftest import assert_parity

pytestmark = pytest.mark.gpu

ALL = list(R.CONFIGS) + list(R.STEPPING_EXTRA)
MAPS = ("err", "debug_Ncalls", "f", "T", "dx", "dy", "df", "debug_d", "debug_a")


@pytest.fixture(scope="module")
def ns():
    from umpa_amd import _lib, model
    from oracle import cpu_model
    if _lib.hip().device_count() < 1:
        pytest.fail("no HIP device: the GPU tests cannot run (there is no CPU fallback)")
    return model, cpu_model.port


def _host(name):
    sam, ref = R.base_stack(name)
    return sam, ref, R.mask_of(name)


def _same(a, b, what, sel=None):
    for k in MAPS:
        assert (k in a) == (k in b), (what, k)
        if k not in a:
            continue
        x, y = (a[k], b[k]) if sel is None else (a[k][:, sel], b[k][:, sel])
        if not np.array_equal(x, y, equal_nan=True):
            bad = ~((x == y) | (np.isnan(x) & np.isnan(y)))
            first = tuple(int(v) for v in np.argwhere(bad)[0])
            raise AssertionError("%s: %s differs on %d of %d entries, first at %r: %r != %r" % (what, k, int(bad.sum()), bad.size, first, x[first], y[first]))


def _copy(res):
    return {k: np.array(v) for k, v in res.items() if isinstance(v, np.ndarray)}


# ----------------------------------------------------------------------------- layouts of a borrowed stack

LAYOUTS = ("nan", "tight", "1e300", "odd")


def _embed(name, layout, stacks=None):
    """The frames of a configuration (sample, reference, masks: 2 K or 3 K frames) inside ONE device tensor.
    tight: back to back, as the rows of a sharding slab -- the bytes after a frame are the next frame's first row;
    nan / 1e300: guards of 2 W + 64 elements between the frames; odd: guards of 2 W + 65, so that the bases of consecutive
    frames (H W is even in every configuration) alternate between 8 and 0 mod 16."""
    cfg = R.config(name)
    sam, ref, mask = _host(name) if stacks is None else stacks
    K, W = cfg["K"], cfg["W"]
    assert cfg["H"] * W % 2 == 0
    g = G.min_guard(W)
    frames = list(sam) + list(ref) + (list(mask) if mask is not None else [])
    guard, fill = {"nan": (g, G.NAN_BITS), "tight": (0, G.NAN_BITS), "1e300": (g, G.BIG_BITS), "odd": (g + 1, G.NAN_BITS)}[layout]
    views, h = G.embed(frames, guard, fill, device="cuda:0", tail=g + (1 if layout == "odd" else 0))
    if layout == "odd":
        assert [v.data_ptr() % 16 for v in views[:4]] == [8, 0, 8, 0]
    elif layout == "tight":
        assert views[1].data_ptr() == views[0].data_ptr() + 8 * sam[0].size
        assert views[K].data_ptr() == views[K - 1].data_ptr() + 8 * sam[0].size       # the reference stack follows the last sample row
    else:
        assert all(v.data_ptr() % 16 == 0 for v in views)
    return views[:K], views[K:2 * K], (views[2 * K:] if mask is not None else None), h


_OWNED, _BORROWED = {}, {}


def _owned(ns, name):
    """The configuration matched by a model that owns copies of the host arrays (once per module run)"""
    if name not in _OWNED:
        sam, ref, mask = _host(name)
        m = R.build(ns[0], name, sam, ref, mask=mask)
        _OWNED[name] = (_copy(R.match(m, name, timing=True)), m.launch_counts)
    return _OWNED[name]


def _borrowed(ns, name, layout="nan"):
    if (name, layout) not in _BORROWED:
        s, r, k, h = _embed(name, layout)
        m = R.build(ns[0], name, s, r, mask=k)
        out = _copy(R.match(m, name, timing=True))
        G.check(h, "%s, %s layout: the borrowed stack after a match" % (name, layout))
        _BORROWED[(name, layout)] = (out, m.launch_counts)
    return _BORROWED[(name, layout)]


# ----------------------------------------------------------------------------- sample stepping: which columns may differ

def _region(cfg):
    """(org, step, N) per axis of the configuration's match, from the extent and its ROI / step"""
    pad = R.padding(cfg)
    pos = cfg.get("pos") or [(0, 0)]
    ext = [max(p[a] for p in pos) + cfg["H" if a == 0 else "W"] - 2 * pad for a in (0, 1)]
    mk = cfg.get("mk", {})
    roi = mk.get("ROI") or tuple((0, e, mk.get("step", 1)) for e in ext)
    return [(pad + s, t, 1 + (e - s - 1) // t) for (s, e, t) in roi]


def sliver_columns(cfg):
    """Frame k contributes to the image columns pj + padding .. pj + W - padding (Model.cpp:428-433).  At the last of them a
    window at the largest column shift reads the frame's last column, which corr_volume would stage as the FIRST half of a
    16-byte pair: a model that borrows its frames (no readable bytes promised behind a row) leaves that output column to the
    general kernel, a model that owns them lets the table kernel have it.  From pos, W and the padding alone: the region
    columns that are image column pj + W - padding of some frame -- one per distinct column position at the most."""
    pad, W = R.padding(cfg), cfg["W"]
    (_, _, _), (org, step, N) = _region(cfg)
    cols = set()
    for (_, pj) in cfg["pos"]:
        q, rem = divmod(pj + W - pad - org, step)
        if rem == 0 and 0 <= q < N:
            cols.add(q)
    assert len(cols) <= len({pj for (_, pj) in cfg["pos"]})
    return sorted(cols)


def test_sliver_columns_of_the_stepping_configurations():
    """stepping_DF and its two siblings: frames at columns 0 and 9, W = 140, padding 6: image columns 134 and 143 = region
    columns 128 and 137, the second past the region's 137 columns.  stepping_s2: image columns 185 and 225, the region
    starts at image column 5 with step 2: columns 90 and 110, the second past its 109."""
    for name in ("stepping_DF", "stepping_mask_DF", "stepping_NoDF"):
        assert sliver_columns(R.config(name)) == [128] and _region(R.config(name))[1] == (6, 1, 137)
    assert sliver_columns(R.config("stepping_s2")) == [90] and _region(R.config("stepping_s2")) == [(8, 2, 86), (5, 2, 109)]


# ----------------------------------------------------------------------------- a. borrowed = owned

@pytest.mark.parametrize("name", ALL)
def test_borrowed_equals_owned(ns, name):
    """The same data as device tensors between NaN guards and as host arrays: one last_path (R.match asserts the
    configuration's on both), the kernel the configuration is named after launched by both, every map equal bit for bit.

    Sample stepping without masks: the borrowed model's last contributing column of a frame (sliver_columns) runs on the
    general kernel, the owning model's on the table kernel (pair_slack, umpa_hip.hip; `cs[k]` in run_stepping_cells); there
    both are held to the CPU oracle by the suite's bar instead, the rest of the region stays bit for bit.  With masks
    pair_slack is false for both models (corr_masked keeps its own column clamp): bit for bit everywhere.
    0/1 masks: the owning model detects them and takes corr_masked's one-multiply pair weight (mask_binary), the borrowed
    one the general weight; the two agree to the last bit, which masked_bin_* and stepping_mask_DF assert here."""
    cfg = R.config(name)
    own, own_launch = _owned(ns, name)
    bor, bor_launch = _borrowed(ns, name)
    for launched in (own_launch, bor_launch):
        assert cfg.get("launch") is None or cfg["launch"] in launched, launched
    assert (own["err"] == 1).sum() > 500
    if not cfg.get("pos"):
        _same(bor, own, name + ": borrowed against owned")
        assert own_launch == bor_launch, (own_launch, bor_launch)
        return
    table = "corr_masked" if cfg.get("mask") else "corr_volume"
    assert own_launch.get(table, 0) >= 1 and bor_launch.get(table, 0) >= 1, (own_launch, bor_launch)
    cols = sliver_columns(cfg)
    assert cols, "the configuration was chosen to have a sliver column"
    # the general kernels run once per rectangle they are given: the borrowed model, without masks, gives them one more per
    # sliver column (full height); with masks both models cut the same rectangles
    general = lambda launched: launched.get("match_direct", 0) + launched.get("match_staged", 0)
    assert general(bor_launch) == general(own_launch) + (0 if cfg.get("mask") else len(cols)), (own_launch, bor_launch)
    if cfg.get("mask"):
        _same(bor, own, name + ": borrowed against owned (masks: the same rectangles)")
        return
    keep = np.ones(own["err"].shape[1], dtype=bool)
    keep[cols] = False
    _same(bor, own, name + ": borrowed against owned off the sliver columns", sel=keep)
    sam, ref, mask = _host(name)
    want = _copy(R.match(R.build(ns[1], name, sam, ref, mask=mask), name))
    cut = lambda res: {k: np.ascontiguousarray(v[:, cols]) for k, v in res.items() if k in MAPS}
    for tag, got in (("borrowed", bor), ("owned", own)):
        st = assert_parity(cut(got), cut(want), cfg["ms"], "borrowed %s sliver %s" % (name, tag), allow_illposed=R.illposed_share(cfg))
        print("%s, %s model, sliver columns %r: %d ok pixels, %d unconverged" % (name, tag, cols, st["ok"], st["unconverged"]))


def test_stepping_s2_runs_subset_rectangles_on_the_table_kernel(ns):
    """stepping_s2's ROI (regimes.STEPPING_EXTRA): the centre and three strips of at least 1024 pixels, each strip with a
    descriptor list of its two frames; at step 1 the whole region has nine rectangles (six with the borrowed model's cut
    column 180 between them and the three to its right).  corr_volume runs once per rectangle."""
    assert _borrowed(ns, "stepping_s2")[1].get("corr_volume") == 4 and _owned(ns, "stepping_s2")[1].get("corr_volume") == 4
    s, r, k, h = _embed("stepping_s2", "nan")
    m = R.build(ns[0], "stepping_s2", s, r, mask=k)
    R.match(m, "stepping_s2", mk=dict(ROI=None), timing=True)
    assert m.launch_counts.get("corr_volume") == 9, m.launch_counts
    G.check(h, "stepping_s2, whole region")


# ----------------------------------------------------------------------------- b. the surroundings of a frame

@pytest.mark.parametrize("name", ALL)
def test_results_do_not_depend_on_what_lies_around_a_frame(ns, name):
    """tight, NaN guards, 1e300 guards, odd element offsets: one result.  A kernel that lets a byte from outside a frame
    into a sum gives NaN in one layout, 1e300 in another and the neighbouring frame's row in the third; _borrowed checks
    after each match that the guards and the frames are what they were.

    Alignment (read in the kernels before this ran): corr_volume, corr_masked and corr_march stage 16-byte column pairs by
    buffer loads into LDS at byte offset 8 (row W + column) with the column of either parity (the shift offsets oj0 are odd
    and even), so sources at 8 mod 16 occur in frames the library owns too, whatever the base; prep_maps, match_staged,
    blur_tiles and match_direct read single doubles.  umpa_hip_create therefore has nothing to refuse for a base at 8 mod 16."""
    first = _borrowed(ns, name, LAYOUTS[0])
    for layout in LAYOUTS[1:]:
        got = _borrowed(ns, name, layout)
        _same(got[0], first[0], "%s: %s layout against %s guards" % (name, layout, LAYOUTS[0]))
        assert got[1] == first[1], (layout, got[1], first[1])


# ----------------------------------------------------------------------------- c. device outputs between canaries

OUT_SENTINEL = 123.25


def _device_match(m, name, region, planar, covermap=None, thr=0.0, uv0=None, abc=None, prefill=None, flags=0):
    """umpa_hip_match_region with UMPA_HIP_F_DEVICE_IO on a side stream, every array between guards; returns the maps as
    model.match names them (and `uv`), after the guards have been checked."""
    import torch
    from umpa_amd import _lib
    cfg = R.config(name)
    (start0, step0, N0), (start1, step1, N1) = region
    npar = m.Nparam
    dev = torch.device("cuda", m._device)
    stream = torch.cuda.Stream(device=dev)
    fill_f = 0.0 if prefill is None else prefill
    fill_i = 0 if prefill is None else 77
    with torch.cuda.stream(stream):
        def out(shape, dtype, row, value):
            (v,), h = G.embed([torch.full(shape, value, dtype=dtype)], G.min_guard(row), device=dev, inputs=False)
            return v, h
        vshape = (npar, N0, N1) if planar else (N0, N1, npar)
        arr = {"values": out(vshape, torch.float64, N1 * (1 if planar else npar), fill_f),
               "err": out((N0, N1), torch.int32, N1, fill_i),
               "debug_d": out((N0, N1, 25), torch.float64, 25 * N1, fill_f),
               "debug_a": out((N0, N1, 16), torch.float64, 16 * N1, fill_f),
               "debug_Ncalls": out((N0, N1), torch.int32, N1, fill_i)}
        if abc is not None:
            t = torch.from_numpy(abc).to(dev)
            if planar:
                arr["values"][0][4:7] = t.permute(2, 0, 1)
            else:
                arr["values"][0][:, :, 4:7] = t
        ins = []
        if uv0 is not None:
            uv = np.zeros((N0, N1, 2))
            uv[..., 0], uv[..., 1] = uv0
            arr["uv"] = out((N0, N1, 2), torch.float64, 2 * N1, 0.0)
            arr["uv"][0].copy_(torch.from_numpy(uv))
        if covermap is not None:
            (cv,), hc = G.embed([covermap], G.min_guard(N1), device=dev)
            ins.append(hc)
        torch.cuda.current_stream().synchronize()
        ptr = lambda k: arr[k][0].data_ptr() if k in arr else None
        fl = cfg["force"] | _lib.F_DEVICE_IO | (_lib.F_PLANAR if planar else 0) | flags
        m._lib.check(m._lib.match_region(m._handle, start0, step0, N0, start1, step1, N1,
                                         ptr("values"), npar, ptr("uv"), ptr("err"),
                                         cv.data_ptr() if covermap is not None else None, float(thr),
                                         ptr("debug_d"), ptr("debug_a"), ptr("debug_Ncalls"), fl,
                                         ctypes.c_void_p(stream.cuda_stream)), "match_region")
    stream.synchronize()
    what = "%s, device outputs (%s)" % (name, "planar" if planar else "interleaved")
    for k, (v, h) in arr.items():
        G.check(h, "%s: %s" % (what, k))
    for h in ins:
        G.check(h, what + ": covermap")
    res = {k: v.cpu().numpy() for k, (v, h) in arr.items()}
    v = res.pop("values")
    planes = v if planar else np.moveaxis(v, 2, 0)
    for q, k in enumerate(("f", "T", "dx", "dy") + (("df",) if cfg["df"] and not cfg.get("kernel") else ())):
        res[k] = np.ascontiguousarray(planes[q])
    res["_planes"] = np.ascontiguousarray(planes)
    return res


def _host_uv(m, name, region, uv0, covermap, thr):
    """umpa_hip_match_region on host arrays: the uv array it hands back (model.match does not return it)"""
    cfg = R.config(name)
    (start0, step0, N0), (start1, step1, N1) = region
    values, err = np.zeros((N0, N1, m.Nparam)), np.zeros((N0, N1), np.int32)
    uv = np.zeros((N0, N1, 2))
    uv[..., 0], uv[..., 1] = uv0
    m._lib.check(m._lib.match_region(m._handle, start0, step0, N0, start1, step1, N1, values.ctypes.data, m.Nparam, uv.ctypes.data,
                                     err.ctypes.data, covermap.ctypes.data if covermap is not None else None, float(thr),
                                     None, None, None, cfg["force"], None), "match_region")
    return uv


def _model_region(m, mk):
    s0, s1 = m._convert_ROI_slice(mk.get("ROI"), mk.get("step"))
    N0, N1 = m._counts(s0, s1)
    return (s0[0], s0[2], N0), (s1[0], s1[2], N1)


def _models(ns, name):
    """(tag, model, guard handle or None): one that owns its frames, one that borrows them between NaN guards"""
    sam, ref, mask = _host(name)
    yield "owned", R.build(ns[0], name, sam, ref, mask=mask), None
    s, r, k, h = _embed(name, "nan")
    yield "borrowed", R.build(ns[0], name, s, r, mask=k), h


def _coverage_args(m, cfg, region):
    """the coverage map and threshold model.match passes (model.pyx:431)"""
    if m._trivial_coverage():
        return None, 0.0
    (a0, t0, N0), (a1, t1, N1) = region
    cover = m.coverage(ROI=((a0, a0 + t0 * (N0 - 1) + 1, t0), (a1, a1 + t1 * (N1 - 1) + 1, t1)))
    return cover, .1 * cover.max() / cfg["K"]


DEVICE_OUT = ["tiled_DF", "tiled_NoDF", "march_DF", "masked_w_DF", "staged_NoDF", "plain_DF", "stepping_DF", "stepping_mask_DF",
              "stepping_s2", "dfkernel"]


@pytest.mark.parametrize("name", DEVICE_OUT)
def test_device_outputs_between_canaries(ns, name):
    """values, uv (where the configuration has start shifts), err and the three debug arrays, each in a tensor of its own
    with guards of two rows and a wavefront; interleaved and UMPA_HIP_F_PLANAR; a model that owns its frames and one that
    borrows them: the maps of the host-output match (the owning model's; on a stepping configuration's sliver columns the
    model's own kind decides, see test_borrowed_equals_owned), every guard intact, the borrowed stack untouched."""
    cfg = R.config(name)
    mk = cfg.get("mk", {})
    for tag, m, h in _models(ns, name):
        region = _model_region(m, mk)
        want = (_owned if tag == "owned" else _borrowed)(ns, name)[0]
        cover, thr = _coverage_args(m, cfg, region)
        abc = R.kernel_abc((region[0][2], region[1][2])) if cfg.get("kernel") else None
        uvs = []
        for planar in (False, True):
            got = _device_match(m, name, region, planar, covermap=cover, thr=thr, uv0=mk.get("dxdy"), abc=abc)
            assert m._lib.last_path(m._handle) == cfg["path"]
            _same({k: got[k] for k in MAPS if k in got}, {k: want[k] for k in MAPS if k in want}, "%s, %s model, planar %r" % (name, tag, planar))
            if abc is not None:                                       # the kernel's inputs stay where they were
                assert np.array_equal(got["_planes"][4:7], np.moveaxis(abc, 2, 0))
            if "uv" in got:
                uvs.append(got["uv"])
        if uvs:                                                       # the in/out start shifts: those of the host-array call
            host_uv = _host_uv(m, name, region, mk["dxdy"], cover, thr)
            assert not np.array_equal(host_uv[..., 0], np.full_like(host_uv[..., 0], mk["dxdy"][0]))     # (the call writes them)
            for u in uvs:
                assert np.array_equal(u, host_uv, equal_nan=True), "%s, %s model: uv differs from the host-array call's" % (name, tag)
        if h is not None:
            G.check(h, name + ": the borrowed stack after device-output matches")


def test_device_outputs_of_an_odd_roi(ns):
    """tiled_DF10, a ROI of 45 x 77 pixels (odd, no multiples of the 32-pixel tile) at an odd origin"""
    name = "tiled_DF10"
    roi = ((5, 50, 1), (7, 84, 1))
    for tag, m, h in _models(ns, name):
        want = _copy(R.match(m, name, mk=dict(ROI=roi)))
        m.ROI = None
        region = _model_region(m, dict(ROI=roi))
        assert (region[0][2], region[1][2]) == (45, 77)
        for planar in (False, True):
            got = _device_match(m, name, region, planar)
            assert m._lib.last_path(m._handle) == 2
            _same({k: got[k] for k in MAPS if k in got}, {k: want[k] for k in MAPS if k in want}, "%s ROI, %s model, planar %r" % (name, tag, planar))
        if h is not None:
            G.check(h, name + " ROI: the borrowed stack")


@pytest.mark.parametrize("name", ["tiled_DF", "staged_NoDF", "stepping_DF"])
def test_pixels_below_the_coverage_threshold_keep_what_the_arrays_held(ns, name):
    """A coverage map of the test's own (uniform numbers in [0, 1)) and a threshold of 0.5: about half of the pixels are
    skipped.  umpa_hip_match_region leaves values, uv and err of a skipped pixel as the caller's arrays held them (host
    arrays: include/umpa_hip.h, "in/out"; the debug arrays of a host-array call are cleared instead); with device arrays
    nothing is seeded or cleared, so every array keeps its bits there.  Elsewhere the maps are those of the match without
    a coverage map."""
    cfg = R.config(name)
    for tag, m, h in _models(ns, name):
        region = _model_region(m, cfg.get("mk", {}))
        N0, N1 = region[0][2], region[1][2]
        cover = np.random.default_rng(99).random((N0, N1))
        skip = cover < 0.5
        assert 0.4 < skip.mean() < 0.6
        want = (_owned if tag == "owned" else _borrowed)(ns, name)[0]
        for planar in (False, True):
            got = _device_match(m, name, region, planar, covermap=cover, thr=0.5, prefill=OUT_SENTINEL)
            for k in MAPS:
                if k not in want:
                    continue
                held = 77 if got[k].dtype == np.int32 else OUT_SENTINEL
                assert np.array_equal(got[k][~skip], want[k][~skip], equal_nan=True), (name, tag, planar, k)
                assert (got[k][skip] == held).all(), "%s, %s model, planar %r: %s of a skipped pixel was written" % (name, tag, planar, k)
        if h is not None:
            G.check(h, name + " coverage: the borrowed stack")


def test_row_pieces_tile_the_region_once(ns):
    """umpa_hip_set_rows_callback with piece_rows = 32 on tiled_DF's 100 rows: the callback's row ranges tile [0, 100)
    exactly once, in order, at multiples of 32, and the maps are those of the match in one piece."""
    from umpa_amd import _lib
    name = "tiled_DF"
    for tag, m, h in _models(ns, name):
        region = _model_region(m, {})
        N0 = region[0][2]
        assert N0 > 64
        pieces = []
        cb = _lib.ROWS_FN(lambda lo, hi, user: pieces.append((lo, hi)))
        want = (_owned if tag == "owned" else _borrowed)(ns, name)[0]
        m._lib.check(m._lib.set_rows_callback(m._handle, cb, None, 32), "set_rows_callback")
        try:
            for planar in (False, True):
                del pieces[:]
                got = _device_match(m, name, region, planar)
                assert pieces[0][0] == 0 and pieces[-1][1] == N0 and len(pieces) >= 3, pieces
                assert all(a[1] == b[0] for a, b in zip(pieces, pieces[1:])) and all(lo < hi for lo, hi in pieces), pieces
                assert all(lo % 32 == 0 for lo, _ in pieces), pieces
                _same({k: got[k] for k in MAPS if k in got}, {k: want[k] for k in MAPS if k in want}, "%s in row pieces, %s model" % (name, tag))
        finally:
            m._lib.set_rows_callback(m._handle, None, None, 0)
        if h is not None:
            G.check(h, name + " pieces: the borrowed stack")


# ----------------------------------------------------------------------------- d. stacks that change in place

def _second_stack(name):
    """another stack of the configuration's shape: the first one's frames in another order, the sample times 1.25 (other
    maps at every pixel, the same speckle statistics)"""
    sam, ref, mask = _host(name)
    return np.ascontiguousarray(1.25 * sam[::-1]), np.ascontiguousarray(ref[::-1])


class InPlace:
    """One borrowed model on tensors the test rewrites; after every match a fresh borrowed model on a copy of the current
    data makes the same call, and the two results are equal bit for bit, last_path included."""

    def __init__(self, ns, name):
        self.ns, self.name = ns, name
        self.sam, self.ref, self.mask, self.h = _embed(name, "nan")
        self.live = R.build(ns[0], name, self.sam, self.ref, mask=self.mask)
        self.steps = 0

    def write(self, sam=None, ref=None, mask=None):
        import torch
        for dst, src in ((self.sam, sam), (self.ref, ref), (self.mask, mask)):
            if src is not None:
                for d, s in zip(dst, src):
                    d.copy_(torch.from_numpy(np.ascontiguousarray(s)))
        torch.cuda.synchronize()

    def match(self, what, flags=0, **mk):
        cfg = R.config(self.name)
        self.live._force = cfg["force"] | flags
        self.live.ROI = None
        got = _copy(R.match(self.live, self.name, mk=mk, path=None))
        path = self.live._lib.last_path(self.live._handle)
        clone = lambda fr: None if fr is None else [f.clone() for f in fr]
        twin = R.build(self.ns[0], self.name, clone(self.sam), clone(self.ref), mask=clone(self.mask))
        want = _copy(R.match(twin, self.name, mk=mk, path=None))
        self.steps += 1
        tag = "%s in place, step %d (%s)" % (self.name, self.steps, what)
        assert path == twin._lib.last_path(twin._handle), tag
        _same(got, want, tag)
        return got, path


def _inside_roi(name):
    """a ROI of at least 1024 pixels that every frame contributes to, off the region's origin"""
    return {"tiled_DF": ((40, 80, 1), (33, 97, 1)), "masked_bin_DF": ((40, 80, 1), (33, 97, 1)),
            "stepping_DF": ((20, 90, 1), (20, 100, 1)), "stepping_s2": ((40, 130, 1), (50, 170, 1))}[name]


@pytest.mark.parametrize("name", ["tiled_DF", "masked_bin_DF", "stepping_DF", "stepping_s2"])
def test_stacks_rewritten_in_place_under_one_borrowed_model(ns, name):
    """The frame addresses of a borrowed model never change, its contents do (KernelSearch blurs into one buffer per
    candidate, a sharded rank receives halos into row views): whatever the library keeps between matches by address --
    the reference-side maps (ref_maps_ok) and the tile rectangle they cover, the stepping rectangles' descriptor lists, the
    coverage map -- must not stand in for data that has changed.  All four trajectories of the issue run on all four
    configurations (stepping_s2 is here for its tiled subset rectangles, which stepping_DF does not have); the mask
    trajectory on the masked one.  (With `reuse` forced true for borrowed frames in run_tiled all four configurations fail here,
    at "reference stack overwritten in place" or, stepping_s2, at "reference overwritten between two matches of the ROI": its
    whole-region matches end on a subset rectangle, which drops the maps.  With mask_binary true for borrowed models the
    fractional step fails against the oracle.)  KernelSearch's A, B, A is tests/test_hip_ddf.py::test_sequence_of_candidates_on_one_searcher."""
    from umpa_amd import _lib
    samA, refA, maskA = _host(name)
    samB, refB = _second_stack(name)
    t = InPlace(ns, name)
    base, p0 = t.match("as built", **R.config(name).get("mk", {}))
    t.write(sam=samB)
    after_sam, _ = t.match("sample stack overwritten in place")
    if "mk" not in R.config(name):
        assert not np.array_equal(after_sam["dx"], base["dx"])
    t.match("the same again")
    t.write(ref=refB)
    after_ref, _ = t.match("reference stack overwritten in place, no reuse flag")
    assert not np.array_equal(after_ref["T"], after_sam["T"])         # (the stacks differ: stale maps would show)
    t.write(sam=samA)
    t.match("only the sample changed, UMPA_HIP_F_REUSE_REF_MAPS", flags=_lib.F_REUSE_REF_MAPS)
    t.write(sam=samB)
    t.match("... and again with the flag", flags=_lib.F_REUSE_REF_MAPS)
    roi = _inside_roi(name)
    _, p_roi = t.match("a ROI every frame covers", ROI=roi)
    assert p_roi == 2                                                 # (every frame contributes: the plain tiled path, stepping or not)
    t.write(ref=refA)
    t.match("reference overwritten after a ROI: the whole region")
    t.match("the ROI again", ROI=roi)
    t.write(ref=refB)
    t.match("reference overwritten between two matches of the ROI, no reuse flag", ROI=roi)
    t.write(ref=refA)
    t.match("... and back", ROI=roi)
    t.write(sam=samA)
    t.match("the ROI, sample overwritten, reuse flag", flags=_lib.F_REUSE_REF_MAPS, ROI=roi)
    t.match("the whole region with the flag: the ROI's tiles do not cover it", flags=_lib.F_REUSE_REF_MAPS)
    back, p1 = t.match("the first stacks again, whole region")
    if "mk" not in R.config(name):
        _same(back, base, name + ": the first data gives the first maps again")
    assert p1 == p0
    if maskA is not None:
        w = np.random.default_rng(4107).uniform(0.2, 1.0, size=maskA.shape) * maskA
        t.write(mask=w)
        frac, _ = t.match("0/1 masks overwritten by fractional weights")
        assert not np.array_equal(frac["f"], back["f"])
        # against the CPU oracle at the suite's bar first (live model, twin and an owning model could share a wrong pair weight) ...
        want = _copy(R.match(R.build(ns[1], name, samA, refA, mask=w), name, mk={}))
        assert_parity(frac, want, R.config(name)["ms"], "borrowed %s fractional masks in place" % name, allow_illposed=R.illposed_share(R.config(name)))
        # ... then bit for bit against a model that owns these weights and has looked at them (mask_binary false there)
        own = R.build(ns[0], name, samA, refA, mask=w)
        _same(frac, _copy(R.match(own, name, mk={})), name + ": fractional weights in place against an owning model")
        t.write(mask=maskA)
        again, _ = t.match("... and back")
        _same(again, back, name + ": the 0/1 masks give their maps again")
    G.check(t.h, name + ": guards of the rewritten stack", frames=False)
    print("\n[borrowed in place] %s: %d steps compared" % (name, t.steps))
