"""
search='grid' and cost_volume() on the GPU (libumpa_grid.so): against extended precision (tests/grid_expect.py), against the
walk on the same device, through every route to the exhaustive table, and the refusals.

REACHES names, per test, the kernels of libumpa_grid.so it is there for (tests/test_grid_cpu.py checks on the CPU that every
grid_min_kernel / cost_volume_kernel symbol of the built library is claimed here, and that no claim is stale).
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import Case, assert_parity

import grid_expect as GE

pytestmark = pytest.mark.gpu

KTEMPL = 24                      # UMPA_KTEMPL: frame counts with their own instantiation (dark-field model)
REACHES = {
    "tests/test_hip_grid.py::test_every_frame_count":
        ["%s<1, %d>" % (f, n if n <= KTEMPL else 0) for f in ("grid_min_kernel", "cost_volume_kernel") for n in range(1, KTEMPL + 2)],
    "tests/test_hip_grid.py::test_cost_volume_against_extended_precision": ["cost_volume_kernel<0, 0>"],
    "tests/test_hip_grid.py::test_grid_integer_minimum_against_extended_precision": ["grid_min_kernel<0, 0>"],
}

HP_CASES = [(n, k, a) for n in sorted(GE.STACKS) for k in (0, 1) for a in ("sam", "ref")]
HP_IDS = ["%s-%s-%s" % (n, "DF" if k else "NoDF", a) for n, k, a in HP_CASES]


@pytest.fixture(scope="module")
def hip_ns():
    from umpa_amd import _lib, model
    if _lib.hip().device_count() < 1:
        pytest.fail("no HIP device: the GPU tests cannot run (there is no CPU fallback)")
    return model


def _model(hip_ns, kind, sam, ref, Nw, ms, assign="sam", subpx=-1, **kw):
    m = (hip_ns.UMPAModelDF if kind else hip_ns.UMPAModelNoDF)(sam, ref, window_size=Nw, max_shift=ms, **kw)
    m.assign_coordinates = assign
    m.sub_pixel_mode = subpx
    return m


def _hp_model(hip_ns, name, kind, assign, subpx):
    sam, ref, c = GE.stack(name)
    return _model(hip_ns, kind, sam, ref, c["Nw"], c["ms"], assign, subpx), sam, ref, c


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


def _same(a, b, keys=None, what=""):
    for k in keys or sorted(set(a) & set(b)):
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s %s" % (what, k))


def _memo_in_volume(walk, vol, ms, pad, org=(0, 0), step=1):
    """the known cells of a sub_pixel_mode-0 walk's memo and the volume's entries for the same (pixel, shift)"""
    from oracle import hp_cost
    (xi, xj, q), _, (si, sj) = hp_cost.memo_cells(walk, pad, org, step)
    return walk["debug_d"][xi, xj, q], vol["cost"][si + ms - 1, sj + ms - 1, xi, xj]


# ----------------------------------------------------------------------------- 1. cost_volume against extended precision

@pytest.mark.parametrize("name,kind,assign", HP_CASES, ids=HP_IDS)
def test_cost_volume_against_extended_precision(hip_ns, name, kind, assign):
    m, sam, ref, c = _hp_model(hip_ns, name, kind, assign, 0)
    ms = c["ms"]
    vol = m.cost_volume(with_fit=True)
    hp = GE.hp_volumes(kind, sam, ref, m.window, ms, m.padding, assign)
    assert vol["cost"].shape == hp["cost"].shape == (2 * ms - 1, 2 * ms - 1) + m.extent
    ratio = np.abs(vol["cost"].astype(np.longdouble) - hp["cost"]) / hp["bound"]
    rT = np.abs(vol["T"] - hp["T"]) / np.abs(hp["T"])
    print("%s kind %d %s: max |gpu - hp| / bound %.4f, T rel %.2e" % (name, kind, assign, ratio.max(), rT.max()), end="")
    assert np.all(ratio <= 1.0), "max |gpu - hp| / bound = %.4f" % ratio.max()
    assert np.all(rT <= 1e-5)
    assert ("df" in vol) == (kind == 1)
    if kind:
        rdf = np.abs(vol["df"] - hp["df"]) / np.abs(hp["df"])
        print(", df rel %.2e" % rdf.max(), end="")
        assert np.all(rdf <= 1e-5)
    print()
    only_cost = m.cost_volume()
    assert sorted(only_cost) == ["cost"]
    np.testing.assert_array_equal(only_cost["cost"], vol["cost"])
    # the numbers are the walk's own: every known cell of a walk's memo, bit for bit
    walk = m.match(quiet=True)
    d, v = _memo_in_volume(walk, vol, ms, m.padding)
    assert d.size > 10 * walk["err"].sum() > 0
    np.testing.assert_array_equal(d, v)


# ----------------------------------------------------------------------------- 2. the integer minimum

@pytest.mark.parametrize("name,kind,assign", HP_CASES, ids=HP_IDS)
def test_grid_integer_minimum_against_extended_precision(hip_ns, name, kind, assign):
    m, sam, ref, c = _hp_model(hip_ns, name, kind, assign, 0)
    got = m.match(quiet=True, search="grid")
    exp, near = GE.expected_for(name, kind, assign, 0)
    keep = ~near
    print("%s kind %d %s: %d of %d pixels near-tie, %d ok" % (name, kind, assign, near.sum(), near.size, exp["err"].sum()))
    assert near.mean() <= GE.NEAR_TIE_CAP
    assert got["err"].dtype == np.int32
    np.testing.assert_array_equal(got["err"][keep], exp["err"][keep])
    np.testing.assert_array_equal(got["debug_Ncalls"][keep], exp["debug_Ncalls"][keep])
    np.testing.assert_array_equal(got["dy"][keep], exp["ci"][keep])
    np.testing.assert_array_equal(got["dx"][keep], exp["cj"][keep])
    ok = keep & (exp["err"] == 1)
    np.testing.assert_array_equal(got["f"][ok], exp["f"][ok])                  # 1 - ip: the quadrant
    # the debug arrays in the documented layout: the 4x4 and the 5x5 (-1 outside the search range) around the minimum
    assert np.array_equal(got["debug_d"][keep] < 0, exp["debug_d"][keep] < 0)
    for k in ("debug_a", "debug_d"):
        assert np.all(np.abs(got[k][keep] - exp[k][keep]) <= 1e-6 * np.abs(exp[k][keep])), k


# ----------------------------------------------------------------------------- 3. the sub-pixel modes, the parity bar

@pytest.mark.parametrize("subpx", [-1, 1])
@pytest.mark.parametrize("name,kind,assign", HP_CASES, ids=HP_IDS)
def test_grid_subpixel_modes_meet_the_parity_bar(hip_ns, name, kind, assign, subpx):
    m, sam, ref, c = _hp_model(hip_ns, name, kind, assign, subpx)
    got = m.match(quiet=True, search="grid")
    exp, near = GE.expected_for(name, kind, assign, subpx)
    assert near.mean() <= GE.NEAR_TIE_CAP
    want = {k: exp[k] for k in ("err", "debug_Ncalls", "dx", "dy", "f", "T", "debug_a", "debug_d") + (("df",) if kind else ())}
    got = {k: np.array(got[k]) for k in want}
    for k in want:                                                    # near-tie pixels: out of both sides
        got[k][near] = want[k][near]
    st = assert_parity(got, want, c["ms"], "grid %s %s %s subpx %d" % (name, "DF" if kind else "NoDF", assign, subpx), subpx=subpx)
    assert st["ok"] > 0.5 * near.size


# ----------------------------------------------------------------------------- 4. walk and grid, same device, same build

def _walk_vs_grid(hip_ns, sam, ref, Nw, ms, kind, assign, label):
    m = _model(hip_ns, kind, sam, ref, Nw, ms, assign, 0)
    walk0 = m.match(quiet=True)
    grid0 = m.match(quiet=True, search="grid")
    cmin = grid0["debug_d"][..., 12]                                  # the grid's minimum cost
    known = walk0["debug_d"] >= 0
    assert not (known & (walk0["debug_d"] < cmin[..., None])).any(), "%s: a walk has seen a cost below the grid's minimum" % label
    both = (walk0["err"] == 1) & (grid0["err"] == 1) & (walk0["dx"] == grid0["dx"]) & (walk0["dy"] == grid0["dy"])
    above = (walk0["err"] == 1) & (walk0["debug_d"][..., 12] > cmin)
    np.testing.assert_array_equal(walk0["f"][both], grid0["f"][both])
    np.testing.assert_array_equal(walk0["debug_a"][both], grid0["debug_a"][both])
    del walk0, grid0, known
    m.debug = False
    for mode in (-1, 1):
        m.sub_pixel_mode = mode
        w, g = m.match(quiet=True), m.match(quiet=True, search="grid")
        for k in ("dx", "dy", "f"):
            np.testing.assert_array_equal(w[k][both], g[k][both], err_msg="%s subpx %d %s" % (label, mode, k))
    print("%s: %d pixels, both ok on the same integer minimum %.2f %%, the walk ended above the global minimum on %.3f %%" % (
        label, both.size, 100.0 * both.mean(), 100.0 * above.mean()))
    assert both.mean() > 0.5


def test_walk_and_grid_agree_at_C2_full_size(hip_ns):
    from umpa_amd.synth import make_stack
    sam, ref, _ = make_stack(2048, 2048, 10, 5, df=True, seed=0, order=1)
    _walk_vs_grid(hip_ns, sam, ref, 5, 5, 1, "sam", "C2")


def test_walk_and_grid_agree_on_golden_B_walks(hip_ns):
    c = Case("B_walks")
    for kind in (0, 1):
        for assign in ("sam", "ref"):
            _walk_vs_grid(hip_ns, c.sam, c.ref, c.Nw, c.max_shift, kind, assign, "B_walks %s %s" % ("DF" if kind else "NoDF", assign))


# ----------------------------------------------------------------------------- 5. every route to the table

def test_wide_windows_through_the_marching_table(hip_ns):
    """C3-type parameters: corr_march's strip-blocked table.  The volume against extended precision on a lattice of pixels
    (all shifts of each: at most regimes.HP_MAX_CELLS cells), the grid's minimum against the volume everywhere."""
    import regimes
    from umpa_amd.synth import make_stack
    K, Nw, ms, n = 20, 7, 8, 384
    U = 2 * ms - 1
    sam, ref, _ = make_stack(n, n, K, ms, df=True, seed=5, order=1)
    m = _model(hip_ns, 1, sam, ref, Nw, ms, "sam", 0)
    got, seen = _launches(m, lambda: m.match(quiet=True, search="grid"))
    assert seen.get("corr_march", 0) >= 1 and seen.get("table_consumer", 0) >= 1 and "replay_walk" not in seen and "corr_volume" not in seen, seen
    vol, seen = _launches(m, lambda: m.cost_volume(with_fit=True))
    assert seen.get("corr_march", 0) >= 1 and seen.get("table_consumer", 0) >= 1, seen
    N0, N1 = m.extent
    stride = next(s for s in range(1, N0) if len(range(s // 2, N0, s)) * len(range(s // 2, N1, s)) * U * U <= regimes.HP_MAX_CELLS)
    xi, xj = np.meshgrid(np.arange(stride // 2, N0, stride), np.arange(stride // 2, N1, stride), indexing="ij")
    hp = GE.hp_volumes(1, sam, ref, m.window, ms, m.padding, "sam", pixels=(xi, xj))
    assert 1000 < hp["cost"].size <= regimes.HP_MAX_CELLS
    ratio = np.abs(vol["cost"][:, :, xi, xj].astype(np.longdouble) - hp["cost"]) / hp["bound"]
    print("C3-type: %d cells on a lattice of stride %d, max |gpu - hp| / bound %.4f" % (hp["cost"].size, stride, ratio.max()))
    assert np.all(ratio <= 1.0)
    for k in ("T", "df"):
        assert np.all(np.abs(vol[k][:, :, xi, xj] - hp[k]) <= 1e-5 * np.abs(hp[k])), k
    near = GE.near_tie(hp["cost"], hp["bound"])
    arg = np.argmin(hp["cost"].reshape((U * U,) + xi.shape), axis=0)
    keep = ~near
    np.testing.assert_array_equal(got["dy"][xi, xj][keep], (arg // U - (ms - 1))[keep])
    np.testing.assert_array_equal(got["dx"][xi, xj][keep], (arg % U - (ms - 1))[keep])
    # every pixel: the first strict minimum of the volume
    arg = np.argmin(vol["cost"].reshape(U * U, N0, N1), axis=0)
    np.testing.assert_array_equal(got["dy"], arg // U - (ms - 1))
    np.testing.assert_array_equal(got["dx"], arg % U - (ms - 1))
    np.testing.assert_array_equal(got["debug_d"][..., 12], vol["cost"].reshape(U * U, N0, N1).min(axis=0))
    np.testing.assert_array_equal(got["debug_Ncalls"], U * U)


def _chunk_stack():
    from umpa_amd.synth import make_stack
    # 128 x 512 output pixels, 81 planes of 512 doubles per row: a 16 MB table holds 32 rows -> four row chunks
    return make_stack(144, 528, 4, 5, df=True, seed=9, order=1)[:2]


def test_four_row_chunks_change_nothing(hip_ns, monkeypatch):
    sam, ref = _chunk_stack()
    res = {}
    for mb in (None, "16"):
        if mb:
            monkeypatch.setenv("UMPA_HIP_TABLE_MB", mb)
        else:
            monkeypatch.delenv("UMPA_HIP_TABLE_MB", raising=False)
        m = _model(hip_ns, 1, sam, ref, 3, 5)
        g, seen_g = _launches(m, lambda: m.match(quiet=True, search="grid"))
        v, seen_v = _launches(m, lambda: m.cost_volume(with_fit=True))
        assert seen_g.get("table_consumer") == seen_v.get("table_consumer") == (4 if mb else 1), (mb, seen_g, seen_v)
        res[mb] = (g, v)
    _same(res[None][0], res["16"][0], what="grid, four chunks")
    _same(res[None][1], res["16"][1], what="volume, four chunks")


def test_roi_and_steps_are_slices_of_the_full_result(hip_ns):
    sam, ref = _chunk_stack()
    for kind in (0, 1):
        m = _model(hip_ns, kind, sam, ref, 3, 5)
        full, vfull = m.match(quiet=True, search="grid"), m.cost_volume(with_fit=True)
        N0, N1 = m.extent
        for step in (2, 3):
            m.ROI = None
            part = m.match(quiet=True, search="grid", step=step)
            for k in full:
                np.testing.assert_array_equal(part[k], full[k][::step, ::step], err_msg="step %d %s" % (step, k))
            m.ROI = None
            vpart = m.cost_volume(step=step, with_fit=True)
            for k in vfull:
                np.testing.assert_array_equal(vpart[k], vfull[k][:, :, ::step, ::step], err_msg="volume step %d %s" % (step, k))
        roi = ((17, 90, 2), (5, 400, 3))
        m.ROI = None
        part, vpart = m.match(quiet=True, search="grid", ROI=roi), m.cost_volume(ROI=roi)
        for k in full:
            np.testing.assert_array_equal(part[k], full[k][17:90:2, 5:400:3], err_msg="ROI %s" % k)
        np.testing.assert_array_equal(vpart["cost"], vfull["cost"][:, :, 17:90:2, 5:400:3])


@pytest.mark.parametrize("K", list(range(1, KTEMPL + 2)))
def test_every_frame_count(hip_ns, K):
    """One instantiation per frame count up to UMPA_KTEMPL, the generic one beyond: the volume holds the walk's numbers bit for
    bit, the grid's minimum is the volume's first strict minimum, and where walk and grid agree on it so do dx, dy, f."""
    from umpa_amd.synth import make_stack
    Nw, ms = 2, 3
    U = 2 * ms - 1
    sam, ref, _ = make_stack(44, 80, K, ms, df=True, seed=100 + K)
    for assign in ("sam", "ref"):
        m = _model(hip_ns, 1, sam, ref, Nw, ms, assign, 0)
        walk = m.match(quiet=True)
        (grid, vol), seen = _launches(m, lambda: (m.match(quiet=True, search="grid"), m.cost_volume(with_fit=True)))
        assert seen.get("table_consumer") == 2 and "replay_walk" not in seen, seen
        d, v = _memo_in_volume(walk, vol, ms, m.padding)
        assert d.size > 0
        np.testing.assert_array_equal(d, v)
        N0, N1 = m.extent
        flat = vol["cost"].reshape(U * U, N0, N1)
        arg = np.argmin(flat, axis=0)
        np.testing.assert_array_equal(grid["dy"], arg // U - (ms - 1))
        np.testing.assert_array_equal(grid["dx"], arg % U - (ms - 1))
        pick = lambda a: np.take_along_axis(a.reshape(U * U, N0, N1), arg[None], axis=0)[0]
        np.testing.assert_array_equal(grid["T"], pick(vol["T"]))
        np.testing.assert_array_equal(grid["df"], pick(vol["df"]))
        both = (walk["err"] == 1) & (grid["err"] == 1) & (walk["dx"] == grid["dx"]) & (walk["dy"] == grid["dy"])
        assert both.any() and (grid["err"] == 1).mean() > 0.3
        m.sub_pixel_mode = -1
        w, g = m.match(quiet=True), m.match(quiet=True, search="grid")
        for k in ("dx", "dy", "f"):
            np.testing.assert_array_equal(w[k][both], g[k][both], err_msg="K %d %s %s" % (K, assign, k))


def test_device_arrays_on_a_side_stream(hip_ns):
    import torch
    from umpa_amd import _lib
    sam, ref = _chunk_stack()
    for kind in (0, 1):
        m = _model(hip_ns, kind, sam, ref, 3, 5)
        host, vhost = m.match(quiet=True, search="grid"), m.cost_volume(with_fit=True)
        N0, N1 = m.extent
        U, np_ = 2 * m.max_shift - 1, m.Nparam
        dev = torch.device("cuda", m._device)
        stream = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(stream):
            values = torch.zeros((N0, N1, np_), dtype=torch.float64, device=dev)
            err = torch.zeros((N0, N1), dtype=torch.int32, device=dev)
            dd = torch.zeros((N0, N1, 25), dtype=torch.float64, device=dev)
            da = torch.zeros((N0, N1, 16), dtype=torch.float64, device=dev)
            dn = torch.zeros((N0, N1), dtype=torch.int32, device=dev)
            vols = {k: torch.zeros((U, U, N0, N1), dtype=torch.float64, device=dev) for k in vhost}
            sp = ctypes.c_void_p(stream.cuda_stream)
            g = _lib.grid()
            g.check(g.match_region(m._handle, 0, 1, N0, 0, 1, N1, values.data_ptr(), np_, None, err.data_ptr(), None, 0.0,
                                   dd.data_ptr(), da.data_ptr(), dn.data_ptr(), _lib.F_DEVICE_IO, sp), "grid match_region")
            g.check(g.cost_volume(m._handle, 0, 1, N0, 0, 1, N1, vols["cost"].data_ptr(), vols["T"].data_ptr(),
                                  vols["df"].data_ptr() if "df" in vols else None, _lib.F_DEVICE_IO, sp), "grid cost_volume")
        stream.synchronize()
        v = values.cpu().numpy()
        for q, k in enumerate(("f", "T", "dx", "dy") + (("df",) if kind else ())):
            np.testing.assert_array_equal(v[..., q], host[k], err_msg=k)
        for k, t in (("err", err), ("debug_d", dd), ("debug_a", da), ("debug_Ncalls", dn)):
            np.testing.assert_array_equal(t.cpu().numpy(), host[k], err_msg=k)
        for k in vhost:
            np.testing.assert_array_equal(vols[k].cpu().numpy(), vhost[k], err_msg="volume " + k)


# ----------------------------------------------------------------------------- 6. refusals

def test_refusals_and_the_walk_afterwards(hip_ns):
    from umpa_amd import _lib
    sam, ref, c = GE.stack("64x72x3")
    Nw, ms = c["Nw"], c["ms"]
    m = _model(hip_ns, 1, sam, ref, Nw, ms)
    before = m.match(quiet=True)
    with pytest.raises(ValueError):
        m.match(quiet=True, search="spiral")
    with pytest.raises(RuntimeError, match="grid"):
        m.match(quiet=True, search="grid", dxdy=(1.0, 0.0))
    # the library's own refusals: start shifts, a forced direct kernel, a step past the tiled path's limit
    g = _lib.grid()
    N0, N1 = m.extent
    vals, err, uv = np.zeros((N0, N1, 5)), np.zeros((N0, N1), np.int32), np.zeros((N0, N1, 2))
    args = lambda uvp, flags, step=1, n0=N0, n1=N1: (m._handle, 0, step, n0, 0, step, n1, vals.ctypes.data, 5, uvp, err.ctypes.data,
                                                    None, 0.0, None, None, None, flags, None)
    assert g.match_region(*args(uv.ctypes.data, 0)) == -1 and "start shifts" in g.error()
    assert g.match_region(*args(None, _lib.F_FORCE_DIRECT)) == -4 and "grid" in g.error()
    assert g.match_region(*args(None, 0, 10, 4, 4)) == -4 and "grid" in g.error()
    with pytest.raises(RuntimeError, match="grid"):
        m.match(quiet=True, search="grid", step=10)
    m.ROI = None
    m._force = _lib.F_FORCE_DIRECT
    with pytest.raises(RuntimeError, match="grid"):
        m.match(quiet=True, search="grid")
    with pytest.raises(RuntimeError, match="grid"):
        m.cost_volume()
    m._force = 0
    mask = np.ones_like(sam)
    mask[:, 20:24, 30:40] = 0.0
    masked = _model(hip_ns, 1, sam, ref, Nw, ms, mask_list=mask)
    with pytest.raises(RuntimeError, match="grid"):
        masked.match(quiet=True, search="grid")
    with pytest.raises(RuntimeError, match="grid"):
        masked.cost_volume()
    pos = [np.array(p) for p in ((0, 0), (2, 1), (1, 3))]
    stepped = _model(hip_ns, 1, sam, ref, Nw, ms, pos_list=pos)
    with pytest.raises(RuntimeError, match="grid"):
        stepped.match(quiet=True, search="grid")
    # ... also where the Python layer's own checks are bypassed: the library refuses, and clears its consumer
    for other in (masked, stepped):
        n0, n1 = other.extent
        v2, e2 = np.zeros((n0, n1, 5)), np.zeros((n0, n1), np.int32)
        cov = np.ascontiguousarray(other.coverage())
        rc = g.match_region(other._handle, 0, 1, n0, 0, 1, n1, v2.ctypes.data, 5, None, e2.ctypes.data, cov.ctypes.data, 0.1,
                            None, None, None, 0, None)
        assert rc == -4 and "grid" in g.error(), (rc, g.error())
        a, b = other.match(quiet=True), other.match(quiet=True)
        _same(a, b, what="walk after a refused grid match")
    k = hip_ns.UMPAModelDFKernel(sam, ref, window_size=Nw, max_shift=ms)
    n0, n1 = k.extent
    with pytest.raises(RuntimeError, match="grid"):
        k.match(abc=np.full((n0, n1, 3), 0.05), quiet=True, search="grid")
    assert not hasattr(k, "cost_volume")
    # the consumer was cleared: grid, then the walk again
    m.match(quiet=True, search="grid")
    m.cost_volume()
    after = m.match(quiet=True)
    _same(before, after, what="walk after grid")


def test_cost_volume_flags(hip_ns):
    """umpa_grid_cost_volume takes UMPA_HIP_F_DEVICE_IO and UMPA_HIP_F_USE_STAGED; every other flag is refused by name before
    anything runs, and the staged flag without a staged stack by the match entry point underneath.  (What the volume of an
    adopted stack IS: tests/test_hip_longlived.py.)"""
    from umpa_amd import _lib
    sam, ref, c = GE.stack("64x72x3")
    m = _model(hip_ns, 1, sam, ref, c["Nw"], c["ms"])
    before = m.cost_volume()["cost"]
    g = _lib.grid()
    N0, N1 = m.extent
    U = 2 * c["ms"] - 1
    vol = np.zeros((U, U, N0, N1))
    call = lambda flags: g.cost_volume(m._handle, 0, 1, N0, 0, 1, N1, vol.ctypes.data, None, None, flags, None)
    for flags in (_lib.F_FORCE_DIRECT, _lib.F_FORCE_TILED, _lib.F_PLANAR, _lib.F_REUSE_REF_MAPS, _lib.F_ASYNC, _lib.F_FORCE_PLAIN_DIRECT,
                  _lib.F_USE_STAGED | _lib.F_ASYNC, _lib.F_DEVICE_IO | _lib.F_PLANAR, 256):
        assert call(flags) == -1, flags
        assert g.error() == "grid: cost_volume takes UMPA_HIP_F_DEVICE_IO, UMPA_HIP_F_USE_STAGED and no other flag", (flags, g.error())
    assert call(_lib.F_USE_STAGED) == -1 and "UMPA_HIP_F_USE_STAGED without a staged sample stack" in g.error(), g.error()
    assert (vol == 0).all()
    assert call(0) >= 0, g.error()                                    # the consumer was cleared, the model is as it was
    np.testing.assert_array_equal(vol, before)
    m.stage_sample(list(np.ascontiguousarray(1.25 * sam[::-1])))
    assert call(_lib.F_USE_STAGED) >= 0, g.error()                    # with a staged stack the flag is taken ...
    assert not np.array_equal(vol, before)
    assert call(_lib.F_USE_STAGED) == -1 and "without a staged sample stack" in g.error()      # ... once
    fresh = _model(hip_ns, 1, np.ascontiguousarray(1.25 * sam[::-1]), ref, c["Nw"], c["ms"])
    np.testing.assert_array_equal(vol, fresh.cost_volume()["cost"])
    m._use_staged = False                                             # (spent through the C ABI, past the Python bookkeeping)
    np.testing.assert_array_equal(m.cost_volume()["cost"], vol)
