"""
The device-pointer entry points of the seven side libraries between canaries (tests/guarded.py): one guarded call each.

Every input array lies inside a larger tensor with guards of NaN, then of 1e300 (two rows and a wavefront long, so an overrun
lands in the test's own memory), every output array inside one of its own; the call runs on a side stream.  The outputs must
equal those of the same call on plain tensors bit for bit -- a read of a neighbouring byte that reached a result would change
it with the fill --, every guard must keep its bit pattern and every input its bits.  No tolerance appears in this file; what
the numbers ARE is the business of each library's own test module.

None of the seven headers documents an alignment requirement: umpa_ddf_blur chooses its 16-byte kernel on the host from the
addresses of ALL frames of a launch and W's parity, the others (umpa_smooth_aggregate, umpa_sigma_region and umpa_sigma_solve
among them) load single elements.  So the misaligned calls are made, not refused.
"""
import ctypes

import numpy as np
import pytest

import guarded as G

pytestmark = pytest.mark.gpu

FILLS = {"nan": G.NAN_BITS, "1e300": G.BIG_BITS}
VP = ctypes.c_void_p


@pytest.fixture(scope="module")
def dev():
    import torch
    from umpa_amd import _lib
    if _lib.hip().device_count() < 1:
        pytest.fail("no HIP device: the GPU tests cannot run (there is no CPU fallback)")
    return torch.device("cuda", 0)


class Arrays:
    """The arrays of one call: plain tensors (guard None), or embedded ones"""

    def __init__(self, dev, fill=None, odd=False):
        self.dev, self.fill, self.odd, self.handles = dev, fill, odd, []

    def _put(self, arrays, row, inputs):
        import torch
        ts = [a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, order="C")) for a in arrays]
        if self.fill is None:
            return [t.to(self.dev).clone() for t in ts]
        fill = self.fill
        if ts[0].dtype != torch.float64:                               # the second pass of the narrower types: 1e30f, a finite integer
            second = 0x7149F2CA if ts[0].dtype == torch.float32 else 0x3C3C3C3C
            fill = None if self.fill == G.NAN_BITS else second         # (None: guarded.default_fill, NaN / INT32_FILL)
        views, h = G.embed(ts, G.min_guard(row) + (1 if self.odd else 0), fill, device=self.dev, inputs=inputs)
        self.handles.append(h)
        return views

    def inp(self, arrays, row):
        return self._put(arrays, row, True)

    def out(self, arrays, row):
        return self._put(arrays, row, False)

    def check(self, what):
        for n, h in enumerate(self.handles):
            G.check(h, "%s: embedding %d" % (what, n))


def _on_side_stream(dev, fn):
    import torch
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        out = fn(VP(stream.cuda_stream))
    stream.synchronize()
    return out


def _guarded_equals_plain(dev, call, what, odd=(False,)):
    """call(arrays, stream) -> list of output tensors.  The plain call first, then the guarded ones."""
    want = [t.cpu().numpy() for t in _on_side_stream(dev, lambda s: call(Arrays(dev), s))]
    for name, fill in FILLS.items():
        for o in odd:
            A = Arrays(dev, fill, o)
            got = [t.cpu().numpy() for t in _on_side_stream(dev, lambda s: call(A, s))]
            tag = "%s, %s guards%s" % (what, name, ", odd element offsets" if o else "")
            A.check(tag)
            assert len(got) == len(want)
            for q, (g, w) in enumerate(zip(got, want)):
                assert g.dtype == w.dtype and g.shape == w.shape
                assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), "%s: output %d differs from the call on plain tensors at %d elements" % (
                    tag, q, int((~((g == w) | ((g != g) & (w != w)))).sum()))
    return want


def _table(tensors):
    t = (VP * len(tensors))()
    for k, x in enumerate(tensors):
        t[k] = x.data_ptr()
    return t


# ----------------------------------------------------------------------------- umpa_ddf_blur / umpa_ddf_fold

def _blur_call(dev, frames, g, alternate=False):
    from umpa_amd import _lib
    lib = _lib.ddf()
    K, H, W = frames.shape

    def call(A, stream):
        fin = A.inp(list(frames), W)
        fout = A.out([np.zeros((H, W))] * K, W)
        if alternate and A.fill is not None:
            assert sorted({f.data_ptr() % 16 for f in fin}) == [0, 8] and W % 2 == 0
        lib.check(lib.blur(_table(fin), _table(fout), K, H, W, g.ctypes.data_as(VP), 0, _lib.F_DEVICE_IO, stream), "ddf blur")
        return fout
    return call


@pytest.mark.parametrize("shape", [(49, 131), (70, 150)], ids=["49x131_scalar", "70x150_vector"])
def test_ddf_blur(dev, shape):
    """49 x 131: odd W, the scalar kernel; 70 x 150 between even guards: every frame 16-byte aligned, the 16-byte kernel"""
    from umpa_amd import ddf
    g = ddf.gaussian_kernel(0.5, 0.2, 0.3)
    frames = 1.0 + 0.3 * np.random.default_rng(3).standard_normal((3,) + shape)
    want = _guarded_equals_plain(dev, _blur_call(dev, frames, g), "ddf blur %r" % (shape,))
    for k in range(3):                                                # the border is the input, the interior is not
        assert np.array_equal(want[k][:8], frames[k][:8]) and np.array_equal(want[k][:, -8:], frames[k][:, -8:])
        assert not np.array_equal(want[k][8:-8, 8:-8], frames[k][8:-8, 8:-8])


def test_ddf_blur_of_a_launch_that_mixes_alignments(dev):
    """70 x 150 (W even), frames alternately at 8 and 0 mod 16: the host's choice between the 16-byte and the scalar kernel
    is made once for the launch and must hold for every frame of it; the result is the aligned launch's bit for bit."""
    from umpa_amd import ddf
    g = ddf.gaussian_kernel(0.5, 0.2, 0.3)
    frames = 1.0 + 0.3 * np.random.default_rng(3).standard_normal((3, 70, 150))
    _guarded_equals_plain(dev, _blur_call(dev, frames, g, alternate=True), "ddf blur, mixed alignment", odd=(True,))


def test_ddf_fold(dev):
    """the hand-made planes of tests/ddf_expect.py, 63 pixels (no multiple of the 256 lanes of a workgroup), candidate after
    candidate into guarded best planes"""
    import ddf_expect as DE
    from umpa_amd import _lib
    lib = _lib.ddf()
    planes = DE.hand_made_planes()
    N = planes[0]["f"].size
    assert N % 256 != 0

    def call(A, stream):
        best = A.out([np.zeros(N)] * 4, N) + A.out([np.zeros(N, np.int32)] * 2, N)
        for m, p in enumerate(planes):
            cand = A.inp([p[k].ravel() for k in ("f", "T", "dx", "dy")], N) + A.inp([p["err"].ravel()], N)
            lib.check(lib.fold(m, N, *[VP(x.data_ptr()) for x in cand], *[VP(x.data_ptr()) for x in best], 0, _lib.F_DEVICE_IO, stream), "ddf fold")
        return best

    got = _guarded_equals_plain(dev, call, "ddf fold")
    want = DE.fold(planes)
    for q, k in enumerate(("f", "T", "dx", "dy", "index", "err")):
        assert np.array_equal(got[q].reshape(want[k].shape), want[k], equal_nan=True), k


# ----------------------------------------------------------------------------- umpa_register_sums

@pytest.mark.parametrize("dtype", [np.uint16, np.float32, np.float64], ids=["u16", "f32", "f64"])
def test_register_sums(dev, dtype):
    """70 x 83, boxes of +-8 and +-32 shifts, weighted and plain, both boundaries; uint16 frames also at an odd element
    offset (2 mod 4 bytes)"""
    import torch
    import register_expect as RE
    from umpa_amd import _lib
    lib = _lib.register()
    H, W = 70, 83
    a, b = RE.make_pair((H, W), 5, (2.37, -3.58))
    a, b = RE.as_dtype(a, dtype), RE.as_dtype(b, dtype)
    w = RE.weights((H, W), 5)
    code = {np.uint16: 2, np.float32: 1, np.float64: 0}[dtype]
    tt = lambda x: torch.from_numpy(x.view(np.int16)).view(torch.uint16) if dtype == np.uint16 else torch.from_numpy(x)
    for S in (8, 32):
        for weighted in (False, True):
            for boundary in (0, 1):
                U = 2 * S + 1

                def call(A, stream):
                    fa, fb = A.inp([tt(a), tt(b)], W)
                    fw = A.inp([w], W)[0] if weighted else None
                    out = A.out([np.zeros((U, U))] * 3, U)
                    if A.odd:
                        assert fa.data_ptr() % 4 == 2
                    lib.check(lib.sums(VP(fa.data_ptr()), VP(fb.data_ptr()), VP(fw.data_ptr()) if weighted else None, code, 1, H, W,
                                       S, S, boundary, *[VP(o.data_ptr()) for o in out], 0, _lib.F_DEVICE_IO, stream), "register sums")
                    return out

                got = _guarded_equals_plain(dev, call, "register sums %s +-%d weighted=%r boundary=%d" % (np.dtype(dtype).name, S, weighted, boundary),
                                            odd=(False, True) if dtype == np.uint16 else (False,))
                assert np.isfinite(got[0]).all() and (got[1] > 0).all()


# ----------------------------------------------------------------------------- umpa_integrate_solve / umpa_integrate_vcycle

@pytest.mark.parametrize("shape,kind", [((37, 130), "holes"), ((70, 73), "ones")], ids=["37x130_holes", "70x73"])
def test_integrate_solve_and_vcycle(dev, shape, kind):
    import integrate_expect as E
    from umpa_amd import _lib
    lib = _lib.integrate()
    H, W = shape
    gx, gy, w, _ = E.case(E.case_name(shape, kind))
    r = np.random.default_rng(17).standard_normal(shape)
    host = {}

    def solve(A, stream):
        fgx, fgy, fw = A.inp([gx, gy, w], W)
        (phi,) = A.out([np.zeros(shape)], W)
        it, st, res = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1)
        lib.check(lib.solve(VP(fgx.data_ptr()), VP(fgy.data_ptr()), VP(fw.data_ptr()), 1, H, W, 1e-10, 500, float("nan"), VP(phi.data_ptr()),
                            it.ctypes.data_as(VP), res.ctypes.data_as(VP), st.ctypes.data_as(VP), 0, _lib.F_DEVICE_IO, stream), "integrate solve")
        host.setdefault("solve", []).append((int(it[0]), float(res[0]), int(st[0])))
        return [phi]

    def vcycle(A, stream):
        fw, fr = A.inp([w, r], W)
        (z,) = A.out([np.zeros(shape)], W)
        lib.check(lib.vcycle(VP(fw.data_ptr()), VP(fr.data_ptr()), VP(z.data_ptr()), H, W, 0, _lib.F_DEVICE_IO, stream), "integrate vcycle")
        return [z]

    (phi,) = _guarded_equals_plain(dev, solve, "integrate solve %dx%d %s" % (H, W, kind))
    assert len(set(host["solve"])) == 1 and host["solve"][0][2] == _lib.INTEGRATE_CONVERGED, host["solve"]
    assert np.isfinite(phi[w > 0]).mean() > 0.9
    (z,) = _guarded_equals_plain(dev, vcycle, "integrate vcycle %dx%d %s" % (H, W, kind))
    assert np.isfinite(z).all() and np.abs(z).max() > 0


# ----------------------------------------------------------------------------- umpa_unwarp_frames

@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("dtype", [np.uint16, np.float32, np.float64], ids=["u16", "f32", "f64"])
def test_unwarp_frames(dev, dtype, interp):
    """37 x 71, the map whose coordinates land exactly on the last row and the last column"""
    import torch
    import unwarp_expect as UE
    from umpa_amd import UnwarpMap
    d0, d1 = UE.maps()["last_row_col"]
    umap = UnwarpMap(d0, d1, interp=interp)
    raw = UE.stack(dtype)
    dark, flat = UE.dark_flat()
    K, H, W = raw.shape
    tt = lambda x: torch.from_numpy(x.view(np.int16)).view(torch.uint16) if dtype == np.uint16 else torch.from_numpy(x)

    def call(A, stream):
        fraw = A.inp([tt(f) for f in raw], W)
        fdf = A.inp(list(dark) + list(flat), W)
        out = A.out([np.zeros((H, W))] * K, W)
        umap.apply_device(fraw, out, dark=fdf[:K], flat=fdf[K:], stream=stream)
        return out

    got = _guarded_equals_plain(dev, call, "unwarp frames %s %s" % (np.dtype(dtype).name, interp), odd=(False, True))
    assert np.isfinite(np.stack(got)).all()


# ----------------------------------------------------------------------------- umpa_grid_match_region / umpa_grid_cost_volume

@pytest.mark.parametrize("frames", ["owned", "borrowed"])
def test_grid_search_and_cost_volume(dev, frames):
    """the 64 x 72 x 3 stack of tests/grid_expect.py, dark-field model: every output array between guards, against the host-array
    calls of a model that owns its frames; the borrowed model's frames lie between NaN guards and stay untouched"""
    import grid_expect as GE
    from umpa_amd import _lib, model
    sam, ref, c = GE.stack("64x72x3")
    own = model.UMPAModelDF(sam, ref, window_size=c["Nw"], max_shift=c["ms"])
    host, vhost = own.match(quiet=True, search="grid"), own.cost_volume(with_fit=True)
    hs = None
    if frames == "owned":
        m = own
    else:
        views, hs = G.embed(list(sam) + list(ref), G.min_guard(c["W"]), G.NAN_BITS, device=dev)
        m = model.UMPAModelDF(views[:c["K"]], views[c["K"]:], window_size=c["Nw"], max_shift=c["ms"])
    N0, N1 = m.extent
    U = 2 * m.max_shift - 1
    g = _lib.grid()

    def call(A, stream):
        (values,) = A.out([np.zeros((N0, N1, 5))], 5 * N1)
        err, dn = A.out([np.zeros((N0, N1), np.int32)] * 2, N1)
        (dd,) = A.out([np.zeros((N0, N1, 25))], 25 * N1)
        (da,) = A.out([np.zeros((N0, N1, 16))], 16 * N1)
        vols = A.out([np.zeros((U, U, N0, N1))] * 3, N1)
        g.check(g.match_region(m._handle, 0, 1, N0, 0, 1, N1, values.data_ptr(), 5, None, err.data_ptr(), None, 0.0,
                               dd.data_ptr(), da.data_ptr(), dn.data_ptr(), _lib.F_DEVICE_IO, stream), "grid match_region")
        g.check(g.cost_volume(m._handle, 0, 1, N0, 0, 1, N1, vols[0].data_ptr(), vols[1].data_ptr(), vols[2].data_ptr(),
                              _lib.F_DEVICE_IO, stream), "grid cost_volume")
        return [values, err, dn, dd, da] + vols

    values, err, dn, dd, da, cost, T, df = _guarded_equals_plain(dev, call, "grid, %s frames" % frames)
    for q, k in enumerate(("f", "T", "dx", "dy", "df")):
        np.testing.assert_array_equal(values[..., q], host[k], err_msg=k)
    for k, x in (("err", err), ("debug_Ncalls", dn), ("debug_d", dd), ("debug_a", da)):
        np.testing.assert_array_equal(x, host[k], err_msg=k)
    for k, x in (("cost", cost), ("T", T), ("df", df)):
        np.testing.assert_array_equal(x, vhost[k], err_msg="volume " + k)
    if hs is not None:
        G.check(hs, "grid: the borrowed stack")


# ----------------------------------------------------------------------------- umpa_smooth_aggregate

@pytest.mark.parametrize("lean", [False, True], ids=["every_output", "shift_alone"])
def test_smooth_aggregate(dev, lean):
    """U = 5 on 21 x 37 pixels: off the 8 columns of the march and off the 32 x 32 tiles of the transpose in both directions,
    all eight directions (both transposed scratch volumes are in play; they are the library's own).  Once with shift, smin,
    margin, valid and total between guards, once with shift alone (the others null: the sum is then the library's own volume
    too).  The volume holds NaN and +-INF entries beside the NaN guards.  Guards sized by the longer side: the horizontal
    passes march over the transposed volume, whose rows are N0 long."""
    import smooth_expect as SE
    from umpa_amd import _lib
    lib = _lib.smooth()
    U, N0, N1, lam, trunc = 5, 21, 37, 0.5, 2.25
    cost = SE.with_specials(SE.random_volume(U, N0, N1, 11), 12)
    assert np.isnan(cost).any() and (cost == np.inf).any() and (cost == -np.inf).any()
    row = max(N0, N1)
    ptr = lambda t: None if t is None else VP(t.data_ptr())

    def call(A, stream):
        (fcost,) = A.inp([cost], row)
        (shift,) = A.out([np.zeros((2, N0, N1), np.int32)], row)
        smin = margin = valid = total = None
        if not lean:
            smin, margin = A.out([np.zeros((N0, N1))] * 2, row)
            (valid,) = A.out([np.zeros((N0, N1), np.int32)], row)
            (total,) = A.out([np.zeros((U, U, N0, N1))], row)
        if A.odd:
            assert fcost.data_ptr() % 16 == 8 and shift.data_ptr() % 8 == 4
        lib.check(lib.aggregate(ptr(fcost), U, N0, N1, lam, trunc, 0xFF, ptr(shift), ptr(smin), ptr(margin), ptr(valid), ptr(total),
                                dev.index, _lib.F_DEVICE_IO, stream), "smooth aggregate")
        return [shift] if lean else [shift, smin, margin, valid, total]

    got = _guarded_equals_plain(dev, call, "smooth aggregate, %s" % ("shift alone" if lean else "every output"), odd=(False, True))
    want = SE.aggregate(cost, lam, trunc, 0xFF)
    for g, k in zip(got, ("shift", "smin", "margin", "valid", "total")):
        np.testing.assert_array_equal(g, want[k], err_msg=k)
    assert want["valid"].min() == 0 and want["valid"].max() == 1


# ----------------------------------------------------------------------------- umpa_sigma_region / umpa_sigma_solve

@pytest.mark.parametrize("kind", [0, 1], ids=["plain", "dark_field"])
def test_sigma_region_and_solve(dev, kind):
    """the 3 x 40 x 44 stacks of tests/sigma_expect.py, Nw = 2, max_shift = 3, a region with an offset and a step whose 27 x 17
    pixels are off the 32 x 8 of the moments kernel; the shift field holds one skipped pixel and one shift far out of range at
    a corner.  Stacks and shift field are guarded inputs, every result a guarded output; once more with the moments null; then
    umpa_sigma_solve on the moments of the first call, 459 pixels (off the 256 of a workgroup)."""
    import sigma_expect as SG
    from umpa_amd import _lib
    lib = _lib.sigma()
    H, W, K, Nw, ms = 40, 44, 3, 2, 3
    reg = (1, 1, 27, 0, 2, 17)
    N0, N1, P = reg[2], reg[5], SG.PLANES[kind]
    sam, ref = SG.stack(H, W, K, ms, kind)
    assert sam.shape == (K, H, W)
    shift = SG.random_shift(N0, N1, ms, 33)
    shift[:, 5, 7] = SG.SKIP
    shift[:, N0 - 1, N1 - 1] = (-10 ** 6, 10 ** 6)
    skipped = ~SG.guard(shift, ms)
    assert skipped.sum() == 2
    win = SG.window(Nw)
    sv = SG.window_sv(win)
    ptr = lambda t: None if t is None else VP(t.data_ptr())

    def outputs(A, n_shape, row):
        (unit,) = A.out([np.zeros((3,) + n_shape)], row)
        s2, dof = A.out([np.zeros(n_shape)] * 2, row)
        (valid,) = A.out([np.zeros(n_shape, np.int32)], row)
        return unit, s2, dof, valid

    def region(with_moments):
        def call(A, stream):
            fsam, fref = A.inp([sam, ref], W)
            (fshift,) = A.inp([shift], N1)
            moments = A.out([np.zeros((P, N0, N1))], N1)[0] if with_moments else None
            unit, s2, dof, valid = outputs(A, (N0, N1), N1)
            if A.odd:
                assert fsam.data_ptr() % 16 == 8 and fshift.data_ptr() % 8 == 4
            lib.check(lib.region(ptr(fsam), ptr(fref), K, H, W, win.ctypes.data_as(VP), Nw, ms, kind, *reg, ptr(fshift), ptr(moments),
                                 ptr(unit), ptr(s2), ptr(dof), ptr(valid), dev.index, _lib.F_DEVICE_IO, stream), "sigma region")
            return ([moments] if with_moments else []) + [unit, s2, dof, valid]
        return call

    what = "sigma region, kind %d" % kind
    moments, unit, s2, dof, valid = _guarded_equals_plain(dev, region(True), what, odd=(False, True))
    lean = _guarded_equals_plain(dev, region(False), what + ", moments null", odd=(False, True))
    want = SG.solve(moments, kind, K, sv)
    for g, l, k in zip((unit, s2, dof, valid), lean, ("unit", "s2", "dof", "valid")):
        np.testing.assert_array_equal(l, g, err_msg=k + ", moments null")
        np.testing.assert_array_equal(g, want[k], err_msg=k)
    assert np.isnan(moments[:, skipped]).all() and np.isfinite(moments[:, ~skipped]).all()
    assert (valid[skipped] == 0).all() and valid[~skipped].mean() > 0.5

    n = N0 * N1
    assert n == 459 and n % 256 != 0
    flat = moments.reshape(P, n)

    def solve(A, stream):
        (fm,) = A.inp([flat], n)
        out = outputs(A, (n,), n)
        lib.check(lib.solve(ptr(fm), kind, K, n, sv, *[ptr(o) for o in out], dev.index, _lib.F_DEVICE_IO, stream), "sigma solve")
        return list(out)

    solved = _guarded_equals_plain(dev, solve, "sigma solve, kind %d" % kind, odd=(False, True))
    for g, r, k in zip(solved, (unit, s2, dof, valid), ("unit", "s2", "dof", "valid")):
        np.testing.assert_array_equal(g.reshape(r.shape), r, err_msg="solve: " + k)
