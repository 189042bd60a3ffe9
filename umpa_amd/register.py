"""
Frame registration: ``libumpa_register.so`` (``include/umpa_register.h``, where the operation is defined).

The registration workflow of the reference's ``UMPA/align.py`` -- ``get_diff_pos(refs)`` for the diffuser positions of a
reference stack, ``get_new_sam_pos(T=...)`` for the sample positions of overlapping transmission maps, ``shift_data`` to
resample the frames -- rests on one distance, ``D(r) = sum w (a - alpha b(. - r))^2`` with the optimal scale ``alpha``,
followed by a 3 x 3 quadratic sub-pixel fit.  The reference evaluates ``D`` for every periodic shift with three
whole-frame FFTs; here it is evaluated on the GPU over a bounded box of shifts ``|r| <= max_shift`` (motor errors and
drift are a few pixels), as plain sums, periodic (``boundary='wrap'``, the reference's convention) or over the
overlapping part of the frames only (``boundary='overlap'``).  Everything after the sums is host arithmetic on
``(2 S + 1)^2`` numbers.  HIP only: there is no CPU fallback.

Left out: ``find_shift`` and ``get_new_diff_pos`` (speckle tracking with a large window: ``UMPA_normal`` plus
``solve_positions`` below express it), the reference's tuple-of-two-masks form of ``w``, ``numiter > 1``, plotting.
"""
import numpy as np

from . import _lib

__all__ = ["shift_sums", "shift_dist", "register", "Registration", "shift_best", "get_diff_pos", "overlap",
           "find_sam_shift", "get_new_sam_pos", "solve_positions", "shift_data", "fit3x3",
           "INTERIOR", "BORDER", "NO_FINITE", "MAX_SHIFT"]

BOUNDARY = {"wrap": 0, "overlap": 1}
MAX_SHIFT = _lib.REGISTER_MAX_SHIFT
EPSILON = 1e-10
INTERIOR, BORDER, NO_FINITE = 0, 1, 2
_CODE = {np.dtype(np.float64): 0, np.dtype(np.float32): 1, np.dtype(np.uint16): 2}


def _box(max_shift):
    s = (max_shift, max_shift) if np.isscalar(max_shift) else tuple(max_shift)
    if len(s) != 2 or any(int(v) != v or v < 0 for v in s):
        raise ValueError("max_shift must be a non-negative int or a pair of them, not %r" % (max_shift,))
    s = (int(s[0]), int(s[1]))
    if max(s) > MAX_SHIFT:
        raise ValueError("max_shift %r: the box of shifts is limited to +-%d (include/umpa_register.h)" % (s, MAX_SHIFT))
    return s


def _check_shapes(ash, bsh, wsh, S):
    if len(bsh) not in (2, 3):
        raise ValueError("b must be [H, W] or [K, H, W], not %r" % (bsh,))
    fr = tuple(bsh[-2:])
    if tuple(ash[-2:]) != fr or len(ash) not in (2, 3) or (len(ash) == 3 and (len(bsh) != 3 or ash[0] != bsh[0])):
        raise ValueError("a %r does not match b %r: a is [H, W] (shared) or [K, H, W]" % (tuple(ash), tuple(bsh)))
    if wsh is not None and (tuple(wsh[-2:]) != fr or len(wsh) not in (2, 3) or (len(wsh) == 3 and (len(bsh) != 3 or wsh[0] != bsh[0]))):
        raise ValueError("w %r does not match b %r: w is [H, W] (shared) or [K, H, W]" % (tuple(wsh), tuple(bsh)))
    if 2 * S[0] + 1 > fr[0] or 2 * S[1] + 1 > fr[1]:
        raise ValueError("a box of %d x %d shifts is wider than the frame of %d x %d pixels" % (2 * S[0] + 1, 2 * S[1] + 1, fr[0], fr[1]))


def shift_sums(a, b, w=None, max_shift=8, boundary="wrap", device=None):
    """The three planes ``P, Q, A`` of ``include/umpa_register.h`` over the box ``|ri| <= S0, |rj| <= S1``
    (``max_shift``: ``S`` or ``(S0, S1)``), entry ``[ri + S0, rj + S1]``::

        P(r) = sum_x w a b_r      Q(r) = sum_x w b_r^2      A(r) = sum_x w a^2        b_r(x) = b(x - r)

    ``b``: ``[H, W]`` or ``[K, H, W]``, float64 / float32 / uint16; ``a``: the same dtype, ``[H, W]`` (shared by all
    ``K`` pairs) or ``[K, H, W]``; ``w``: float64, finite and ``>= 0``, ``[H, W]`` or ``[K, H, W]``.  Host arrays give
    host arrays; HIP tensors (all of them on one device, contiguous) give HIP tensors, computed on the current stream.
    The planes are ``[K, U0, U1]``, or ``[U0, U1]`` for a 2-D ``b``."""
    if boundary not in BOUNDARY:
        raise ValueError("boundary must be 'wrap' or 'overlap', not %r" % (boundary,))
    S = _box(max_shift)
    lib = _lib.register()
    U = (2 * S[0] + 1, 2 * S[1] + 1)
    io = _lib.Side(b, a, w, device=device)
    if io.on_device:
        import torch
        code = {torch.float64: 0, torch.float32: 1, getattr(torch, "uint16", None): 2}.get(b.dtype)
        if code is None or a.dtype != b.dtype or (w is not None and w.dtype != torch.float64):
            raise ValueError("frames must be float64, float32 or uint16 (a and b alike), weights float64.")
    else:
        a, b = np.asarray(a), np.asarray(b)
        code = _CODE.get(b.dtype)
        if code is None or a.dtype != b.dtype:
            raise ValueError("frames must be float64, float32 or uint16 (a and b alike), not %s and %s." % (a.dtype, b.dtype))
        if w is not None:
            w = np.ascontiguousarray(w, dtype=np.float64)
    _check_shapes(a.shape, b.shape, None if w is None else w.shape, S)
    if not io.on_device:                                              # (on tensors the kernels define what a bad weight does)
        if w is not None and not (np.isfinite(w).all() and (w >= 0).all()):
            raise ValueError("weights must be finite and >= 0")
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    shared = (_lib.REGISTER_F_SHARED_A if len(a.shape) == 2 else 0) | (_lib.REGISTER_F_SHARED_W if w is not None and len(w.shape) == 2 else 0)
    tail = io.tail(shared)
    batch = len(b.shape) == 3
    K = b.shape[0] if batch else 1
    out = io.empty((3, K) + U, np.float64)
    rc = lib.sums(io.ptr(a), io.ptr(b), io.ptr(w), code, K, b.shape[-2], b.shape[-1], S[0], S[1], BOUNDARY[boundary],
                  io.ptr(out[0]), io.ptr(out[1]), io.ptr(out[2]), *tail)
    lib.check(rc, "register sums")
    return tuple(out[i] if batch else out[i, 0] for i in range(3))


def _host(t):
    return t.cpu().numpy() if hasattr(t, "data_ptr") else t


def distance(P, Q, A, eps):
    """``(D, alpha) = (A - P^2 / (Q + eps), P / (Q + eps))``"""
    with np.errstate(divide="ignore", invalid="ignore"):
        alpha = P / (Q + eps)
        return A - P * P / (Q + eps), alpha


def shift_dist(a, b, w=None, max_shift=8, boundary="wrap", device=None):
    """``(cc, coeff)`` over the box: the distance ``D(r) = sum_x w (a - alpha b_r)^2`` at the optimal scale, and that scale
    ``alpha(r)``.  ``eps = 1e-10`` in the denominator when weights are given or the boundary is ``'overlap'``, 0 in the
    unweighted periodic case (the two branches of the reference's formula with real input)."""
    P, Q, A = (_host(t) for t in shift_sums(a, b, w, max_shift, boundary, device))
    return distance(P, Q, A, EPSILON if (w is not None or boundary == "overlap") else 0.0)


def fit3x3(z):
    """The sub-pixel minimum of ``include/umpa_register.h`` on ``z[u + 1, v + 1]``, ``u, v = -1, 0, 1``: ``((u*, v*),
    value)``.  The least-squares paraboloid where it is a minimum, the two parabolas through the centre column and the
    centre row otherwise."""
    z = np.asarray(z, dtype=np.float64)
    u = np.array([-1.0, 0.0, 1.0])
    c1 = (u[:, None] * z).sum() / 6.0
    c2 = (u[None, :] * z).sum() / 6.0
    c5 = (u[:, None] * u[None, :] * z).sum() / 4.0
    c3 = ((u[:, None] ** 2 - 2.0 / 3.0) * z).sum() / 2.0
    c4 = ((u[None, :] ** 2 - 2.0 / 3.0) * z).sum() / 2.0
    c0 = z.sum() / 9.0 - 2.0 * (c3 + c4) / 3.0
    det = 4.0 * c3 * c4 - c5 * c5
    if c3 > 0 and c4 > 0 and det > 0:
        us = -(2.0 * c4 * c1 - c5 * c2) / det
        vs = -(2.0 * c3 * c2 - c5 * c1) / det
        return np.array([us, vs]), c0 + 0.5 * (c1 * us + c2 * vs)

    def parabola(m, c, p):
        curv = p + m - 2.0 * c
        if not curv > 0:
            return 0.0, c
        x = -(p - m) / (2.0 * curv)
        return x, c - 0.125 * (p - m) ** 2 / curv

    us, d0 = parabola(z[0, 1], z[1, 1], z[2, 1])
    vs, d1 = parabola(z[1, 0], z[1, 1], z[1, 2])
    return np.array([us, vs]), max(d0, d1)


class Registration:
    """``shift``: the (row, col) shift ``r*`` that minimises ``D(r) = sum w (a(x) - alpha b(x - r))^2``, sub-pixel where
    ``status == INTERIOR``; ``alpha``: the scale at the integer minimum; ``mindist``: the fitted minimum of ``D`` (its
    value at the integer minimum where nothing was fitted); ``status``; ``cc``: ``D`` over the box.  For a batch every
    field is an array over the pairs.

    ``status``: ``INTERIOR`` -- an interior minimum, fitted.  ``BORDER`` -- the minimum lies on the border of the box (or
    next to a non-finite value): the integer shift, no fit; widen the box.  ``NO_FINITE`` -- no finite value of ``D``: a
    NaN or infinity in a frame poisons every sum it touches, in the periodic case all of them; ``shift`` is NaN."""

    def __init__(self, shift, alpha, mindist, status, cc):
        self.shift, self.alpha, self.mindist, self.status, self.cc = shift, alpha, mindist, status, cc

    def __repr__(self):
        return "Registration(shift=%r, alpha=%r, mindist=%r, status=%r)" % (self.shift, self.alpha, self.mindist, self.status)


def locate(cc, coeff):
    """The minimum of one box ``cc`` (host arithmetic): ``(shift, alpha, mindist, status)``."""
    S0, S1 = cc.shape[0] // 2, cc.shape[1] // 2
    fin = np.isfinite(cc)
    if not fin.any():
        return np.array([np.nan, np.nan]), np.nan, np.nan, NO_FINITE
    i, j = np.unravel_index(np.argmin(np.where(fin, cc, np.inf)), cc.shape)      # the first minimum, rows first
    r = np.array([i - S0, j - S1], dtype=np.float64)
    if i == 0 or j == 0 or i == cc.shape[0] - 1 or j == cc.shape[1] - 1 or not fin[i - 1:i + 2, j - 1:j + 2].all():
        return r, coeff[i, j], cc[i, j], BORDER
    off, val = fit3x3(cc[i - 1:i + 2, j - 1:j + 2])
    return r + off, coeff[i, j], val, INTERIOR


def register(a, b, w=None, max_shift=8, boundary="wrap", device=None):
    """Register ``b`` against ``a``: a ``Registration`` (of arrays, for ``b`` of ``[K, H, W]``).  The integer minimum is
    the first minimum of ``D`` over the box, rows first; the sub-pixel position is ``fit3x3`` of the 3 x 3 values around it."""
    cc, coeff = shift_dist(a, b, w, max_shift, boundary, device)
    if cc.ndim == 2:
        return Registration(*locate(cc, coeff), cc)
    rows = [locate(c, f) for c, f in zip(cc, coeff)]
    return Registration(np.array([r[0] for r in rows]).reshape(-1, 2), np.array([r[1] for r in rows]), np.array([r[2] for r in rows]),
                        np.array([r[3] for r in rows], dtype=np.int64), cc)


def _pshift_linear(b, r):
    """``out(x) = b(x - r)``, periodic, bilinear"""
    f = np.floor(-r).astype(int)
    t = -r - f
    out = np.zeros_like(b, dtype=np.float64)
    for c0, w0 in ((0, 1.0 - t[0]), (1, t[0])):
        for c1, w1 in ((0, 1.0 - t[1]), (1, t[1])):
            out += (w0 * w1) * np.roll(b, (-(f[0] + c0), -(f[1] + c1)), axis=(0, 1))
    return out


def shift_best(a, b, w=None, max_shift=8, return_params=True, device=None):
    """The reference's ``shift_best``: ``(b', -r*, alpha)`` -- ``b' = alpha b(. - r*)``, resampled with periodic bilinear
    interpolation on the host, the translation with the reference's sign, and the scale ``alpha = sum a b(. - r*) / sum
    b(. - r*)^2`` of the resampled frame.  ``r*`` comes from ``register`` on the periodic box ``|r| <= max_shift``."""
    a, b = np.asarray(a), np.asarray(b)
    reg = register(a, b, w, max_shift, "wrap", device)
    if reg.status == NO_FINITE:
        raise RuntimeError("shift_best: no finite value of the distance (non-finite pixels in a frame)")
    bs = _pshift_linear(b.astype(np.float64), reg.shift)
    alpha = float((a.astype(np.float64) * bs).sum() / (bs * bs).sum())
    shift_best.mindist = reg.mindist
    return (alpha * bs, -reg.shift, alpha) if return_params else alpha * bs


def wrap_centred(x, size):
    """``x`` modulo ``size`` (per axis), into ``[-size / 2, size / 2)``: ``x - size * floor(x / size + 1 / 2)``"""
    x, size = np.asarray(x, dtype=np.float64), np.asarray(size, dtype=np.float64)
    return x - size * np.floor(x / size + 0.5)


def get_diff_pos(refs, max_shift=8, device=None):
    """Diffuser positions ``[K, 2]`` (row, col) of a reference stack: every frame registered against ``refs[0]`` in one
    batched call, ``-r*`` wrapped to ``[-size / 2, size / 2)`` and rounded to 0.01 as the reference does."""
    refs = np.asarray(refs)
    reg = register(refs[0], refs, None, max_shift, "wrap", device)
    if (reg.status == NO_FINITE).any():
        raise RuntimeError("get_diff_pos: no finite value of the distance for frame(s) %s" % np.flatnonzero(reg.status == NO_FINITE))
    return np.round(wrap_centred(-reg.shift, refs.shape[-2:]), 2)


def overlap(mpos, size):
    """``(d0, d1, ov)`` for frame positions ``mpos`` (``[N, 2]``): ``d0[i, j]``, ``d1[i, j]`` the row and column distance
    from frame ``j`` to frame ``i``, ``ov[i, j]`` the fraction of a frame of ``size`` that the two share once the distance
    is rounded to whole pixels: ``prod_axis max(0, size - |round(d)|) / prod_axis size``."""
    mpos = np.asarray(mpos, dtype=np.float64)
    delta = mpos[:, None, :] - mpos[None, :, :]                       # [N, N, 2]
    size = np.asarray(size, dtype=np.float64)
    common = np.maximum(size - np.abs(np.rint(delta)), 0.0)
    return delta[..., 0], delta[..., 1], common.prod(axis=-1) / size.prod()


def common_region(shape, step):
    """Two frames of ``shape``, the second displaced by the integer ``step`` (row, col) on the sample: the slices of the
    first and of the second that show the same sample pixels.  Per axis the first frame's pixel ``x`` is the second's
    ``x - step``, so the intersection of ``[0, n)`` and ``[step, n + step)`` in the first, shifted by ``-step`` in the second."""
    first, second = [], []
    for n, s in zip(shape, step):
        lo, hi = max(0, s), min(n, n + s)
        first.append(slice(lo, hi))
        second.append(slice(lo - s, hi - s))
    return tuple(first), tuple(second)


def find_sam_shift(T, sample_pos=None, max_shift=8, p=99.9, device=None):
    """Shifts between consecutive maps ``T[i]``, ``T[i + 1]`` (a list of ``[row, col]``, the first ``[0, 0]``): the maps
    are cropped to their common region from the rounded difference of ``sample_pos``, outliers above the ``p``-th
    percentile of each crop are repaired (``correct_bad_pixels``), and the crops are registered periodically.
    ``p`` may be a sequence, one value per pair.  (Two things the reference does differently, both slips of its loop: its
    loop variable shadows ``p``, so it thresholds pair ``i`` at the ``i``-th percentile -- ``p=0`` reproduces its result
    for two maps, the only form ``get_new_sam_pos`` uses --, and it overwrites the frame shape with the last crop's, so
    from the second pair of a longer chain on it crops less than the common region.  Neither is reproduced.)"""
    from .align import correct_bad_pixels
    T = [np.asarray(t, dtype=np.float64) for t in T]
    n = len(T)
    pos = np.zeros((n, 2)) if sample_pos is None else np.asarray(sample_pos, dtype=np.float64)
    steps = np.rint(pos[1:] - pos[:-1]).astype(int)
    ps = [float(p)] * (n - 1) if np.isscalar(p) else [float(v) for v in p]
    shift = [np.array([0.0, 0.0])]
    for i in range(n - 1):
        first, second = common_region(T[i].shape, steps[i])
        crops = []
        for im in (T[i][first], T[i + 1][second]):
            crops.append(correct_bad_pixels(im, th=np.percentile(im, ps[i]), device=device))
        reg = register(crops[0], crops[1], None, max_shift, "wrap", device)
        if reg.status == NO_FINITE:
            raise RuntimeError("find_sam_shift: no finite value of the distance for maps %d, %d" % (i, i + 1))
        shift.append(wrap_centred(reg.shift, crops[1].shape))
    return shift


def solve_positions(pairs, found, x0):
    """The positions ``x`` (``[N, 2]``) that minimise ``sum_pairs |x[j] - x[i] - found_ij|^2`` for ``pairs`` of ``(i, j)``:
    a linear least-squares problem, solved in closed form.  A common offset of all positions does not change the cost; the
    reference's BFGS never moves along it, so it keeps the mean of its start ``x0``.  The same gauge here:
    ``x = x0 + lstsq(A, d - A x0)``, the minimum-norm correction."""
    x0 = np.asarray(x0, dtype=np.float64)
    pairs = np.asarray(pairs, dtype=int).reshape(-1, 2)
    found = np.asarray(found, dtype=np.float64).reshape(-1, 2)
    Amat = np.zeros((len(pairs), len(x0)))
    Amat[np.arange(len(pairs)), pairs[:, 0]] = -1.0
    Amat[np.arange(len(pairs)), pairs[:, 1]] = 1.0
    if len(pairs) == 0:
        return x0.copy()
    return x0 + np.linalg.lstsq(Amat, found - Amat @ x0, rcond=None)[0]


def matching_pairs(sample_pos, size, ov_thr):
    ov = overlap(sample_pos, size)[2]
    n = len(ov)
    return [(i, j) for i in range(n) for j in range(i + 1, n) if ov[i, j] > ov_thr]


def get_new_sam_pos(T, sample_pos=None, ov_thr=0.5, max_shift=8, p=99.9, device=None):
    """Refined sample positions ``[N, 2]``: every pair of maps whose overlap at ``sample_pos`` exceeds ``ov_thr`` is
    registered (``find_sam_shift`` of the two), then ``solve_positions`` from ``sample_pos``."""
    T = [np.asarray(t, dtype=np.float64) for t in T]
    pos = np.zeros((len(T), 2)) if sample_pos is None else np.asarray(sample_pos, dtype=np.float64)
    pairs = matching_pairs(pos, T[-1].shape, ov_thr)
    found = [find_sam_shift([T[i], T[j]], pos[[i, j]], max_shift, p, device)[1] for i, j in pairs]
    return solve_positions(pairs, found, pos)


def shift_data(frames, shift_list, interp="cubic", device=None):
    """``out[k][x] = frames[k][x - shift_list[k]]`` with edge clamping (``scipy.ndimage.shift``'s sign and its
    ``mode='nearest'`` border), float64.  Each frame goes through a constant-displacement ``UnwarpMap``
    (``libumpa_unwarp.so``): the interpolant is that library's Catmull-Rom (``interp='cubic'``) or bilinear
    (``'linear'``) kernel, NOT scipy's prefiltered cubic spline; integer shifts copy pixels exactly.  The displacement
    is stored as float32."""
    from .unwarp import UnwarpMap
    frames = np.asarray(frames)
    shifts = np.asarray(shift_list, dtype=np.float64).reshape(-1, 2)
    if frames.ndim != 3 or len(shifts) != len(frames):
        raise ValueError("frames must be [K, H, W] with one (row, col) shift per frame, not %r and %r" % (frames.shape, shifts.shape))
    device = _lib.host_device(device)
    out = np.empty(frames.shape, dtype=np.float64)
    d0, d1 = np.empty(frames.shape[1:], np.float32), np.empty(frames.shape[1:], np.float32)
    for k in range(len(frames)):
        d0[...] = -shifts[k, 0]
        d1[...] = -shifts[k, 1]
        m = UnwarpMap(d0, d1, interp=interp, device=device)
        out[k] = m.apply(frames[k])[0]
        m.destroy()
    return out
