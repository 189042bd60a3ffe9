"""
Phase integration: ``libumpa_integrate.so`` (``include/umpa_integrate.h``, where the operation is defined).

``dx`` and ``dy`` of a match are the two components of the differential phase.  ``integrate`` solves the weighted
least-squares problem ``min sum_edges w_e (Phi_q - Phi_p - e)^2`` for the phase ``Phi`` on the GPU, by conjugate gradients
preconditioned with one geometric multigrid V-cycle.  Pixels of weight 0 (failed matches, masked detector areas) take no
part: they neither streak across the image, as they do with a Fourier integration, nor do NaNs in them reach the result.
HIP only: there is no CPU fallback.

The gauge is one global mean over the pixels that have a positive-weight edge; where zero-weight pixels cut the map into
several connected components, every component other than the largest keeps an arbitrary constant against it.
"""
import numpy as np

from . import _lib

__all__ = ["integrate", "vcycle", "phase_from_match", "Integration", "CONVERGED", "MAXITER", "BREAKDOWN"]

CONVERGED, MAXITER, BREAKDOWN = _lib.INTEGRATE_CONVERGED, _lib.INTEGRATE_MAXITER, _lib.INTEGRATE_BREAKDOWN


class Integration:
    """The result of ``integrate``: ``phi`` (``[H, W]`` or ``[K, H, W]``), and per map ``iterations``, ``residual`` (the
    true relative residual ``|b - L phi|_2 / |b|_2``) and ``status`` (``CONVERGED``, ``MAXITER`` or ``BREAKDOWN``); ints
    and floats for a single map, arrays for a batch."""
    CONVERGED, MAXITER, BREAKDOWN = CONVERGED, MAXITER, BREAKDOWN

    def __init__(self, phi, iterations, residual, status):
        self.phi, self.iterations, self.residual, self.status = phi, iterations, residual, status

    @property
    def converged(self):
        return bool(np.all(np.asarray(self.status) == CONVERGED))

    def __repr__(self):
        return "Integration(phi %r, iterations %r, residual %r, status %r)" % (tuple(self.phi.shape), self.iterations, self.residual, self.status)


def _check_shapes(gsh, other, wsh):
    if len(gsh) not in (2, 3):
        raise ValueError("gx must be [H, W] or [K, H, W], not %r" % (tuple(gsh),))
    if tuple(other) != tuple(gsh):
        raise ValueError("gy %r does not match gx %r" % (tuple(other), tuple(gsh)))
    if wsh is not None and tuple(wsh) != tuple(gsh):
        raise ValueError("weight %r does not match gx %r" % (tuple(wsh), tuple(gsh)))
    if gsh[-2] < 2 or gsh[-1] < 2:
        raise ValueError("maps of %d x %d pixels: at least 2 x 2" % (gsh[-2], gsh[-1]))


def _check_params(tol, maxiter):
    if not (np.isfinite(tol) and tol >= 0):
        raise ValueError("tol must be finite and >= 0, not %r" % (tol,))
    if int(maxiter) != maxiter or maxiter < 0:
        raise ValueError("maxiter must be a non-negative int, not %r" % (maxiter,))


_MIXED = "device arrays must be contiguous HIP tensors on one device (host arrays and tensors are not mixed)"


def _typed(io, *arrays):
    """Host arrays as contiguous float64 copies; tensors as they are, which the caller refuses with ``_refuse``."""
    if io.on_device:
        return arrays
    return tuple(None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in arrays)


def _refuse(io, *arrays):
    """After the shapes: tensors of another dtype, host weights that are not finite and >= 0 (on tensors the library's
    kernels define what such a weight does)."""
    if io.on_device:
        for t in arrays:
            if t is not None and str(t.dtype) != "torch.float64":
                raise ValueError("gradients and weights must be float64, not %s" % t.dtype)
    else:
        weight = arrays[-1]
        if weight is not None and not (np.isfinite(weight).all() and (weight >= 0).all()):
            raise ValueError("weights must be finite and >= 0")


def _solve(gx, gy, weight, tol, maxiter, fill, device, flags):
    _check_params(tol, maxiter)
    lib = _lib.integrate()
    io = _lib.Side(gx, gy, weight, device=device, mixed=_MIXED)
    gx, gy, weight = _typed(io, gx, gy, weight)
    _check_shapes(gx.shape, gy.shape, None if weight is None else weight.shape)
    _refuse(io, gx, gy, weight)
    tail = io.tail(flags)
    single = len(gx.shape) == 2
    K = 1 if single else gx.shape[0]
    phi = io.empty(gx.shape, np.float64)
    it, st, res = np.zeros(K, dtype=np.int32), np.zeros(K, dtype=np.int32), np.zeros(K)
    rc = lib.solve(io.ptr(gx), io.ptr(gy), io.ptr(weight), K, gx.shape[-2], gx.shape[-1], float(tol), int(maxiter), float(fill),
                   io.ptr(phi), io.ptr(it), io.ptr(res), io.ptr(st), *tail)
    lib.check(rc, "integrate solve")
    if single:
        return Integration(phi, int(it[0]), float(res[0]), int(st[0]))
    return Integration(phi, it, res, st)


def _flags(no_tail, jacobi):
    return (_lib.INTEGRATE_F_NO_TAIL if no_tail else 0) | (_lib.INTEGRATE_F_JACOBI if jacobi else 0)


def integrate(gx, gy, weight=None, tol=1e-10, maxiter=500, fill=np.nan, device=None, no_tail=False, jacobi=False):
    """The phase ``Phi`` with ``dPhi/dj = gx`` (along the columns) and ``dPhi/di = gy`` (along the rows), in the weighted
    least-squares sense of ``include/umpa_integrate.h``, as an ``Integration``.

    ``gx``, ``gy``: ``[H, W]`` or ``[K, H, W]`` (``K`` independent maps), float64, in units of ``Phi`` per pixel;
    ``weight``: the same shape, finite and ``>= 0``.  A pixel whose weight is not ``> 0`` takes no part and its gradients may
    be anything; without ``weight`` these are the pixels with a non-finite gradient.  ``phi`` has its mean over the pixels
    with a positive-weight edge removed (one global mean, see the module text); pixels without such an edge receive
    ``fill``.  The solve stops when the true residual is at most ``tol |b|``, or after ``maxiter`` iterations.

    Host arrays give host arrays; HIP tensors (all on one device, contiguous) give a HIP tensor ``phi``, computed on the
    current stream.  ``no_tail`` launches every level of the V-cycle separately (the result is bit-identical), ``jacobi``
    replaces the V-cycle by the diagonal: both exist for tests and measurements."""
    return _solve(gx, gy, weight, tol, maxiter, fill, device, _flags(no_tail, jacobi))


def rhs(gx, gy, weight=None, device=None):
    """The right-hand side ``b`` of the normal equations (for the tests)."""
    return _solve(gx, gy, weight, 0.0, 0, 0.0, device, _lib.INTEGRATE_F_DEBUG).phi


def vcycle(r, weight=None, device=None, no_tail=False, jacobi=False, diagonal=False):
    """The preconditioner alone: ``z = M r`` for one ``[H, W]`` map on the hierarchy of ``weight`` (all 1 without it).
    ``diagonal=True`` returns the diagonal ``d`` of the fine operator instead (for the tests)."""
    lib = _lib.integrate()
    flags = _flags(no_tail, jacobi) | (_lib.INTEGRATE_F_DEBUG if diagonal else 0)
    io = _lib.Side(r, weight, device=device, mixed=_MIXED)
    r, weight = _typed(io, r, weight)
    if len(r.shape) != 2 or (weight is not None and weight.shape != r.shape):
        raise ValueError("r must be [H, W] and weight of the same shape")
    _refuse(io, r, weight)
    tail = io.tail(flags)
    z = io.empty(r.shape, np.float64)
    rc = lib.vcycle(io.ptr(weight), io.ptr(r), io.ptr(z), r.shape[0], r.shape[1], *tail)
    lib.check(rc, "integrate vcycle")
    return z


def match_weight(result, weight="err"):
    """The pixel weights ``phase_from_match`` derives from a ``match()`` dictionary."""
    dx, dy = np.asarray(result["dx"], dtype=np.float64), np.asarray(result["dy"], dtype=np.float64)
    if not isinstance(weight, str):
        w = np.asarray(weight, dtype=np.float64)
        if w.shape != dx.shape:
            raise ValueError("weight %r does not match the maps %r" % (w.shape, dx.shape))
        return w
    if weight not in ("err", "f"):
        raise ValueError("weight must be 'err', 'f' or an array, not %r" % (weight,))
    ok = (np.asarray(result["err"]) == 1) & np.isfinite(dx) & np.isfinite(dy)
    if weight == "err":
        return ok.astype(np.float64)
    f = np.asarray(result["f"], dtype=np.float64)
    ok &= np.isfinite(f) & (f >= 0)
    med = np.median(f[ok]) if ok.any() else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        conf = 1.0 / (f + med)
    return np.where(ok & np.isfinite(conf), conf, 0.0)


def phase_from_match(result, scale=1.0, weight="err", bias=None, **kw):
    """Integrate the ``dx``, ``dy`` maps of a ``match()`` dictionary: ``integrate(scale * (dx - dx0), scale * (dy - dy0), w)``.

    ``bias``: a pair ``(dx0, dy0)`` (numbers or maps) to subtract, e.g. the result of a sample-free match.  ``scale``
    converts pixels of displacement into phase per pixel: a displacement of ``dx`` pixels of size ``p`` at a distance ``z``
    between sample (or diffuser) and detector is a refraction angle ``dx p / z``, and ``dPhi/dx = (2 pi / lambda) * angle``
    per unit length, so per pixel ``scale = 2 pi p^2 / (lambda z)`` for the wavelength ``lambda``; with ``scale = 1`` the
    result is in units of pixels^2.  The sign follows the match's convention ``sam[i, j] = ref[i + dy, j + dx]``: ``phi``
    increases along ``+j`` where ``dx > 0``.

    ``weight='err'``: 1 where ``err == 1`` and both maps are finite, else 0.  ``weight='f'``: that times the confidence
    ``1 / (f + median f)`` of the match's residual ``f``.  An array is used as it is.  Further keywords go to ``integrate``."""
    dx, dy = np.asarray(result["dx"], dtype=np.float64), np.asarray(result["dy"], dtype=np.float64)
    w = match_weight(result, weight)
    dx0, dy0 = (0.0, 0.0) if bias is None else bias
    with np.errstate(invalid="ignore"):
        gx, gy = scale * (dx - dx0), scale * (dy - dy0)
    return integrate(gx, gy, w, **kw)
