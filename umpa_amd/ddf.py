"""
Directional dark-field: the search for the blur kernel of the kernel dark-field model among candidates, on
``libumpa_ddf.so`` (``include/umpa_ddf.h``, where the operations are defined).

``UMPAModelDFKernel`` describes the sample as the reference blurred by a 17 x 17 Gaussian ``exp(-a i^2 - b i j - c j^2)``
(``i``: rows, ``j``: columns); the strength and the direction of the scattering are read from ``(a, b, c)``, which that model
takes as an input.  ``KernelSearch`` finds it: for every candidate it blurs the reference stack once as a whole image, runs
the plain match (``UMPAModelNoDF``) of the sample against the blurred stack, and keeps per pixel the candidate of the lowest
cost.  With ``(a, b, c)`` the same for every pixel that plain match IS the kernel model's match (the blurred value a window
asks for does not depend on which window asks), at the price of one convolution per candidate instead of 289 taps per
window pixel of every cost call.  HIP only: there is no CPU fallback.

Widths and angle.  The kernel is ``exp(-x' A x / 2)`` with ``A = [[2a, b], [b, 2c]]`` and ``x = (i, j)``; its covariance is
the inverse of ``A``.  ``sigma_major >= sigma_minor`` are the square roots of the covariance's eigenvalues (pixels) and
``theta`` is the direction of the major axis measured from the row axis ``i`` towards the column axis ``j``, in ``[0, pi)``:
``theta = 0`` is a blur along the rows (vertical in the image), ``pi / 2`` one along the columns.  An isotropic kernel has
``theta = 0``.
"""
import ctypes as C
import time

import numpy as np

from . import _lib, model

__all__ = ["gaussian_kernel", "kernel_from_sigma", "sigma_from_kernel", "candidate_grid", "check_candidates", "blur_frames",
           "fold", "KernelSearch", "TAPS", "HALF"]

TAPS, HALF = _lib.DDF_TAPS, _lib.DDF_HALF
_ptr = _lib.Side.ptr


def _admissible(a, b, c):
    return bool(np.isfinite(a) and np.isfinite(b) and np.isfinite(c) and a > 0 and c > 0 and 4.0 * a * c - b * b > 0)


def check_candidates(candidates):
    """The candidate list as a ``[M, 3]`` float64 array; ``ValueError`` for an empty list, a wrong shape or a candidate
    that is no Gaussian (finite, ``a > 0``, ``c > 0``, ``4 a c - b^2 > 0``)."""
    cand = np.asarray(candidates, dtype=np.float64)
    if cand.size == 0:
        raise ValueError("the candidate list is empty")
    if cand.ndim == 1 and cand.shape[0] == 3:
        cand = cand[None, :]
    if cand.ndim != 2 or cand.shape[1] != 3:
        raise ValueError("candidates must be [M, 3] rows (a, b, c), not %r" % (cand.shape,))
    for m, (a, b, c) in enumerate(cand):
        if not _admissible(a, b, c):
            raise ValueError("candidate %d, (a, b, c) = (%r, %r, %r), is inadmissible: finite values with a > 0, c > 0 and "
                             "4 a c - b^2 > 0 are required" % (m, a, b, c))
    return np.ascontiguousarray(cand)


def gaussian_kernel(a, b, c):
    """The normalised 17 x 17 kernel ``g[k, l] = exp(-a (k-8)^2 - b (k-8)(l-8) - c (l-8)^2) / sum`` (``k``: row) of
    ``include/umpa_ddf.h``, computed by the library's host function in double."""
    if not _admissible(a, b, c):
        raise ValueError("(a, b, c) = (%r, %r, %r) is inadmissible: finite values with a > 0, c > 0 and 4 a c - b^2 > 0 "
                         "are required" % (a, b, c))
    lib = _lib.ddf()
    g = np.empty((TAPS, TAPS), dtype=np.float64)
    lib.check(lib.kernel(float(a), float(b), float(c), _ptr(g)), "ddf kernel")
    return g


def kernel_from_sigma(s_major, s_minor, theta):
    """``(a, b, c)`` of the Gaussian with the widths ``s_major >= s_minor > 0`` (pixels) and the major axis at ``theta``
    from the row axis (module text).  Numbers or arrays."""
    s_major, s_minor, theta = np.asarray(s_major, dtype=np.float64), np.asarray(s_minor, dtype=np.float64), np.asarray(theta, dtype=np.float64)
    if np.any(~(s_minor > 0)) or np.any(~(s_major >= s_minor)) or np.any(~np.isfinite(s_major)):
        raise ValueError("widths must be finite with s_major >= s_minor > 0")
    p, q = 1.0 / (s_major * s_major), 1.0 / (s_minor * s_minor)      # the eigenvalues of A
    cs, sn = np.cos(theta), np.sin(theta)
    a = 0.5 * (cs * cs * p + sn * sn * q)
    c = 0.5 * (sn * sn * p + cs * cs * q)
    b = cs * sn * (p - q)
    if a.ndim == 0:
        return float(a), float(b), float(c)
    return a, b, c


def sigma_from_kernel(a, b, c):
    """The inverse of ``kernel_from_sigma``: ``(sigma_major, sigma_minor, theta)`` with ``theta`` in ``[0, pi)`` and 0 for
    an isotropic kernel.  Works on maps; NaN where an input is NaN or ``(a, b, c)`` is no Gaussian."""
    a, b, c = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        root = np.sqrt((a - c) * (a - c) + b * b)
        lo, hi = (a + c) - root, (a + c) + root                      # the eigenvalues of A = [[2a, b], [b, 2c]]
        ok = (a > 0) & (c > 0) & (4.0 * a * c - b * b > 0) & np.isfinite(a) & np.isfinite(b) & np.isfinite(c)
        s_major = np.where(ok, 1.0 / np.sqrt(lo), np.nan)
        s_minor = np.where(ok, 1.0 / np.sqrt(hi), np.nan)
        # the eigenvector of the larger eigenvalue of A lies at atan2(b, a - c) / 2; the major axis is across it
        theta = np.mod(0.5 * np.arctan2(b, a - c) + 0.5 * np.pi, np.pi)
        theta = np.where(theta >= np.pi, 0.0, theta)                 # mod() may round up to pi itself
        theta = np.where(ok, np.where(root == 0, 0.0, theta), np.nan)
    if s_major.ndim == 0:
        return float(s_major), float(s_minor), float(theta)
    return s_major, s_minor, theta


def candidate_grid(sigmas, ratios, n_angles):
    """Candidates ``[M, 3]``: for every major width of ``sigmas`` and every ``ratio = s_minor / s_major`` of ``ratios``
    (``0 < ratio <= 1``) the ``n_angles`` orientations ``theta = pi n / n_angles``; a ratio of 1 (isotropic) gives one."""
    sigmas, ratios = np.atleast_1d(np.asarray(sigmas, dtype=np.float64)), np.atleast_1d(np.asarray(ratios, dtype=np.float64))
    if int(n_angles) != n_angles or n_angles < 1:
        raise ValueError("n_angles must be a positive int, not %r" % (n_angles,))
    if sigmas.size == 0 or ratios.size == 0:
        raise ValueError("sigmas and ratios must not be empty")
    if np.any(~(sigmas > 0)) or np.any(~np.isfinite(sigmas)) or np.any(~(ratios > 0)) or np.any(~(ratios <= 1)):
        raise ValueError("sigmas must be finite and > 0, ratios in (0, 1]")
    rows = []
    for s in sigmas:
        for r in ratios:
            for n in range(1 if r == 1 else int(n_angles)):
                rows.append(kernel_from_sigma(s, s * r, np.pi * n / int(n_angles)))
    return check_candidates(rows)


def _table(ptrs):
    t = (C.c_void_p * len(ptrs))()
    for k, p in enumerate(ptrs):
        t[k] = p
    return t


def _blur(frames_in, frames_out, g, tail):
    lib = _lib.ddf()
    H, W = frames_in[0].shape
    rc = lib.blur(_table([_ptr(f) for f in frames_in]), _table([_ptr(f) for f in frames_out]), len(frames_in), H, W, _ptr(g), *tail)
    lib.check(rc, "ddf blur")


def _blur_device(frames_in, frames_out, g, dev, stream):
    _blur(frames_in, frames_out, g, (dev, _lib.F_DEVICE_IO, stream))


def blur_frames(frames, abc, device=None):
    """The frames blurred by the kernel of ``abc = (a, b, c)`` as ``include/umpa_ddf.h`` defines it: the convolution on the
    pixels at least 8 from every edge, the input unchanged on the border.  ``frames``: a ``[K, H, W]`` array or a list of
    ``[H, W]`` frames, ``H, W >= 17``; host arrays give a float64 ``[K, H, W]`` array, HIP tensors (float64, contiguous, one
    device) a tensor, computed on the current stream."""
    a, b, c = abc
    g = gaussian_kernel(a, b, c)
    single = hasattr(frames, "ndim") and frames.ndim == 2 or hasattr(frames, "dim") and frames.dim() == 2
    flist = [frames] if single else list(frames)
    if not flist:
        raise ValueError("no frames")
    io = _lib.Side(*flist, device=device)
    if io.on_device:
        import torch
        for f in flist:
            if not hasattr(f, "data_ptr") or f.dtype != torch.float64 or not f.is_cuda or not f.is_contiguous() or f.dim() != 2 \
                    or f.device != flist[0].device:
                raise ValueError("device frames must be contiguous 2-D float64 HIP tensors on one device")
    else:
        flist = [np.ascontiguousarray(f, dtype=np.float64) for f in flist]
    sh = tuple(flist[0].shape)
    if len(sh) != 2 or any(tuple(f.shape) != sh for f in flist):
        raise ValueError("frames of unequal shapes: %r" % ([tuple(f.shape) for f in flist],))
    if sh[0] < TAPS or sh[1] < TAPS:
        raise ValueError("frames of %d x %d pixels are smaller than the %d x %d kernel" % (sh[0], sh[1], TAPS, TAPS))
    tail = io.tail()
    out = io.empty((len(flist),) + sh, np.float64)
    _blur(flist, [out[k] for k in range(len(flist))], g, tail)
    return out[0] if single else out


_FOLD_DTYPES = ["float64"] * 4 + ["int32"] + ["float64"] * 4 + ["int32"] * 2


def fold(m, cand, best, device=None):
    """``umpa_ddf_fold``: candidate ``m``'s planes ``cand = (f, T, dx, dy, err)`` into ``best = (f, T, dx, dy, index, err)``,
    in place (float64 and int32 arrays of one size, C-contiguous): host arrays, or HIP tensors on the current stream."""
    lib = _lib.ddf()
    planes = list(cand) + list(best)
    n = int(np.prod(cand[0].shape))
    io = _lib.Side(*planes, device=device)
    for x, dt in zip(planes, _FOLD_DTYPES):
        if str(x.dtype).split(".")[-1] != dt or int(np.prod(x.shape)) != n or not (io.on_device or x.flags.c_contiguous):
            raise ValueError("fold planes must be C-contiguous float64 (int32: err, index) arrays of one size")
    rc = lib.fold(int(m), n, *[_ptr(x) for x in planes], *io.tail())
    lib.check(rc, "ddf fold")


class KernelSearch:
    """Per-pixel search of the kernel dark-field model's ``(a, b, c)`` among candidates (module text).

    ``sam_list``, ``ref_list``: frames of ONE shape, host arrays or float64 HIP tensors; no masks, no ``pos_list`` (the
    reference's masked model normalises the blur by the mask, which is no whole-image convolution).  The stacks are held
    on the device, with one blurred stack of the same shape and one ``UMPAModelNoDF`` that borrows the sample stack and the
    blurred stack as device frames; ``model.py`` lets the library keep its reference-side maps only for frames the library
    owns, so those maps are rebuilt for every candidate.

    ``match`` returns a dictionary with ``index`` (int32: the winning candidate, -1 where every candidate failed), the
    winner's ``a``, ``b``, ``c``, ``sigma_major``, ``sigma_minor``, ``theta`` (NaN where ``index < 0``) and its ``f``, ``T``,
    ``dx``, ``dy``, ``err``; extent, ROI / step semantics and coordinates are those of ``UMPAModelDFKernel`` on the same
    stacks, so ``np.stack([a, b, c], -1)`` can go into ``UMPAModelDFKernel.match(abc=...)``.  Pixels where all candidates
    failed keep the first candidate's maps.

    The candidates are ranked by ``f``, the cost the sub-pixel fit returns (``sub_pixel_mode`` -1 and 1).  With
    ``sub_pixel_mode = 0`` the plain model's ``f`` is the start offset ``1 - ip`` of the reference, 0 or 1, and no cost: the
    search then asks the plain model for its 5 x 5 memo, ranks the candidates by the memo's centre (``debug_d[..., 12]``, the
    cost at the candidate's own integer minimum) and returns that cost as ``f`` and ``f_all``.

    ``last_times`` holds the host-clock seconds the last ``match`` spent in
    the blurs, the plain matches and the folds."""

    def __init__(self, sam_list, ref_list, window_size=2, max_shift=4, device=None, mask_list=None, pos_list=None):
        if mask_list is not None:
            raise ValueError("KernelSearch takes no masks: the masked kernel model normalises the blur by the mask, which is no "
                             "whole-image convolution")
        if pos_list is not None:
            raise ValueError("KernelSearch takes no pos_list: frames at different positions (sample stepping) are not supported")
        sam_list, ref_list = list(sam_list), list(ref_list)
        if not sam_list or len(sam_list) != len(ref_list):
            raise ValueError("sam_list and ref_list must be two non-empty lists of one length")
        shapes = [tuple(x.shape) for x in sam_list + ref_list]
        if any(len(s) != 2 for s in shapes) or any(s != shapes[0] for s in shapes):
            raise ValueError("frames of unequal shapes are not supported: %r" % (sorted(set(shapes)),))
        H, W = shapes[0]
        if H < TAPS or W < TAPS:
            raise ValueError("frames of %d x %d pixels are smaller than the %d x %d kernel" % (H, W, TAPS, TAPS))
        self._Nw, self._max_shift = int(window_size), int(max_shift)
        self._padding = self._max_shift + self._Nw + HALF             # UMPAModelDFKernel's
        if H - 2 * self._padding < 1 or W - 2 * self._padding < 1:
            raise ValueError("frames of %d x %d pixels leave no pixel inside the padding %d of the kernel model" % (H, W, self._padding))
        import torch
        self._lib = _lib.ddf()
        if hasattr(sam_list[0], "data_ptr") and device is None:
            device = sam_list[0].device.index
        self._device = _lib.host_device(device)
        if _lib.hip().device_count() < 1:
            raise _lib.NativeError("no HIP device available (this library has no CPU fallback)")
        self._tdev = torch.device("cuda", self._device)
        self._shape = (H, W)
        self._sam = self._upload(sam_list)
        self._ref = self._upload(ref_list)
        self._blur = torch.empty_like(self._ref)
        K = len(sam_list)
        self._ref_frames = [self._ref[k] for k in range(K)]
        self._blur_frames = [self._blur[k] for k in range(K)]
        self._model = model.UMPAModelNoDF([self._sam[k] for k in range(K)], self._blur_frames, window_size=self._Nw,
                                          max_shift=self._max_shift, device=self._device)
        self.debug = False
        self.last_times = None

    def _upload(self, frames):
        import torch
        if hasattr(frames[0], "data_ptr"):
            return torch.stack([f.to(device=self._tdev, dtype=torch.float64) for f in frames]).contiguous()
        return torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(f, dtype=np.float64) for f in frames]))).to(self._tdev)

    # -- the kernel model's geometry (model.py: _calculate_extent, resolve_region)
    @property
    def padding(self):
        return self._padding

    @property
    def extent(self):
        return self._shape[0] - 2 * self._padding, self._shape[1] - 2 * self._padding

    def _region(self, ROI, step):
        """The models' ``resolve_region`` with this class's default: without ``ROI`` the whole extent taken with ``step``."""
        N0, N1 = self.extent
        return model.resolve_region((N0, N1), ROI, None if ROI is not None else step, ((0, N0, 1), (0, N1, 1)))[:2]

    def coords(self, ROI=None, step=None):
        s0, s1 = self._region(ROI, step)
        return self._padding + np.arange(*s0), self._padding + np.arange(*s1)

    @property
    def assign_coordinates(self):
        return self._model.assign_coordinates

    @assign_coordinates.setter
    def assign_coordinates(self, mode):
        self._model.assign_coordinates = mode

    @property
    def sub_pixel_mode(self):
        return self._model.sub_pixel_mode

    @sub_pixel_mode.setter
    def sub_pixel_mode(self, mode):
        self._model.sub_pixel_mode = mode

    def match(self, candidates, ROI=None, step=None, keep=False):
        """Search ``candidates`` (``[M, 3]`` rows ``(a, b, c)``) on the region ``ROI`` (``step`` is ignored beside it, as in
        the models).  ``keep=True`` adds ``f_all`` and ``err_all``, ``[M, N0, N1]``: every candidate's cost and flag.  With
        the attribute ``debug`` set (as the models', e.g. ``True`` or ``"ncalls"``) the result also carries the winning
        candidate's ``debug_*`` arrays."""
        import torch
        cand = check_candidates(candidates)
        s0, s1 = self._region(ROI, step)
        roi = ((s0[0] + HALF, s0[1] + HALF, s0[2]), (s1[0] + HALF, s1[1] + HALF, s1[2]))   # the plain model's pixels
        M = len(cand)
        # mode 0: the plain model's f is the start offset 1 - ip, no cost; the cost of the integer minimum is the centre
        # of the 5 x 5 memo, so the plain model is asked for the memo whatever `debug` says
        mode0 = self.sub_pixel_mode == 0
        self._model.debug = True if mode0 and (not self.debug or self.debug == "ncalls") else self.debug
        stream = torch.cuda.current_stream(self._tdev).cuda_stream
        best = None
        f_all = err_all = None
        dbg = {}
        times = self.last_times = dict(blur=0.0, match=0.0, fold=0.0)   # host clock, seconds; every phase ends synchronised
        for m, (a, b, c) in enumerate(cand):
            t0 = time.perf_counter()
            _blur_device(self._ref_frames, self._blur_frames, gaussian_kernel(a, b, c), self._device, stream)
            t1 = time.perf_counter()
            res = self._model.match(ROI=roi, quiet=True)
            t2 = time.perf_counter()
            times["blur"] += t1 - t0
            times["match"] += t2 - t1
            sh = res["err"].shape
            n = res["err"].size
            if best is None:
                best = [torch.empty(n, dtype=torch.float64, device=self._tdev) for _ in range(4)] + \
                       [torch.empty(n, dtype=torch.int32, device=self._tdev) for _ in range(2)]
                if keep:
                    f_all, err_all = np.empty((M,) + sh), np.empty((M,) + sh, dtype=np.int32)
            cost = np.ascontiguousarray(res["debug_d"][..., 12]) if mode0 else res["f"]
            if keep:
                f_all[m], err_all[m] = cost, res["err"]
            planes = [torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).to(self._tdev)
                      for x in (cost, res["T"], res["dx"], res["dy"], res["err"])]
            fold(m, planes, best)
            times["fold"] += time.perf_counter() - t2                 # the upload of the candidate's planes and the kernel
            if self.debug:                                            # the winner's debug arrays, selected on the host
                idx = best[4].cpu().numpy().reshape(sh)
                for k in ("debug_Ncalls",) if self.debug == "ncalls" else ("debug_d", "debug_a", "debug_Ncalls"):
                    if k in res:
                        if m == 0:
                            dbg[k] = np.array(res[k])
                        else:
                            dbg[k][idx == m] = res[k][idx == m]
        out = {}
        for k, t in zip(("f", "T", "dx", "dy", "index", "err"), best):
            out[k] = t.cpu().numpy().reshape(sh)
        idx = out["index"]
        won = idx >= 0
        sel = cand[np.where(won, idx, 0)]
        for n_, k in enumerate(("a", "b", "c")):
            out[k] = np.where(won, sel[..., n_], np.nan)
        out["sigma_major"], out["sigma_minor"], out["theta"] = sigma_from_kernel(out["a"], out["b"], out["c"])
        if keep:
            out["f_all"], out["err_all"] = f_all, err_all
        out.update(dbg)
        return out
