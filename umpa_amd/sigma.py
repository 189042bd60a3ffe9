"""
Per-pixel uncertainty maps: ``libumpa_sigma.so`` (``include/umpa_sigma.h``, where the operation is defined).

No matcher says how good a pixel's ``dx``, ``dy`` are, and the result map ``f`` cannot (with the sub-pixel step on it is the
value of a smoothing spline surface, 60 to 70 times the windowed residual on a noise-only stack).  ``uncertainty`` evaluates
what any least-squares estimator offers: the covariance of the estimated shift from the model linearised at the matched
integer shift -- in the sandwich form, because the window weights are not inverse variances -- and a noise estimate from
the residual after a linearised sub-pixel refit.  ``Uncertainty.weight()`` is an inverse-variance weight for
``phase_from_match(result, weight=...)``.  HIP only: there is no CPU fallback.

``uncertainty(..., resident=True)`` and ``resident`` run the same operation on the model's own device frames
(``umpa_grid_uncertainty`` of ``libumpa_grid.so``, ``include/umpa_grid.h``): no upload, staged stacks, masked models.
"""
import numpy as np

from . import _lib

__all__ = ["region", "solve", "resident", "shift_field", "uncertainty", "Uncertainty", "SKIP"]

SKIP = _lib.SIGMA_SKIP                 # the shift of a pixel that is to be skipped (any value outside +-(max_shift - 1) is)


def _planes(kind):
    if kind not in (0, 1):
        raise ValueError("kind must be 0 (plain) or 1 (dark-field), not %r" % (kind,))
    return _lib.SIGMA_PLANES[kind]


def window_sv(win):
    """``sv`` of the header: the squares of the window summed in tap order."""
    sv = 0.0
    for w in np.asarray(win, dtype=np.float64).ravel():
        sv = sv + float(w) * float(w)
    return sv


def region(sam, ref, win, max_shift, kind, area, shift, moments=False, device=None):
    """``umpa_sigma_region``: a dictionary with ``unit`` (``[3, N0, N1]``: the variance of dy, the variance of dx and their
    covariance per unit noise variance), ``s2``, ``dof``, ``valid`` (int32) and, with ``moments``, the ``[P, N0, N1]`` planes
    of the header.  ``sam``, ``ref``: ``[K, H, W]`` float64; ``win``: the normalised ``(2 Nw + 1)^2`` window (a host array);
    ``area``: ``(start0, step0, N0, start1, step1, N1)``; ``shift``: ``[2, N0, N1]`` int32.  Host arrays give host arrays;
    contiguous HIP tensors give HIP tensors, computed on the current stream."""
    P = _planes(kind)
    win = np.ascontiguousarray(win, dtype=np.float64)
    if win.ndim != 2 or win.shape[0] != win.shape[1] or win.shape[0] % 2 == 0:
        raise ValueError("win must be a square array of odd side, not %r" % (win.shape,))
    Nw = win.shape[0] // 2
    start0, step0, N0, start1, step1, N1 = (int(v) for v in area)
    if N0 < 1 or N1 < 1:
        raise ValueError("an empty region: %d x %d pixels" % (N0, N1))
    lib = _lib.sigma()
    io = _lib.Side(sam, ref, shift, device=device, mixed="sam, ref and shift must all be host arrays or all HIP tensors")
    if io.on_device:
        import torch
        if sam.dtype != torch.float64 or ref.dtype != torch.float64 or shift.dtype != torch.int32:
            raise ValueError("sam and ref must be float64 and shift int32")
    else:
        sam, ref = np.ascontiguousarray(sam, dtype=np.float64), np.ascontiguousarray(ref, dtype=np.float64)
        shift = np.ascontiguousarray(shift, dtype=np.int32)
    if sam.ndim != 3 or tuple(sam.shape) != tuple(ref.shape):
        raise ValueError("sam and ref must be [K, H, W] stacks of one shape, not %r and %r" % (tuple(sam.shape), tuple(ref.shape)))
    if tuple(shift.shape) != (2, N0, N1):
        raise ValueError("shift must be [2, %d, %d], not %r" % (N0, N1, tuple(shift.shape)))
    K, H, W = (int(v) for v in sam.shape)
    tail = io.tail()
    out = _outputs(io, (N0, N1), (P, N0, N1) if moments else None)
    rc = lib.region(io.ptr(sam), io.ptr(ref), K, H, W, io.ptr(win), Nw, int(max_shift), kind, start0, step0, N0, start1, step1, N1,
                    io.ptr(shift), *[io.ptr(out.get(k)) for k in ("moments", "unit", "s2", "dof", "valid")], *tail)
    lib.check(rc, "sigma region")
    return out


def _outputs(io, sh, moments=None):
    """The result dictionary of both stages for planes of the shape ``sh``, on the side of ``io``."""
    out = {"unit": io.empty((3,) + sh, np.float64), "s2": io.empty(sh, np.float64), "dof": io.empty(sh, np.float64),
           "valid": io.empty(sh, np.int32)}
    if moments:
        out["moments"] = io.empty(moments, np.float64)
    return out


def solve(moments, kind, K, sv, device=None):
    """``umpa_sigma_solve``: the solve stage alone on ``moments[P, ...]`` (host array or HIP tensor): a dictionary with
    ``unit`` (``[3, ...]``), ``s2``, ``dof`` and ``valid`` in the shape of one plane."""
    P = _planes(kind)
    lib = _lib.sigma()
    if tuple(moments.shape)[:1] != (P,) or len(moments.shape) < 2:
        raise ValueError("moments must be [%d, ...] for kind %d, not %r" % (P, kind, tuple(moments.shape)))
    sh = tuple(int(v) for v in moments.shape[1:])
    n = int(np.prod(sh))
    if n < 1:
        raise ValueError("moments of %r: no pixel" % (tuple(moments.shape),))
    io = _lib.Side(moments, device=device)
    if not io.on_device:
        moments = np.ascontiguousarray(moments, dtype=np.float64)
    elif str(moments.dtype) != "torch.float64":
        raise ValueError("moments must be float64, not %s" % moments.dtype)
    tail = io.tail()
    out = _outputs(io, sh)
    rc = lib.solve(io.ptr(moments), kind, int(K), n, float(sv), *[io.ptr(out[k]) for k in ("unit", "s2", "dof", "valid")], *tail)
    lib.check(rc, "sigma solve")
    return out


def shift_field(result, max_shift):
    """The integer shift field of a match result: per axis ``clip(round(d), +-(max_shift - 1))`` of ``dy`` (rows) and ``dx``
    (columns), halves rounded away from zero as the matchers round; ``SKIP`` where ``err != 1`` or a map is not finite."""
    dy, dx = np.asarray(result["dy"], dtype=np.float64), np.asarray(result["dx"], dtype=np.float64)
    ok = (np.asarray(result["err"]) == 1) & np.isfinite(dy) & np.isfinite(dx)
    for k in ("f", "T", "df"):
        if k in result:
            ok &= np.isfinite(np.asarray(result[k]))
    lim = int(max_shift) - 1
    out = np.empty((2,) + dy.shape, dtype=np.int32)
    for n, d in enumerate((dy, dx)):
        d = np.where(ok, d, 0.0)
        out[n] = np.clip(np.sign(d) * np.floor(np.abs(d) + 0.5), -lim, lim).astype(np.int32)
        out[n][~ok] = SKIP
    return out


class Uncertainty:
    """The uncertainty maps of one match: ``sigma_dx``, ``sigma_dy`` (standard deviations in pixels), ``rho`` (their
    correlation), ``s2`` (the noise variance estimated from the residual), ``dof`` (its divisor), ``valid`` (bool), ``unit``
    (the covariance per unit noise variance) and ``noise_var`` (what the variances were scaled with: the caller's value, or
    ``None`` for ``s2``).  Invalid pixels hold NaN."""

    def __init__(self, unit, s2, dof, valid, noise_var=None):
        self.unit, self.s2, self.dof, self.noise_var = unit, s2, dof, noise_var
        scale = s2 if noise_var is None else float(noise_var)
        with np.errstate(invalid="ignore", divide="ignore"):
            var_dy, var_dx = scale * unit[0], scale * unit[1]
            self.sigma_dy, self.sigma_dx = np.sqrt(var_dy), np.sqrt(var_dx)
            self.rho = unit[2] / np.sqrt(unit[0] * unit[1])
        self.valid = (valid == 1) & np.isfinite(self.sigma_dx) & np.isfinite(self.sigma_dy)

    def weight(self):
        """``1 / (sigma_dx^2 + sigma_dy^2)`` where valid and positive, 0 elsewhere: ``phase_from_match(result, weight=...)``."""
        with np.errstate(invalid="ignore", divide="ignore"):
            w = 1.0 / (self.sigma_dx ** 2 + self.sigma_dy ** 2)
        return np.where(self.valid & np.isfinite(w), w, 0.0)


def _check_model(model, resident=False):
    """What the definition does not cover is refused here by name.  ``resident``: the call on the model's own device frames
    (``umpa_grid_uncertainty``), which takes masks."""
    from . import model as M
    why = None
    if not model._lib.is_hip:
        why = "it runs on the HIP library only"
    elif model._kind == M.KIND_DFKERNEL:
        why = "the kernel dark-field model is not supported"
    elif model._mask is not None and not resident:
        why = "masked models are not supported"
    elif not (model._one_frame_box() if resident else model._trivial_coverage()):
        why = "frames at different positions (pos_list) or of different shapes are not supported"
    elif model._refshift != 0:
        why = "assign_coordinates='ref' is not supported"
    elif not 1 <= model._Nw <= _lib.SIGMA_MAX_NW:
        why = "Nw = %d (1 to %d are supported)" % (model._Nw, _lib.SIGMA_MAX_NW)
    elif model._padding != model._Nw + model._max_shift:
        why = "a window narrower than the one the model was built with is not supported"
    if why:
        raise RuntimeError("uncertainty: %s" % why)


def _stack(frames):
    """[K, H, W] of a model's frame list: host frames are stacked; HIP tensors that are the consecutive planes of one stack
    are borrowed as they lie, others are stacked on the device."""
    if not hasattr(frames[0], "data_ptr"):
        return np.ascontiguousarray(np.stack(frames), dtype=np.float64)
    import torch
    step = frames[0].numel() * 8
    if all(f.data_ptr() == frames[0].data_ptr() + k * step for k, f in enumerate(frames)):
        base = getattr(frames[0], "_base", None)
        if base is not None and base.dim() == 3 and base.is_contiguous() and base.data_ptr() == frames[0].data_ptr() \
                and base.shape[0] >= len(frames) and tuple(base.shape[1:]) == tuple(frames[0].shape):
            return base[:len(frames)]
    return torch.stack(list(frames))


def _given_stack(model, sam):
    """The caller's sample stack in place of model._sam: [K, H, W] float64, a host array or a contiguous HIP tensor on the
    model's device, of the model's frames' shape."""
    shape = (len(model._sam),) + tuple(int(v) for v in model._sam[0].shape)
    if hasattr(sam, "data_ptr"):
        import torch
        if not sam.is_cuda or sam.device.index != model._device:
            raise ValueError("sam must be a host array or a HIP tensor on the model's device %d, not on %s" % (model._device, sam.device))
        if sam.dtype != torch.float64:
            raise ValueError("sam must be float64, not %s" % sam.dtype)
        if not sam.is_contiguous():
            raise ValueError("sam must be contiguous")
    else:
        sam = np.asarray(sam)
        if sam.dtype != np.float64:
            raise ValueError("sam must be float64, not %s" % sam.dtype)
        sam = np.ascontiguousarray(sam)
    if tuple(sam.shape) != shape:
        raise ValueError("sam must be [K, H, W] = %r as the model's stack, not %r" % (shape, tuple(sam.shape)))
    return sam


def resident(model, area, shift, moments=False):
    """``umpa_grid_uncertainty`` (``include/umpa_grid.h``): ``region`` on the model's own device frames -- the sample stack
    the last match adopted, the reference stack, the masks of a masked model, its window -- without passing or uploading a
    stack.  ``area``: ``(start0, step0, N0, start1, step1, N1)``; ``shift``: ``[2, N0, N1]`` int32, a host array (host arrays
    come back) or a contiguous HIP tensor on the model's device (HIP tensors come back, computed on the current stream).
    ``moments``: also the ``[P, N0, N1]`` planes, ``P`` = 16 / 34 without masks, 17 / 50 with."""
    start0, step0, N0, start1, step1, N1 = (int(v) for v in area)
    if N0 < 1 or N1 < 1:
        raise ValueError("an empty region: %d x %d pixels" % (N0, N1))
    kind = int(model._kind)
    P = (_lib.GRID_SIGMA_PLANES if model._mask is not None else _lib.SIGMA_PLANES)[kind]
    lib = _lib.grid()
    io = _lib.Side(shift, device=model._device)
    if io.on_device:
        import torch
        if shift.dtype != torch.int32:
            raise ValueError("shift must be int32, not %s" % shift.dtype)
        if not shift.is_cuda or shift.device.index != model._device:
            raise ValueError("shift must be a host array or a HIP tensor on the model's device %d, not on %s" % (model._device, shift.device))
    else:
        shift = np.ascontiguousarray(shift, dtype=np.int32)
    if tuple(shift.shape) != (2, N0, N1):
        raise ValueError("shift must be [2, %d, %d], not %r" % (N0, N1, tuple(shift.shape)))
    _, flags, stream = io.tail()
    out = _outputs(io, (N0, N1), (P, N0, N1) if moments else None)
    rc = lib.uncertainty(model._handle, start0, step0, N0, start1, step1, N1, io.ptr(shift),
                         *[io.ptr(out.get(k)) for k in ("moments", "unit", "s2", "dof", "valid")], flags, stream)
    lib.check(rc, "grid uncertainty")
    return out


def _uncertainty_resident(model, result, noise_var, ROI, step, shift):
    """``uncertainty(..., resident=True)``: no stacking, no upload of frames; the outputs are numpy as ever."""
    s0, s1, N0, N1 = model._region(ROI, step, ROI_wins=True)
    if tuple(np.shape(result["dx"])) != (N0, N1):
        raise ValueError("the maps of result are %r, the region has %d x %d pixels" % (tuple(np.shape(result["dx"])), N0, N1))
    if shift is None:
        shift = shift_field(result, model._max_shift)
    out = resident(model, (s0[0], s0[2], N0, s1[0], s1[2], N1), shift)
    if hasattr(shift, "data_ptr"):
        out = {k: v.cpu().numpy() for k, v in out.items()}
    return Uncertainty(out["unit"], out["s2"], out["dof"], out["valid"], noise_var)


def uncertainty(model, result, noise_var=None, ROI=None, step=None, sam=None, resident=False, shift=None):
    """The uncertainty maps of ``result = model.match(...)``: an ``Uncertainty``.

    The model supplies its stacks and its window (host frames are uploaded by the call, HIP tensors are read where they
    lie), ``result`` the shift field (``shift_field``).  ``sam``: the sample stack to use in place of the model's own,
    ``[K, H, W]`` float64, a host array or a contiguous HIP tensor on the model's device -- required after
    ``stage_sample``, whose stack (flat-corrected on the device) the model keeps no host copy of: without it the call
    raises ``RuntimeError`` until ``update_frames(sam_list=...)`` gives the model a stack again.  ``ROI`` / ``step`` as for ``match()``; the default is the model's
    current ROI, which ``match()`` left at the region of ``result``.  ``noise_var``: the variance of ``sam - model``, i.e.
    ``sigma_sam^2 + T^2 sigma_ref^2``, where it is known; by default the variances are scaled with ``s2``, which at low noise
    also contains interpolation and model misfit and is then an upper estimate.

    Plain and dark-field models without masks or ``pos_list``, ``assign_coordinates='sam'``.

    ``resident=True`` computes the maps on the model's own device frames instead (``umpa_grid_uncertainty``,
    ``include/umpa_grid.h``): nothing is stacked and no frame is uploaded, so it also works after ``stage_sample`` -- the
    stack is the one the last match adopted -- and on a model WITH masks, where the pair weight of the cost function enters
    the window weight and ``dof`` is the weight sum minus the trace.  ``sam=`` is then an error.  ``shift``: an int32
    ``[2, N0, N1]`` host array or HIP tensor on the model's device to use in place of ``shift_field(result)``, e.g. the stacked
    ``(si, sj)`` of ``basins`` / ``track`` / ``sequence``; it needs ``resident=True``.  Without ``resident`` the call is what
    it always was."""
    _check_model(model, resident=bool(resident))
    if noise_var is not None and not (np.isfinite(noise_var) and noise_var >= 0 and np.ndim(noise_var) == 0):
        raise ValueError("noise_var must be a finite scalar >= 0, not %r" % (noise_var,))
    if resident:
        if sam is not None:
            raise ValueError("uncertainty: resident=True reads the model's own device frames; sam= cannot be given with it")
        return _uncertainty_resident(model, result, noise_var, ROI, step, shift)
    if shift is not None:
        raise ValueError("uncertainty: shift= needs resident=True")
    s0, s1, N0, N1 = model._region(ROI, step, ROI_wins=True)
    if tuple(np.shape(result["dx"])) != (N0, N1):
        raise ValueError("the maps of result are %r, the region has %d x %d pixels" % (tuple(np.shape(result["dx"])), N0, N1))
    if sam is not None:
        sam = _given_stack(model, sam)
    elif model._sam_staged:
        raise RuntimeError("uncertainty: the sample stack was staged (stage_sample); pass it as sam=")
    shift = shift_field(result, model._max_shift)
    sam, ref = _stack(model._sam) if sam is None else sam, _stack(model._ref)
    reg = (s0[0], s0[2], N0, s1[0], s1[2], N1)
    if hasattr(sam, "data_ptr") != hasattr(ref, "data_ptr"):          # a given stack on the other side: both onto the device
        import torch
        dev = torch.device("cuda", model._device)
        sam, ref = (torch.from_numpy(x).to(dev) if not hasattr(x, "data_ptr") else x for x in (sam, ref))
    if hasattr(sam, "data_ptr"):
        import torch
        with torch.cuda.device(sam.device):
            out = region(sam, ref, model._window, model._max_shift, model._kind, reg, torch.from_numpy(shift).to(sam.device))
            out = {k: v.cpu().numpy() for k, v in out.items()}
    else:
        out = region(sam, ref, model._window, model._max_shift, model._kind, reg, shift, device=model._device)
    return Uncertainty(out["unit"], out["s2"], out["dof"], out["valid"], noise_var)
