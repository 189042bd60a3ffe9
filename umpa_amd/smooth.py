"""
Regularised shift search: ``libumpa_smooth.so`` (``include/umpa_smooth.h``, where the operation is defined).

``match()`` decides every pixel on its own, ``search='grid'`` included: where the speckle visibility is low or the frames
are noisy, the lowest of the ``(2 max_shift - 1)^2`` noisy costs of a pixel is now and then a spurious one, and the ``dx`` /
``dy`` maps carry isolated pixels from a wrong basin.  ``aggregate`` is the spatially regularised consumer of the cost
volume (semi-global matching): the costs are summed along 4 or 8 path directions under a truncated-linear penalty on shift
changes between neighbours, then the minimum is taken.  ``match_smooth`` uses the resulting INTEGER field only as the
per-pixel start shift of the ordinary walk: regularisation chooses the basin, the data term alone gives ``dx``, ``dy``,
``T``, ``df`` and ``f``.  HIP only: there is no CPU fallback.
"""
import numpy as np

from . import _lib

__all__ = ["aggregate", "cost_scale", "match_smooth", "LAM_REL", "TRUNC_REL"]

# The default penalties in units of cost_scale(); chosen on synthetic stacks with the numpy restatement (DESIGN.md section
# 4.10 holds the table).
LAM_REL, TRUNC_REL = 1.0, 2.0


def _dirs(paths):
    if paths not in (4, 8):
        raise ValueError("paths must be 4 or 8, not %r" % (paths,))
    return 0x0F if paths == 4 else 0xFF


def _volume_shape(shape):
    shape = tuple(int(v) for v in shape)
    if len(shape) == 4 and shape[0] == shape[1]:
        U = shape[0]
    elif len(shape) == 3 and int(round(shape[0] ** 0.5)) ** 2 == shape[0]:
        U = int(round(shape[0] ** 0.5))
    else:
        raise ValueError("cost must be [U, U, N0, N1] or [U * U, N0, N1], not %r" % (shape,))
    if U % 2 == 0 or not _lib.SMOOTH_MIN_U <= U <= _lib.SMOOTH_MAX_U:
        raise ValueError("cost of %r: U = %d must be odd and within %d to %d" % (shape, U, _lib.SMOOTH_MIN_U, _lib.SMOOTH_MAX_U))
    if shape[-2] < 1 or shape[-1] < 1:
        raise ValueError("cost of %r: an empty region" % (shape,))
    return U, shape[-2], shape[-1]


def _check_penalties(lam, trunc):
    lam, trunc = float(lam), float(trunc)
    if not lam >= 0:
        raise ValueError("lam must be >= 0, not %r" % (lam,))
    if not trunc >= 0:
        raise ValueError("trunc must be >= 0 (inf: no truncation), not %r" % (trunc,))
    return lam, trunc


def aggregate(cost, lam, trunc, paths=8, return_total=False, device=None, dirs=None):
    """Path aggregation and selection on a cost volume: a dictionary with ``shift`` (``[2, N0, N1]`` int32, the row and the
    column shift of the chosen label), ``smin`` (the summed cost of that label), ``margin`` (how far the best label at
    least 2 steps away lies above it; ``inf`` where there is none), ``valid`` (int32; 0 where every cost of the pixel is
    non-finite: shift, smin and margin are 0 there) and, with ``return_total``, the summed volume ``total`` in the shape of
    ``cost``.

    ``cost``: ``[U, U, N0, N1]``, as ``cost_volume()`` returns it, or ``[U * U, N0, N1]``; float64, ``U`` odd, 3 to 15.
    ``lam`` is the penalty per unit of shift change between neighbouring pixels, ``trunc`` the cap on that penalty
    (``inf``: none), both in the units of ``cost`` (``cost_scale`` gives a natural one).  ``paths``: 4 (rows and columns)
    or 8 (and the diagonals); ``dirs`` selects single directions by the bit mask of the header instead.

    A host array gives host arrays; a HIP tensor (contiguous) gives HIP tensors, computed on the current stream."""
    lam, trunc = _check_penalties(lam, trunc)
    mask = _dirs(paths) if dirs is None else int(dirs)
    if not 1 <= mask <= _lib.SMOOTH_ALL_DIRS:
        raise ValueError("dirs must be a mask of the directions 0 to 7, not %r" % (dirs,))
    lib = _lib.smooth()
    io = _lib.Side(cost, device=device)
    if not io.on_device:
        cost = np.ascontiguousarray(cost, dtype=np.float64)
    elif str(cost.dtype) != "torch.float64":
        raise ValueError("cost must be float64, not %s" % cost.dtype)
    U, N0, N1 = _volume_shape(cost.shape)
    tail = io.tail()
    out = {"shift": io.empty((2, N0, N1), np.int32), "smin": io.empty((N0, N1), np.float64),
           "margin": io.empty((N0, N1), np.float64), "valid": io.empty((N0, N1), np.int32)}
    if return_total:
        out["total"] = io.empty(cost.shape, np.float64)
    rc = lib.aggregate(io.ptr(cost), U, N0, N1, lam, trunc, mask, *[io.ptr(out.get(k)) for k in ("shift", "smin", "margin", "valid", "total")], *tail)
    lib.check(rc, "smooth aggregate")
    return out


def cost_scale(cost):
    """The unit in which relative penalties are given: the median, over the pixels that have a finite cost, of (the mean
    of the pixel's finite costs - the least of them).  Host array or HIP tensor; a float (``nan`` where no pixel has a
    finite cost)."""
    if hasattr(cost, "data_ptr"):
        import torch
        _volume_shape(cost.shape)
        c = cost.reshape(-1, cost.shape[-2] * cost.shape[-1])
        fin = torch.isfinite(c)
        n = fin.sum(dim=0)
        live = n > 0
        if not bool(live.any()):
            return float("nan")
        mean = torch.where(fin, c, torch.zeros_like(c)).sum(dim=0)[live] / n[live]
        low = torch.where(fin, c, torch.full_like(c, float("inf"))).min(dim=0).values[live]
        s = torch.sort(mean - low).values
        return float((s[(s.numel() - 1) // 2] + s[s.numel() // 2]) / 2)
    cost = np.asarray(cost, dtype=np.float64)
    _volume_shape(cost.shape)
    c = cost.reshape(-1, cost.shape[-2] * cost.shape[-1])
    fin = np.isfinite(c)
    n = fin.sum(axis=0)
    live = n > 0
    if not live.any():
        return float("nan")
    mean = np.where(fin, c, 0.0).sum(axis=0)[live] / n[live]
    low = np.where(fin, c, np.inf).min(axis=0)[live]
    return float(np.median(mean - low))


def match_smooth(model, lam=None, trunc=None, paths=8, ROI=None, step=None, quiet=True):
    """``model.match()`` started, pixel by pixel, from the regularised integer shift field of the model's own cost volume.

    The volume is computed on the device (``umpa_grid_cost_volume``) and stays there (a stack uploaded by ``stage_sample``
    is adopted by that call, so the volume and the match read the same stack); ``lam`` and ``trunc`` default to
    ``LAM_REL`` and ``TRUNC_REL`` times ``cost_scale`` of it.  Returns the dictionary of
    ``model.match(dxdy=(start[0], start[1]), ROI=..., step=...)`` plus ``start`` (``[2, N0, N1]`` int32), ``margin``
    (``aggregate``), ``valid`` and the penalties used, ``lam`` and ``trunc``.

    Models ``cost_volume()`` takes only (no ``pos_list``, not the kernel dark-field model, masks with ``masked_grid`` on): anything else
    raises what ``cost_volume()`` raises.  Mind the memory: four volumes of ``(2 max_shift - 1)^2 N0 N1`` doubles."""
    import torch
    _dirs(paths)
    dev = torch.device("cuda", model._device)

    def volume(U, N0, N1):
        if not _lib.SMOOTH_MIN_U <= U <= _lib.SMOOTH_MAX_U:
            raise RuntimeError("match_smooth: max_shift = %d (2 to 8 are supported)" % model._max_shift)
        return {"cost": torch.empty((U, U, N0, N1), dtype=torch.float64, device=dev)}

    s0, s1, out = model._grid_cost_volume(ROI, step, volume)
    with torch.cuda.device(dev):
        cost = out.pop("cost")
        if lam is None or trunc is None:
            unit = cost_scale(cost)
            lam = LAM_REL * unit if lam is None else lam
            trunc = TRUNC_REL * unit if trunc is None else trunc
        lam, trunc = _check_penalties(lam, trunc)
        agg = aggregate(cost, lam, trunc, paths=paths)
        start = agg["shift"].cpu().numpy()
        margin, valid = agg["margin"].cpu().numpy(), agg["valid"].cpu().numpy()
        del cost, agg
    result = model.match(dxdy=(start[0], start[1]), ROI=(s0, s1), quiet=quiet)
    result.update(start=start, margin=margin, valid=valid, lam=lam, trunc=trunc)
    return result
