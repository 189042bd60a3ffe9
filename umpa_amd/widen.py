"""
umpa_amd.widen -- window widening: the grid consumers on a box-pooled shift table.

``model.match(search='grid', widen=b)``, ``cost_volume``, ``basins`` and ``track`` (``include/umpa_grid.h``: window widening)
average the shift table and the maps over the ``(2b + 1)^2`` dense pixels around each pixel before they search.  Every
quantity averaged is a windowed sum, linear in the window, so the result is that of a model whose window is the model's
Hamming window convolved with the box -- wider, hence less noisy and less prone to a wrong basin, and coarser -- without a
second model, upload or table.  This module has what goes with the keyword:

  ``window(Nw, b)``        the window ``W'`` of half-width ``Nw + b`` the widened model matches with;
  ``valid_region(model, b, ROI=None, step=None)``  the pixels a widened call returns: a row and a column
                           ``(start, end, step)`` triple (the ``region`` key of the results);
  ``embed(map, region, into_region, fill=nan)``  a map of one region laid into another on the same grid;
  ``coarse_to_fine(model, levels=(4, 2, 1, 0), radius=None, lam=None)``  a grid search at the widest level, then one
                           ``track`` per level with the level before as its prior.
"""
import numpy as np

from . import model as _model
from .track import prior_from

__all__ = ["window", "valid_region", "embed", "coarse_to_fine"]


def window(Nw, b):
    """The window of the widened model: the model's normalised Hamming window of half-width ``Nw`` convolved with the
    ``(2b + 1)^2`` box and divided by ``(2b + 1)^2`` -- separable, of half-width ``Nw + b``, with the sum of the model's."""
    b = _model.check_widen(b)
    h = np.hamming(2 * Nw + 1)
    if b == 0:                                                      # the model's own window, bit for bit (model.pyx:691-696)
        w = np.multiply.outer(h, h)
        return np.ascontiguousarray(w / w.sum())
    w1 = np.convolve(h / h.sum(), np.ones(2 * b + 1) / (2 * b + 1))
    return np.ascontiguousarray(np.multiply.outer(w1, w1))


def valid_region(model, b, ROI=None, step=None):
    """The pixels ``model.match(search='grid', widen=b, ROI=ROI, step=step)`` returns (the model's remembered ROI by
    default): ``((start0, end0, step0), (start1, end1, step1))``.  ``b = 0``: the requested region."""
    b = _model.check_widen(b)
    s0, s1, N0, N1 = model._region(ROI, step, ROI_wins=True)
    if b == 0:
        return (s0[0], s0[0] + s0[2] * (N0 - 1) + 1, s0[2]), (s1[0], s1[0] + s1[2] * (N1 - 1) + 1, s1[2])
    return _model.widen_region(model._calculate_extent(), s0, s1, N0, N1, b)[2]


def _axis_index(src, dst):
    """Where the pixels of the triple ``src`` sit in ``dst``: ``(indices into src, indices into dst)`` of the shared ones."""
    a, c = np.arange(*src), np.arange(*dst)
    _, ia, ic = np.intersect1d(a, c, return_indices=True)
    return ia, ic


def embed(map, region, into_region, fill=float("nan")):
    """``map`` (last two axes: the pixels of ``region``) laid into an array of ``into_region``'s pixels, ``fill`` where
    ``region`` has none; pixels of ``region`` outside ``into_region`` are dropped.  Regions are pairs of
    ``(start, end, step)`` triples, as the ``region`` key of a widened result; numpy arrays and HIP tensors (which stay on
    the device) alike."""
    (ia0, ic0), (ia1, ic1) = _axis_index(region[0], into_region[0]), _axis_index(region[1], into_region[1])
    shape = tuple(map.shape[:-2]) + (len(range(*into_region[0])), len(range(*into_region[1])))
    if hasattr(map, "data_ptr"):
        import torch
        out = torch.full(shape, fill, dtype=map.dtype, device=map.device)
        if ia0.size and ia1.size:
            i0, i1 = (torch.as_tensor(v, device=map.device) for v in (ia0, ia1))
            o0, o1 = (torch.as_tensor(v, device=map.device) for v in (ic0, ic1))
            out[..., o0[:, None], o1[None, :]] = map[..., i0[:, None], i1[None, :]]
        return out
    map = np.asarray(map)
    out = np.full(shape, fill, dtype=map.dtype)
    if ia0.size and ia1.size:
        out[..., ic0[:, None], ic1[None, :]] = map[..., ia0[:, None], ia1[None, :]]
    return out


def coarse_to_fine(model, levels=(4, 2, 1, 0), radius=None, lam=None):
    """Coarse to fine in window size on one model, over its remembered ROI: ``match(search='grid', widen=levels[0])``,
    then for every later level ``track(prior, widen=level)`` whose prior is ``prior_from`` of the level before, laid into
    the level's own region with NaN (no prior: the data term decides) where the level before has no pixel.  ``radius``,
    ``lam`` as for ``model.track``.  On a model that matches HIP tensors the tracked levels' maps and the priors between
    them stay on the device.

    Returns ``(result, all)``: the last level's result and the list of every level's, each with its ``region`` (added here
    for a level of 0)."""
    levels = [_model.check_widen(b) for b in levels]
    if not levels:
        raise ValueError("coarse_to_fine: no levels")
    if hasattr(model, "_no_masked_widening"):
        model._no_masked_widening("coarse_to_fine")
    on_device = hasattr(model.sam_list[0], "data_ptr")
    results = []
    for n, b in enumerate(levels):
        region = valid_region(model, b)
        if n == 0:
            res = model.match(search='grid', widen=b, quiet=True)
        else:
            pdx, pdy = prior_from(results[-1])
            pdx, pdy = (embed(p, results[-1]['region'], region) for p in (pdx, pdy))
            if on_device and not hasattr(pdx, "data_ptr"):          # (the first level's maps come back on the host)
                import torch
                dev = model.sam_list[0].device
                pdx, pdy = (torch.as_tensor(p, dtype=torch.float64, device=dev) for p in (pdx, pdy))
            res = model.track(pdx, pdy, lam=lam, radius=radius, widen=b)
        res.setdefault('region', region)
        results.append(res)
    return results[-1], results
