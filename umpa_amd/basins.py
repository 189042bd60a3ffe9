"""
umpa_amd.basins -- choosing among the basins of ``model.basins()``.

``model.basins(k)`` (``include/umpa_grid.h``: ``umpa_grid_basins``) returns, per pixel, the ``k`` lowest local minima of the
cost over the search box, each with the sub-pixel step and the fit ``match(search='grid')`` would have given it.  Which of
them is the right one is decided with information the data term lacks -- the previous projection of a step scan, a
low-resolution estimate, a neighbour.  The helpers here are that decision's host side: small numpy functions on the
dictionary, no device work.

  ``nearest(b, prior_dx, prior_dy)``  per pixel, the rank of the kept basin closest to a prior shift field;
  ``select(b, index)``                an ordinary result dictionary (``dx``, ``dy``, ``f``, ``T``, ``df``, ``err``) from a rank per pixel;
  ``start_shifts(b, index)``          the ``dxdy`` argument of ``model.match()`` that starts the walk in those basins;
  ``ambiguity(b)``                    ``cost[1] - cost[0]``: how far the second basin lies above the first.
"""
import numpy as np

__all__ = ["select", "nearest", "start_shifts", "ambiguity"]

_MAPS = ("dx", "dy", "f", "T", "df", "cost")


def _index(b, index):
    """``index`` as an intp ``[1, N0, N1]`` array of ranks, checked against the dictionary's ``k``."""
    k, N0, N1 = np.shape(b["err"])
    idx = np.asarray(index)
    if idx.dtype.kind not in "iu":
        raise ValueError("basins: the rank index must be of an integer type, not %s" % idx.dtype)
    if idx.ndim not in (0, 2) or (idx.ndim == 2 and idx.shape != (N0, N1)):
        raise ValueError("basins: the rank index must be a scalar or of shape %s, not %s" % ((N0, N1), idx.shape))
    if idx.size and (idx.min() < 0 or idx.max() >= k):
        raise ValueError("basins: ranks must lie in 0 .. %d" % (k - 1))
    return np.broadcast_to(idx, (N0, N1)).astype(np.intp)[None]


def select(b, index):
    """The maps of rank ``index`` (a scalar, or one rank per pixel ``[N0, N1]``) as ``match()`` returns them: ``dx``,
    ``dy``, ``f``, ``T`` (``df``) float64 and ``err`` int32, ``[N0, N1]`` each, plus ``cost`` and ``shift`` (``[2, N0, N1]``,
    row shift first).  A pixel that has no basin of the rank asked for gets what ``match()`` gives a pixel it could not
    match: ``err = 0`` and zeros."""
    idx = _index(b, index)
    out = {n: np.take_along_axis(np.asarray(b[n]), idx, axis=0)[0] for n in _MAPS if n in b}
    err = np.take_along_axis(np.asarray(b["err"]), idx, axis=0)[0]
    out["err"] = np.where(err > 0, 1, 0).astype(np.int32)
    out["shift"] = np.take_along_axis(np.asarray(b["shift"]), idx[:, None], axis=0)[0]
    return out


def nearest(b, prior_dx, prior_dy):
    """Per pixel, the rank (intp ``[N0, N1]``) of the kept basin whose integer shift is closest, in the Euclidean sense, to
    the prior ``(prior_dy rows, prior_dx columns)`` -- the conventions of ``match()``: ``dy`` is the row shift.  Scalars or
    ``[N0, N1]`` arrays.  Among equally close basins the lower rank (the lower cost) wins; a NaN prior, and a pixel
    without any basin, give rank 0."""
    err = np.asarray(b["err"])
    shift = np.asarray(b["shift"]).astype(np.float64)
    pdx = np.broadcast_to(np.asarray(prior_dx, dtype=np.float64), err.shape[1:])
    pdy = np.broadcast_to(np.asarray(prior_dy, dtype=np.float64), err.shape[1:])
    d2 = (shift[:, 0] - pdy[None]) ** 2 + (shift[:, 1] - pdx[None]) ** 2
    d2 = np.where((err >= 0) & ~np.isnan(d2), d2, np.inf)
    return np.argmin(d2, axis=0)                                     # the first of equal distances: the lower rank


def start_shifts(b, index):
    """``dxdy`` for ``model.match(dxdy=...)``: the integer shifts of rank ``index`` as a pair of float64 ``[N0, N1]`` arrays,
    row shift first (the order in which ``match()`` reads its start shifts).  (0, 0) where the pixel has no such basin."""
    sh = np.take_along_axis(np.asarray(b["shift"]), _index(b, index)[:, None], axis=0)[0]
    return sh[0].astype(np.float64), sh[1].astype(np.float64)


def ambiguity(b):
    """``cost[1] - cost[0]`` per pixel: small where the data term alone hardly tells the two best basins apart.  ``+Inf``
    where the pixel has fewer than two basins.  Needs ``k >= 2``."""
    cost = np.asarray(b["cost"])
    if cost.shape[0] < 2:
        raise ValueError("basins: ambiguity needs the two best basins (k >= 2)")
    with np.errstate(invalid="ignore"):
        gap = cost[1] - cost[0]
    return np.where(np.asarray(b["count"]) >= 2, gap, np.inf)
