"""
umpa_amd.levels -- scale-space search: every widening level from one table pass, and the level to trust per pixel.

``umpa_amd.widen.coarse_to_fine`` runs a grid search under the widest window and one ``track`` per narrower level, each a
call of its own that rebuilds the shift table and the maps.  ``scale_space`` is the same chain as ONE call
(``include/umpa_grid.h``: ``umpa_grid_levels_track``): the table of a row chunk is computed once and pooled to every level in
one read, the prior goes from level to level on the device, and the device then answers the question a scale space is
there for -- which window to trust at which pixel: the narrowest level that still agrees, within ``tol``, with every wider
one that matched (Lepski's rule).

  ``scale_space(model, levels=(4, 2, 1, 0), tol=None, lam=None, radius=None, ROI=None, step=None)``  ``(selected, all)``;
  ``select_levels(results, tol, levels=None)``  the rule in numpy, on a list of level results of one region.
"""
import numpy as np

from . import _lib
from . import model as _model

__all__ = ["scale_space", "select_levels"]

_DBL = ('f', 'T', 'dx', 'dy', 'cost', 'df', 'cost0')
_INT = ('si', 'sj', 'err', 'count', 'found')
_ORDER = ('f', 'T', 'dx', 'dy', 'cost', 'df', 'si', 'sj', 'err', 'cost0', 'count', 'found')    # the library's argument order


def check_levels(levels):
    """``levels`` as the library takes them: 1 to 4 integer half-widths, strictly decreasing, the widened ones from
    {1, 2, 4, 8} and at most three, a 0 (the model's own window) only at the end.  Returns them as a list of ``int``."""
    text = ("levels must be 1 to %d decreasing half-widths, the widened ones from %s and at most three, a 0 only at the end, not %r"
            % (_lib.GRID_MAX_LEVELS, set(_lib.GRID_LEVEL_WIDTHS), levels))
    try:
        given = list(levels)
    except TypeError:
        raise ValueError(text) from None
    if not 1 <= len(given) <= _lib.GRID_MAX_LEVELS:
        raise ValueError(text)
    for n, b in enumerate(given):
        if isinstance(b, (bool, np.bool_)) or not isinstance(b, (int, np.integer)):
            raise ValueError(text)
        if not (b in _lib.GRID_LEVEL_WIDTHS or (b == 0 and n == len(given) - 1)) or (n and b >= given[n - 1]):
            raise ValueError(text)
    if sum(1 for b in given if b > 0) > 3:
        raise ValueError(text)
    return [int(b) for b in given]


def check_tol(tol, L):
    """``tol`` as ``L`` doubles: ``None`` (no limit: the narrowest level that matched), one number for every level, or one
    per level; each ``>= 0`` or ``inf``."""
    if tol is None:
        return np.full(L, np.inf)
    t = np.asarray(tol, dtype=np.float64)
    if t.ndim == 0:
        t = np.full(L, float(t))
    if t.shape != (L,) or not (t >= 0.0).all():
        raise ValueError("tol must be None, a number >= 0 or one such number per level (%d), not %r" % (L, tol))
    return np.ascontiguousarray(t)


def _host(a):
    return a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)


def select_levels(results, tol, levels=None):
    """The selection rule of ``umpa_grid_levels_track`` in numpy.  ``results``: the level results, widest first, all on one
    region (``scale_space``'s list, or ``coarse_to_fine``'s after ``umpa_amd.widen.embed`` onto one region); ``tol`` as for
    ``scale_space``.  With ``ok_l = (err_l == 1) & isfinite(dx_l) & isfinite(dy_l)``, level ``l`` is consistent where ``ok_l``
    and ``|dx_l - dx_m| <= tol[m]`` and ``|dy_l - dy_m| <= tol[m]`` for every wider ``m`` with ``ok_m``; ``level`` is the
    largest consistent ``l``, -1 where no level is ok.  Returns the maps every level has, taken per pixel from its
    ``level`` (from the last level at -1), ``level`` and, with ``levels`` (the half-widths), ``halfwidth`` (int32)."""
    L = len(results)
    if L < 1:
        raise ValueError("select_levels: no levels")
    t = check_tol(tol, L)
    dx = [np.asarray(_host(r['dx']), dtype=np.float64) for r in results]
    dy = [np.asarray(_host(r['dy']), dtype=np.float64) for r in results]
    ok = [(_host(r['err']) == 1) & np.isfinite(x) & np.isfinite(y) for r, x, y in zip(results, dx, dy)]
    level = np.full(dx[0].shape, -1, dtype=np.int32)
    with np.errstate(invalid='ignore'):
        for l in range(L):
            good = ok[l].copy()
            for m in range(l):
                good &= ~ok[m] | ((np.abs(dx[l] - dx[m]) <= t[m]) & (np.abs(dy[l] - dy[m]) <= t[m]))
            level[good] = l
    pick = np.where(level < 0, L - 1, level)
    out = {}
    for k in results[0]:
        if k == 'region' or not all(k in r for r in results):
            continue
        stack = np.stack([_host(r[k]) for r in results])               # [L, (2,) N0, N1]
        idx = np.broadcast_to(pick, stack.shape[1:])[None]
        out[k] = np.take_along_axis(stack, idx, axis=0)[0]
    out['level'] = level
    if levels is not None:
        b = np.asarray(list(levels) + [-1], dtype=np.int32)
        out['halfwidth'] = b[level]
    if 'region' in results[0]:
        out['region'] = results[0]['region']
    return out


def _kept(native, region):
    """the slices of a map of the region ``native`` (two triples) that hold the pixels of ``region`` on the same grid"""
    out = []
    for n, r in zip(native, region):
        first = (r[0] - n[0]) // n[2]
        out.append(slice(first, first + len(range(*r))))
    return tuple(out)


def _pack(arrays, region, on_device):
    """a dictionary of the library's planes as ``model.track()`` returns it"""
    out = {k: v for k, v in arrays.items() if k not in ('si', 'sj', 'err')}
    if on_device:
        import torch
        out['shift'] = torch.stack([arrays['si'], arrays['sj']], dim=0)
        out['err'] = torch.clamp(arrays['err'], min=0)
    else:
        out['shift'] = np.stack([arrays['si'], arrays['sj']], axis=0)
        out['err'] = np.maximum(arrays['err'], 0)
    out['region'] = region
    return out


def scale_space(model, levels=(4, 2, 1, 0), tol=None, lam=None, radius=None, ROI=None, step=None):
    """Every level of ``umpa_amd.widen.coarse_to_fine(model, levels, radius, lam)`` from one pass over the shift table, and
    the level to trust per pixel.

    ``levels``: up to four decreasing half-widths, the widened ones from {1, 2, 4, 8} (at most three), an optional final 0 for
    the model's own window.  The first level is the grid search under the widest window; every later level is
    ``model.track(widen=level)`` with ``prior_from`` the level before as its prior, ``lam`` and ``radius`` as for
    ``model.track``.  ``tol`` (``None``, a number, or one per level): a level is trusted at a pixel where it matched and its
    ``dx``, ``dy`` lie within ``tol[m]`` of those of every wider level ``m`` that matched.

    The call is made on the region (``ROI`` / ``step``, the model's remembered ROI by default) grown by ``levels[0]`` where the
    extent allows, and every result is cropped to ``umpa_amd.widen.valid_region(model, min(levels))``: a level wider than
    that holds, at the pixels near the border of the extent where its window does not fit, what ``track`` gives a pixel
    without a basin (``found == 0``, ``err == 0``, zeros).

    Returns ``(selected, all)``.  ``all``: one dictionary per level with the keys of ``model.track()`` and ``region``.
    ``selected``: the same keys, per pixel the values of the narrowest trusted level (of the last level where no level
    matched), plus ``level`` (its index, -1 where none matched) and ``halfwidth`` (``levels[level]`` or -1), int32.  On a
    model that matches HIP tensors all maps are HIP tensors filled on the current stream; else page-locked numpy arrays."""
    if not hasattr(model, "_grid_check"):
        raise RuntimeError("scale_space needs a model with track() (UMPAModelNoDF or UMPAModelDF)")
    model._grid_check("scale_space")
    model._no_masked_widening("scale_space")
    levels = check_levels(levels)
    L = len(levels)
    tol = check_tol(tol, L)
    number = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))
    if lam is not None and not (number(lam) and 0.0 <= float(lam) < np.inf):
        raise ValueError("scale_space: lam must be None (the nearest basin) or a finite number >= 0, not %r" % (lam,))
    if radius is not None and not (number(radius) and float(radius) >= 0.0):
        raise ValueError("scale_space: radius must be None (no limit) or a number >= 0, not %r" % (radius,))
    mode = _lib.GRID_TRACK_NEAREST if lam is None else _lib.GRID_TRACK_PENALTY

    s0, s1, N0, N1 = model._region(ROI, step, ROI_wins=True)
    extent = model._calculate_extent()
    bmax, bmin = levels[0], levels[-1]
    if bmin:
        region = _model.widen_region(extent, s0, s1, N0, N1, bmin)[2]
    else:
        region = ((s0[0], s0[0] + s0[2] * (N0 - 1) + 1, s0[2]), (s1[0], s1[0] + s1[2] * (N1 - 1) + 1, s1[2]))
    if bmax:
        n0, n1, N0, N1 = _model.widen_region(extent, s0, s1, N0, N1, bmax)[0]
    else:
        n0, n1 = region
    crop = _kept((n0, n1), region)

    on_device = hasattr(model.sam_list[0], "data_ptr")
    df = model._kind == _model.KIND_DF
    dbl = [k for k in _DBL if df or k != 'df']
    if on_device:
        import torch
        dev = model.sam_list[0].device
        mk = lambda shape, dt: torch.empty(shape, dtype=torch.float64 if dt is np.float64 else torch.int32, device=dev)
    else:
        mk = lambda shape, dt: _lib.pinned_empty(shape, np.dtype(dt))
    lev = {k: mk((L, N0, N1), np.float64) for k in dbl}
    lev.update({k: mk((L, N0, N1), np.int32) for k in _INT})
    sel = {k: mk((N0, N1), np.float64) for k in dbl}
    sel.update({k: mk((N0, N1), np.int32) for k in _INT + ('level', 'halfwidth')})

    _, flags, stream = _lib.Side(*lev.values(), *sel.values(), device=model._device).tail(model._staged_flag())
    b = np.ascontiguousarray(levels, dtype=np.int32)
    ptr = _lib.Side.ptr
    args = [model._handle, n0[0], n0[2], N0, n1[0], n1[2], N1, L, b.ctypes.data, int(mode), 0.0 if lam is None else float(lam),
            -1.0 if radius is None else float(radius), tol.ctypes.data]
    args += [ptr(lev.get(k)) for k in _ORDER] + [ptr(sel.get(k)) for k in _ORDER] + [ptr(sel['level']), ptr(sel['halfwidth'])]
    try:
        _lib.grid().check(_lib.grid().levels_track(*args, flags, stream), "grid levels_track")
    except _lib.NativeError as e:
        raise RuntimeError("scale_space: %s" % e) from None

    every = [_pack({k: _model._cropped(v[l], crop) for k, v in lev.items()}, region, on_device) for l in range(L)]
    selected = _pack({k: _model._cropped(v, crop) for k, v in sel.items()}, region, on_device)
    return selected, every
