"""
Host-side mirror of the reference's model API on top of the HIP library.

Classes ``UMPAModelNoDF`` / ``UMPAModelDF`` / ``UMPAModelDFKernel`` keep the names,
constructor arguments, methods, properties, result dictionaries and error behaviour of
the reference extension types (reference ``UMPA/model.pyx:116-997``), so code written
against ``UMPA.model`` runs unchanged.  All numerics happen in ``libumpa_hip.so``
(``include/umpa_hip.h``); this module only does what the Cython layer did around the C++
core: pointer marshalling, padding / extent / ROI arithmetic, the Hamming window and
result packing.

Differences from the reference, all deliberate:
 * frames that are not float64 are converted to float64 copies (the reference casts to a
   temporary and then reads freed memory);
 * ``num_threads`` is accepted and ignored (the pixel loop runs on the GPU);
 * ``ROI`` tuples and a grown ``Nw`` are range-checked (the reference reads out of bounds);
 * ``debug_a`` of a pixel whose walk ended before the 4x4 gather is zero (the reference
   leaves whatever the same OpenMP thread computed for an earlier pixel).
 * extra keyword ``device`` (HIP device index, default: ``UMPA_HIP_DEVICE`` or 0) and
   attribute ``debug`` (default True, as the reference is compiled with DEBUG=True,
   ``model.pyx:26``): set False to skip the three ``debug_*`` outputs (332 B/pixel).
"""
import os

import numpy as np

from . import _lib

__all__ = ["UMPAModelBase", "UMPAModelNoDF", "UMPAModelDF", "UMPAModelDFKernel",
           "spm", "spmq"]

NPDOUBLE = np.dtype("float64")

KIND_NODF, KIND_DF, KIND_DFKERNEL = 0, 1, 2


def _cround(x):
    """libc round(): halves away from zero (the reference's `from libc.math cimport round`, model.pyx:20);
    Python's round() goes to the even neighbour."""
    x = float(x)
    return int(np.sign(x) * np.floor(abs(x) + 0.5))


def _default_device():
    if "UMPA_HIP_DEVICE" in os.environ:
        return int(os.environ["UMPA_HIP_DEVICE"])
    if "LOCAL_RANK" in os.environ:            # one process per GPU under torch.distributed.run
        n = _lib.hip().device_count()
        return int(os.environ["LOCAL_RANK"]) % max(n, 1)
    return 0


def _spfit(a, quad):
    """reference ``model.spm`` / ``model.spmq`` (``model.pyx:31-80``) evaluated on the device."""
    if a.shape != (4, 4):
        raise RuntimeError("input array must be (4,4)")
    if a.dtype not in (np.dtype("float64"), np.dtype("float32")):
        raise RuntimeError("Unsupported data type")
    a64 = np.ascontiguousarray(a, dtype=np.float64)
    pos = np.zeros(2)
    val = np.zeros(1)
    lib = _lib.hip()
    fn = lib.spmin_quad if quad else lib.spmin
    lib.check(fn(_default_device(), _lib._ptr(a64, _lib._dp), _lib._ptr(pos, _lib._dp),
                 _lib._ptr(val, _lib._dp)), "spmin")
    if a.dtype == np.dtype("float32"):
        return pos.astype(np.float32), np.float32(val[0])
    return pos, float(val[0])


def spm(a):
    """Sub-pixel minimum of a 4x4 array by quadratic fit (``model.pyx:31-54`` -> ``spmin_quad``)."""
    return _spfit(np.asarray(a), True)


def spmq(a):
    """Sub-pixel minimum of a 4x4 array by the B-spline model (``model.pyx:57-80`` -> ``spmin``)."""
    return _spfit(np.asarray(a), False)


# -- ROI / extent arithmetic (model.pyx:531-623), as functions of the extent: the models and ddf.KernelSearch share it
def _roi_slices(extent, ROI, step, current):
    N0, N1 = extent
    if ROI is not None:
        if step is not None:
            raise RuntimeError('Step and ROI should not be specified simultaneously.')
        s0, s1 = ROI
        if type(s0) is slice:
            s0 = s0.indices(N0)
        if type(s1) is slice:
            s1 = s1.indices(N1)
    else:
        s0, s1 = current
        if step is not None:
            s0 = slice(s0[0], s0[1], step).indices(N0)
            s1 = slice(s1[0], s1[1], step).indices(N1)
    return tuple(int(v) for v in s0), tuple(int(v) for v in s1)


def _roi_counts(s0, s1):
    start0, end0, step0 = s0
    start1, end1, step1 = s1
    if step0 < 1 or step1 < 1:
        raise RuntimeError('ROI steps must be positive.')
    N0 = 1 + (end0 - start0 - 1) // step0                           # model.pyx:414-415
    N1 = 1 + (end1 - start1 - 1) // step1
    return N0, N1


def _roi_check_range(extent, s0, s1, N0, N1):
    E0, E1 = extent
    if N0 < 1 or N1 < 1:
        raise RuntimeError('Empty ROI %s.' % ((s0, s1),))
    if s0[0] < 0 or s1[0] < 0 or s0[0] + s0[2] * (N0 - 1) >= E0 or s1[0] + s1[2] * (N1 - 1) >= E1:
        raise RuntimeError('ROI %s exceeds the reconstructible extent %s.' % ((s0, s1), (E0, E1)))


def resolve_region(extent, ROI, step, current):
    """``(s0, s1, N0, N1)`` of ``ROI`` (slices or ``(start, end, step)`` triples), or of ``current`` (such triples) taken
    with ``step``, on an image of ``extent``: the two ranges and their pixel counts.  Refused in this order: both ``ROI``
    and ``step``, steps that are not positive, an empty region, one that leaves the extent."""
    s0, s1 = _roi_slices(extent, ROI, step, current)
    N0, N1 = _roi_counts(s0, s1)
    _roi_check_range(extent, s0, s1, N0, N1)
    return s0, s1, N0, N1


def check_widen(widen, search='grid'):
    """``widen`` as the grid consumers take it (``include/umpa_grid.h``, window widening): an integer half-width from 0 to
    ``_lib.GRID_MAX_WIDEN``; more than 0 only beside ``search='grid'``.  Returns it as an ``int``."""
    if isinstance(widen, (bool, np.bool_)) or not isinstance(widen, (int, np.integer)) or not 0 <= widen <= _lib.GRID_MAX_WIDEN:
        raise ValueError("widen must be an integer from 0 to %d, not %r" % (_lib.GRID_MAX_WIDEN, widen))
    if widen and search != 'grid':
        raise ValueError("widen > 0 needs search='grid': the walk reads the cost under the model's own window")
    return int(widen)


def _widen_axis(E, s, N, b):
    """One axis of ``widen_region``: ``(native start, native count, first kept native index, kept count)``."""
    start, step = s[0], s[2]
    last = start + step * (N - 1)
    m = -(-b // step)                                               # grid points that cover b dense pixels
    lo, hi = min(m, start // step), min(m, (E - 1 - last) // step)
    n_start, n_last = start - step * lo, last + step * hi
    klo = max(0, -((start - n_start - b) // step))                  # the first k with start + step k - b >= n_start
    khi = min(N - 1, (n_last - b - start) // step)
    return n_start, N + lo + hi, klo + lo, khi - klo + 1


def widen_region(extent, s0, s1, N0, N1, b):
    """The region a widened call (half-width ``b``) computes for the requested one, and what of it is kept.

    The library gives NaN costs to the pixels within ``b`` dense pixels of the border of the region it is called on.  So the
    call is made on the requested grid grown by ``ceil(b / step)`` grid points on every side, or by as many as stay inside
    ``extent``, and the result is cropped to the requested pixels whose ``(2b + 1)^2`` block lies inside the grown
    region's dense grid: with unit steps, all whose widened window fits the extent.

    Returns ``(native, crop, region)``: ``native = (s0, s1, N0, N1)`` for the library, ``crop`` the two slices of its maps
    that are kept, ``region`` the kept pixels as two ``(start, end, step)`` triples."""
    a0 = _widen_axis(extent[0], s0, N0, b)
    a1 = _widen_axis(extent[1], s1, N1, b)
    if a0[3] < 1 or a1[3] < 1:
        raise RuntimeError("widen=%d: no pixel of the region %s keeps its widened window inside the extent %s"
                           % (b, (s0, s1), tuple(extent)))
    native = ((a0[0], a0[0] + s0[2] * (a0[1] - 1) + 1, s0[2]), (a1[0], a1[0] + s1[2] * (a1[1] - 1) + 1, s1[2]), a0[1], a1[1])
    crop = (slice(a0[2], a0[2] + a0[3]), slice(a1[2], a1[2] + a1[3]))
    first0, first1 = a0[0] + s0[2] * a0[2], a1[0] + s1[2] * a1[2]
    region = ((first0, first0 + s0[2] * (a0[3] - 1) + 1, s0[2]), (first1, first1 + s1[2] * (a1[3] - 1) + 1, s1[2]))
    return native, crop, region


def _grown(p, shape, crop):
    """A prior plane of the kept region inside a NaN plane of the grown one (``widen_region``), on the prior's side."""
    if hasattr(p, "data_ptr"):
        import torch
        full = torch.full(tuple(shape), float("nan"), dtype=p.dtype, device=p.device)
    else:
        full = np.full(shape, np.nan, dtype=NPDOUBLE)
    full[tuple(crop)] = p
    return full


def _cropped(a, crop):
    """The kept pixels (last two axes) of a map of a widened call, contiguous: a numpy array or a HIP tensor."""
    v = a[(Ellipsis,) + tuple(crop)]
    return v.contiguous() if hasattr(v, "data_ptr") else np.ascontiguousarray(v)


class UMPAModelBase:
    """Mirror of ``UMPAModelBase`` (``model.pyx:116-755``)."""

    Nparam = 0
    safe_crop = 0
    _kind = None
    debug = True

    # -- backend hook (the test-suite's CPU checkers override this; the product never does)
    def _native(self):
        return _lib.hip()

    def __init__(self, sam_list, ref_list, mask_list=None, pos_list=None,
                 window_size=2, max_shift=4, ROI=None, device=None):
        if self._kind is None:
            raise NotImplementedError(
                'UMPAModelBase is not supposed to be called directly, use one of '
                'the subclasses "UMPAModelNoDF", "UMPAModelDF", or "UMPAModelDFKernel".')
        Nw = int(window_size)
        Na = len(sam_list)
        self._handle = None
        self._lib = self._native()
        self._device = _lib.host_device(device)

        # frames and shapes (model.pyx:225-254)
        self._sam = self._prepare_frames(sam_list)
        self._shape_list = [np.array(s.shape, dtype=np.int32) for s in self._sam]
        self._sam_list = sam_list
        self._ref = self._prepare_frames(ref_list)
        for k, r in enumerate(self._ref):
            samsh = tuple(int(x) for x in self._shape_list[k])
            if samsh != tuple(r.shape):
                raise RuntimeError('Incompatible shape between sample {0} and '
                                   'reference frames {1} (entry [{2}] in the '
                                   'datasets).'.format(samsh, tuple(r.shape), k))
        self._ref_list = ref_list
        self._mask = None
        if mask_list is not None:                                   # model.pyx:257-262
            self._mask = self._prepare_frames(mask_list)
            if len(self._mask) != Na or any(tuple(m.shape) != tuple(s.shape)
                                            for m, s in zip(self._mask, self._sam)):
                raise RuntimeError('mask_list must match sam_list in length and frame shapes.')
        self._mask_list = mask_list

        # positions (model.pyx:265-283)
        if pos_list is None:
            pos_list = [np.zeros((2,), dtype=np.int32) for _ in range(Na)]
        else:
            pos_list = [np.asarray(p).astype(np.int32) for p in pos_list]
            if len(pos_list) != Na:
                raise RuntimeError(
                    'Unexpected length for position list (len(pos_list)={0}, '
                    'len(sam_list)={1})'.format(len(pos_list), Na))
        if np.any(np.array(pos_list) < 0):
            raise RuntimeError('Negative frame positions (entries in pos_list) are not allowed.')
        pmin = np.min(pos_list, axis=0)
        if not np.all(pmin == 0):
            raise RuntimeError('Positions should start at 0.')
        self._pos_list = pos_list

        self._max_shift = int(max_shift)
        self._padding = self._max_shift + Nw + self.safe_crop      # model.pyx:286
        self._Nw = Nw
        self._subpx = -1
        self._refshift = 0
        win = self._make_window(Nw)

        dims = np.ascontiguousarray(np.array(self._shape_list, dtype=np.int32).reshape(Na, 2))
        pos = np.ascontiguousarray(np.array(pos_list, dtype=np.int32).reshape(Na, 2))
        self._fs = (_lib.FrameSet(self._sam), _lib.FrameSet(self._ref),
                    _lib.FrameSet(self._mask) if self._mask is not None else None)
        on_device = hasattr(self._sam[0], "data_ptr")
        args = [self._kind, Na, _lib._ptr(dims, _lib._ip), self._fs[0].table, self._fs[1].table,
                self._fs[2].table if self._fs[2] is not None else None,
                _lib._ptr(pos, _lib._ip), Nw, _lib._ptr(win, _lib._dp), self._max_shift, self._padding]
        if self._lib.is_hip:
            args += [self._device, _lib.F_DEVICE_FRAMES if on_device else 0]
        self._handle = self._lib.create(*args)
        if not self._handle:
            raise RuntimeError("could not create the native model: %s" % self._lib.error())
        self._ROI = None
        self._set_ROI(ROI)

    def __del__(self):
        h, self._handle = getattr(self, "_handle", None), None
        if h:
            self._lib.destroy(h)

    def update_frames(self, sam_list=None, ref_list=None):
        """Swap in new sample and/or reference stacks of the same shapes without rebuilding the model
        (extension: the reference rebuilds a model per projection, ``umpa_multi.py:149``).  On the GPU
        the untouched stack stays resident.  The last stack wins: a sample stack given here drops one that ``stage_sample``
        uploaded and no call has adopted yet; ``ref_list`` alone leaves it pending."""
        new_sam = self._prepare_frames(sam_list) if sam_list is not None else None
        new_ref = self._prepare_frames(ref_list) if ref_list is not None else None
        for new in (new_sam, new_ref):
            if new is not None and [tuple(x.shape) for x in new] != [tuple(x.shape) for x in self._sam]:
                raise RuntimeError('update_frames needs stacks of the shapes the model was built with.')
        if not self._lib.is_hip or hasattr(self._sam[0], "data_ptr"):
            raise RuntimeError('update_frames needs a model that owns device copies of host frames.')
        fs_s = _lib.FrameSet(new_sam) if new_sam is not None else None
        fs_r = _lib.FrameSet(new_ref) if new_ref is not None else None
        self._lib.check(self._lib.update_frames(self._handle, fs_s.table if fs_s else None,
                                                fs_r.table if fs_r else None), "update_frames")
        if new_sam is not None:
            self._sam, self._sam_list = new_sam, sam_list
            self._use_staged = self._sam_staged = False            # (the library dropped a pending staged stack too)
        if new_ref is not None:
            self._ref, self._ref_list = new_ref, ref_list
        self._fs = (_lib.FrameSet(self._sam), _lib.FrameSet(self._ref), self._fs[2])

    # -- input handling
    def _check_contiguous(self, a):
        if any(not (x.is_contiguous() if hasattr(x, "is_contiguous") else x.flags.c_contiguous) for x in a):
            raise RuntimeError('The provided image frames are not C-contiguous.')      # model.pyx:311-317

    def _prepare_frames(self, frames):
        frames = list(frames)
        if len(frames) and hasattr(frames[0], "data_ptr"):          # torch tensors already on the GPU
            for x in frames:
                if not x.is_cuda or str(x.dtype) != "torch.float64" or x.dim() != 2:
                    raise RuntimeError('device frames must be 2-D float64 CUDA/HIP tensors.')
            self._check_contiguous(frames)
            return frames
        frames = [np.asarray(x) for x in frames]
        self._check_contiguous(frames)
        out = []
        for x in frames:
            if x.ndim != 2:
                raise RuntimeError('frames must be two-dimensional.')
            out.append(x if x.dtype == NPDOUBLE else np.ascontiguousarray(x, dtype=NPDOUBLE))
        return out

    def _make_window(self, n):                                      # model.pyx:691-696
        window = np.multiply.outer(np.hamming(2 * n + 1), np.hamming(2 * n + 1))
        window /= window.sum()
        self._window = np.ascontiguousarray(window, dtype=NPDOUBLE)
        return self._window

    # -- single-pixel entry points
    def _min(self, i, j, values):
        uv = np.zeros(2)                                            # Model.cpp:316-321
        self._lib.check(self._lib.min(self._handle, int(i), int(j), _lib._ptr(values, _lib._dp),
                                      _lib._ptr(uv, _lib._dp), None, None, None), "min")

    def min(self, x, y):
        raise NotImplementedError

    # -- ROI / extent arithmetic (model.pyx:531-623)
    def _calculate_extent(self):
        padding = self._padding
        pmax = np.max(np.array(self._pos_list) + np.array(self._shape_list), axis=0)
        N0 = 1 + (pmax[0] - 2 * padding - 1)
        N1 = 1 + (pmax[1] - 2 * padding - 1)
        return int(N0), int(N1)

    def _convert_ROI_slice(self, ROI=None, step=None):
        return _roi_slices(self._calculate_extent(), ROI, step, self._ROI)

    def _set_ROI(self, ROI=None):
        N0, N1 = self._calculate_extent()
        if ROI is None:
            self._ROI = ((0, N0, 1), (0, N1, 1))
        else:
            s0, s1 = ROI
            if type(s0) is slice:
                s0 = s0.indices(N0)
            if type(s1) is slice:
                s1 = s1.indices(N1)
            self._ROI = (tuple(int(v) for v in s0), tuple(int(v) for v in s1))

    def set_step(self, step):
        self._set_ROI(ROI=self._convert_ROI_slice(step=step))
        return self._ROI

    def coords(self, ROI=None):
        offset = self.padding
        if ROI is not None:
            s0, s1 = self._convert_ROI_slice(ROI=ROI)
        else:
            s0, s1 = self._ROI
        return offset + np.arange(*s0), offset + np.arange(*s1)

    def test(self):                                                 # ModelBase::test, Model.cpp:226-234
        return float(len(self._sam))

    _counts = staticmethod(_roi_counts)

    def _check_range(self, s0, s1, N0, N1):
        _roi_check_range(self._calculate_extent(), s0, s1, N0, N1)

    def _region(self, ROI=None, step=None, ROI_wins=False):
        """``resolve_region`` on this model: the default region is the remembered ROI.  ``ROI_wins``: ``step`` is ignored
        beside ``ROI``, as ``match()`` ignores it, where ``coverage()`` refuses the pair."""
        if ROI_wins and ROI is not None:
            step = None
        return resolve_region(self._calculate_extent(), ROI, step, self._ROI)

    # -- coverage (model.pyx:499-529)
    def _one_frame_box(self):
        """All frames of one shape at position (0, 0)."""
        sh0 = tuple(self._shape_list[0])
        return all(tuple(p) == (0, 0) for p in self._pos_list) and all(tuple(s) == sh0 for s in self._shape_list)

    def _trivial_coverage(self):
        if self._mask is not None:
            return False
        return self._one_frame_box()

    def _masked_admitted(self):
        """A model with masks whose ``masked_grid`` switch is on (a stub without the attribute counts as off)."""
        return self._mask is not None and bool(getattr(self, "_masked_grid", False))

    def _general_admitted(self):
        """The ``general_grid`` switch is on (a stub without the attribute counts as off)."""
        return bool(getattr(self, "_general_grid", False))

    def _goes_general(self):
        """With ``general_grid`` on: the model is one the tiled paths never take whole, so its grid consumers run on the general
        table (steps and search ranges past the tiled limits go there too, but only the library knows those)."""
        return self._general_admitted() and ((self._mask is not None and not self._masked_admitted())
                                             or not self._one_frame_box() or bool(self._force & _lib.F_FORCE_DIRECT))

    def _marks_covered(self):
        """The consumers without a coverage argument compute every pixel and return ``covered``: an admitted masked model, or a
        model on the general table whose coverage is not trivial."""
        return self._masked_admitted() or (self._goes_general() and not self._trivial_coverage())

    def _covered(self, s0, s1):
        """``coverage >= thr`` on the region, with the threshold of ``match()`` (model.pyx:431): a numpy bool ``[N0, N1]``."""
        covermap = self.coverage(ROI=(s0, s1))
        return covermap >= .1 * covermap.max() / len(self._sam)

    def _no_masked_widening(self, what):
        if self._goes_general():
            raise RuntimeError("%s: not available on the general table (general_grid): it holds finished costs, and a finished cost is "
                               "not linear in the windowed sums, so a box average of costs is not the cost under a wider window" % what)
        if self._masked_admitted():
            raise RuntimeError("%s: not available on a masked model: its table holds finished costs, and a finished cost is not "
                               "linear in the windowed sums, so a box average of costs is not the cost under a wider window" % what)

    def coverage(self, step=None, ROI=None):
        s0, s1, N0, N1 = self._region(ROI, step)
        cmap = np.zeros((N0, N1), dtype=NPDOUBLE)
        if self._lib.is_hip:
            self._lib.check(self._lib.coverage_region(self._handle, s0[0], s0[2], N0, s1[0], s1[2], N1,
                                                      _lib._ptr(cmap, _lib._dp)), "coverage")
        else:
            off = self._padding
            one = np.zeros(1)
            for xi in range(N0):
                for xj in range(N1):
                    self._lib.coverage(self._handle, _lib._ptr(one, _lib._dp),
                                       off + s0[0] + s0[2] * xi, off + s1[0] + s1[2] * xj)
                    cmap[xi, xj] = one[0]
        return cmap

    # -- the match loop (model.pyx:334-497)
    def _match(self, step=None, input_values=None, dxdy=None, ROI=None,
               num_threads=None, quiet=False, search='walk', widen=0):
        if search not in ('walk', 'grid'):
            raise ValueError("search must be 'walk' or 'grid', not %r" % (search,))
        widen = check_widen(widen, search)
        grid = search == 'grid'
        if grid:
            self._grid_check("search='grid'")
            if widen:
                self._no_masked_widening("search='grid', widen=%d" % widen)
            if dxdy is not None:
                raise RuntimeError("search='grid' looks at every shift of the search box: start shifts (dxdy) mean nothing to it")
        if (ROI is not None) and (step is not None):
            print("Warning: 'ROI' and 'step' parameters are set simultaneously. "
                  "'step' parameter is ignored.")
            step = None
        if not quiet:
            if self._lib.is_hip:
                print("Using HIP device %d" % self._device)
        self._set_ROI(self._convert_ROI_slice(ROI, step))                # remembered before it is checked, as in the reference
        s0, s1, N0, N1 = self._region()
        wide = None
        if widen:                                                   # the call is made on a grown region and cropped below
            wide = widen_region(self._calculate_extent(), s0, s1, N0, N1, widen)
            s0, s1, N0, N1 = wide[0]
        sh = (N0, N1)
        shp = (N0, N1, self.Nparam)
        planar = False

        if self._trivial_coverage():
            covermap = None                                         # == Na everywhere: nothing is skipped
            thr = 0.0
        else:
            covermap = self.coverage(ROI=(s0, s1))
            thr = .1 * covermap.max() / len(self._sam)              # model.pyx:431

        if input_values is not None:                                # model.pyx:442-455
            if input_values.shape != shp:
                raise RuntimeError("Input values have the wrong shape: "
                                   "%s, should be %s" % (input_values.shape, shp))
            if input_values.dtype != np.float64:
                raise RuntimeError("Input values have the wrong type: "
                                   "%s, should be %s" % (input_values.dtype, np.float64))
            values = np.ascontiguousarray(input_values)
        elif self._lib.is_hip:
            # one plane per map: the device writes the result maps directly (no host-side de-interleaving)
            planar = True
            shp = (self.Nparam, N0, N1)
            values = self._alloc(shp, NPDOUBLE, covermap is not None)
        else:
            values = np.zeros(shp, dtype=NPDOUBLE)

        uv = None
        if dxdy is not None:                                        # model.pyx:461-465
            uv = np.zeros((N0, N1, 2), dtype=NPDOUBLE)
            uv[:, :, 0] = dxdy[0]
            uv[:, :, 1] = dxdy[1]
        if self._lib.is_hip:                                        # page-locked: downloaded at PCIe rate, chunk by chunk
            err = self._alloc(sh, np.int32, covermap is not None)
        else:
            err = np.zeros(sh, dtype=np.int32)
        result = {}
        dd = da = dn = None
        if self.debug:                                              # debug = "ncalls": only the evaluation counts
            mk = (lambda shape, dt: self._alloc(shape, dt, covermap is not None)) if self._lib.is_hip else \
                 (lambda shape, dt: np.zeros(shape, dtype=dt))
            if self.debug != "ncalls":
                dd = mk(sh + (25,), NPDOUBLE)
                da = mk(sh + (16,), NPDOUBLE)
            dn = mk(sh, np.int32)

        vp = lambda a: a.ctypes.data if a is not None else None
        args = [self._handle, s0[0], s0[2], N0, s1[0], s1[2], N1, vp(values), self.Nparam, vp(uv), vp(err),
                vp(covermap), float(thr), vp(dd), vp(da), vp(dn)]
        if self._lib.is_hip:
            flags = self._match_flags() | (_lib.F_PLANAR if planar else 0)
            if not hasattr(self._sam[0], "data_ptr"):               # frames owned by the library: it knows when the
                flags |= _lib.F_REUSE_REF_MAPS                      # reference stack changed (update_frames, Nw)
            args += [flags, None]
        else:
            if uv is None:
                uv = np.zeros((N0, N1, 2), dtype=NPDOUBLE)
                args[9] = vp(uv)
            args += [int(num_threads) if num_threads else max(1, self._lib.max_threads())]
        if grid:
            try:
                if wide:
                    _lib.grid().check(_lib.grid().wide_match_region(*(args[:7] + [widen] + args[7:])), "grid wide_match_region")
                else:
                    _lib.grid().check(_lib.grid().match_region(*args), "grid match_region")
            except _lib.NativeError as e:
                raise RuntimeError("search='grid': %s" % e) from None
        else:
            self._lib.check(self._lib.match_region(*args), "match_region")

        if wide:                                                    # (planar on this path: the maps' last axes are the pixels)
            r0, r1 = wide[1]
            if planar:
                values = _cropped(values, wide[1])
            else:
                values = np.ascontiguousarray(values[r0, r1])
            err = _cropped(err, wide[1])
            dd, da = [None if a is None else np.ascontiguousarray(a[r0, r1]) for a in (dd, da)]
            dn = None if dn is None else _cropped(dn, wide[1])
            result['region'] = wide[2]
        result['values'] = values
        result['_planar'] = planar
        result['err'] = err
        if self.debug:
            if dd is not None:
                result['debug_d'] = dd
                result['debug_a'] = da
            result['debug_Ncalls'] = dn
        return result

    # -- the exhaustive table's other consumers (include/umpa_grid.h)
    def _grid_check(self, what):
        """The grid kernels read the plain tiled path's table: what that path never takes whole is refused here by name,
        the rest (steps, search ranges) by the library."""
        why = None
        if not self._lib.is_hip:
            why = "it runs on the HIP library only"
        elif self._kind == KIND_DFKERNEL:
            why = "the kernel dark-field model has no shift table"
        elif self._general_admitted():
            # the general table takes masks, positions, shapes and a forced direct kernel; a forced model's consumers other
            # than match() pass no force flag, so the library's switch carries the wish
            if getattr(self, "_handle", None) is not None:
                always = 2 if self._force & _lib.F_FORCE_DIRECT else 0
                _lib.grid().check(_lib.grid().set_general(self._handle, 1 | always), "grid set_general")
        elif self._mask is not None and not self._masked_admitted():
            why = "masked models are not supported (their table holds finished costs)"
        elif not self._one_frame_box():
            why = "frames at different positions (pos_list) or of different shapes are not supported"
        elif self._force & _lib.F_FORCE_DIRECT:
            why = "the model is forced onto the direct kernel"
        if why:
            raise RuntimeError("%s (grid search / cost volume): %s" % (what, why))

    def _grid_cost_volume(self, ROI, step, alloc, widen=0):
        """The one ``umpa_grid_cost_volume`` call.  ``alloc(U, N0, N1)`` gives the output arrays once the model and the region
        have passed, as a dictionary of ``cost`` and, where wanted, ``T`` and ``df``: host arrays, or HIP tensors that the
        library fills on the current stream.  This call is given the staged stack, so it spends the one-shot flag.
        Returns ``(s0, s1, arrays)``.  ``widen`` > 0 (window widening): ``alloc`` is asked for the grown region's arrays,
        and what comes back is the kept region (``widen_region``) and contiguous copies of its part of the arrays."""
        self._grid_check("cost_volume")
        widen = check_widen(widen)
        if widen:
            self._no_masked_widening("cost_volume, widen=%d" % widen)
        s0, s1, N0, N1 = self._region(ROI, step, ROI_wins=True)
        wide = widen_region(self._calculate_extent(), s0, s1, N0, N1, widen) if widen else None
        if wide:
            s0, s1, N0, N1 = wide[0]
        out = alloc(2 * self._max_shift - 1, N0, N1)
        _, flags, stream = _lib.Side(out['cost'], device=self._device).tail(self._staged_flag())
        region = (self._handle, s0[0], s0[2], N0, s1[0], s1[2], N1)
        tail = [_lib.Side.ptr(out.get(k)) for k in ('cost', 'T', 'df')] + [flags, stream]
        try:
            if wide:
                _lib.grid().check(_lib.grid().wide_cost_volume(*region, widen, *tail), "grid wide_cost_volume")
            else:
                _lib.grid().check(_lib.grid().cost_volume(*region, *tail), "grid cost_volume")
        except _lib.NativeError as e:
            raise RuntimeError("cost_volume: %s" % e) from None
        if wide:
            return wide[2][0], wide[2][1], {k: _cropped(v, wide[1]) for k, v in out.items()}
        return s0, s1, out

    def _cost_volume(self, ROI=None, step=None, with_fit=False, widen=0):
        keys = ['cost'] + (['T'] + (['df'] if self._kind == KIND_DF else []) if with_fit else [])
        s0, s1, out = self._grid_cost_volume(ROI, step, lambda U, N0, N1: {k: np.empty((U, U, N0, N1), dtype=NPDOUBLE) for k in keys}, widen)
        if widen:
            out['region'] = (s0, s1)
        if self._marks_covered():                                   # every pixel is computed: what match() would have skipped is marked
            out['covered'] = self._covered(s0, s1)
        return out

    def _grid_basins(self, k, ROI, step, alloc, widen=0):
        """The one ``umpa_grid_basins`` call.  ``alloc(k, N0, N1)`` gives the output arrays once the model, ``k`` and the region
        have passed: a dictionary of ``f``, ``T``, ``dx``, ``dy``, ``cost`` (and ``df``: dark-field model) as float64
        ``[k, N0, N1]``, ``si``, ``sj``, ``err`` as int32 ``[k, N0, N1]`` and ``count`` as int32 ``[N0, N1]`` -- host arrays, or
        HIP tensors that the library fills on the current stream.  This call is given the staged stack, so it spends the
        one-shot flag.  Returns ``(s0, s1, arrays)``.  ``widen`` as for ``_grid_cost_volume``."""
        self._grid_check("basins")
        widen = check_widen(widen)
        if widen:
            self._no_masked_widening("basins, widen=%d" % widen)
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not _lib.GRID_MIN_K <= k <= _lib.GRID_MAX_K:
            raise ValueError("basins: k must be an integer from %d to %d, not %r" % (_lib.GRID_MIN_K, _lib.GRID_MAX_K, k))
        k = int(k)
        s0, s1, N0, N1 = self._region(ROI, step, ROI_wins=True)
        wide = widen_region(self._calculate_extent(), s0, s1, N0, N1, widen) if widen else None
        if wide:
            s0, s1, N0, N1 = wide[0]
        out = alloc(k, N0, N1)
        _, flags, stream = _lib.Side(out['cost'], device=self._device).tail(self._staged_flag())
        names = ('f', 'T', 'dx', 'dy', 'cost', 'df', 'si', 'sj', 'err', 'count')
        region = (self._handle, s0[0], s0[2], N0, s1[0], s1[2], N1)
        tail = [k] + [_lib.Side.ptr(out.get(n)) for n in names] + [flags, stream]
        try:
            if wide:
                _lib.grid().check(_lib.grid().wide_basins(*region, widen, *tail), "grid wide_basins")
            else:
                _lib.grid().check(_lib.grid().basins(*region, *tail), "grid basins")
        except _lib.NativeError as e:
            raise RuntimeError("basins: %s" % e) from None
        if wide:
            return wide[2][0], wide[2][1], {n: _cropped(v, wide[1]) for n, v in out.items()}
        return s0, s1, out

    def _basins(self, k=4, ROI=None, step=None, widen=0):
        dbl = ['f', 'T', 'dx', 'dy', 'cost'] + (['df'] if self._kind == KIND_DF else [])

        def alloc(k, N0, N1):                                      # page-locked, as the result maps of match(): downloaded at PCIe rate
            out = {n: _lib.pinned_empty((k, N0, N1), NPDOUBLE) for n in dbl}
            out.update({n: _lib.pinned_empty((k, N0, N1), np.int32) for n in ('si', 'sj', 'err')})
            out['count'] = _lib.pinned_empty((N0, N1), np.int32)
            return out

        s0, s1, out = self._grid_basins(k, ROI, step, alloc, widen)
        out['shift'] = np.stack([out.pop('si'), out.pop('sj')], axis=1)
        if widen:
            out['region'] = (s0, s1)
        if self._marks_covered():
            out['covered'] = self._covered(s0, s1)
        return out

    def _grid_track(self, prior, mode, lam, radius, ROI, step, alloc, widen=0):
        """The one ``umpa_grid_track`` call.  ``prior(N0, N1)`` gives the two prior planes (row shift, column shift) and
        ``alloc(N0, N1)`` the output arrays once the model and the region have passed: float64 ``[N0, N1]`` each, the
        outputs a dictionary of ``f``, ``T``, ``dx``, ``dy``, ``cost``, ``cost0`` (and ``df``: dark-field model) as float64 and
        ``si``, ``sj``, ``err``, ``count``, ``found`` as int32 -- all host arrays, or all HIP tensors that the library reads and
        fills on the current stream.  This call is given the staged stack, so it spends the one-shot flag.
        Returns ``(s0, s1, arrays)``.  ``widen`` as for ``_grid_cost_volume``; ``prior`` is asked for planes of the KEPT
        region, which go into NaN planes of the grown one (its other pixels have no basin anyway)."""
        self._grid_check("track")
        widen = check_widen(widen)
        if widen:
            self._no_masked_widening("track, widen=%d" % widen)
        s0, s1, N0, N1 = self._region(ROI, step, ROI_wins=True)
        wide = widen_region(self._calculate_extent(), s0, s1, N0, N1, widen) if widen else None
        if wide:
            s0, s1, N0, N1 = wide[0]
            kept = prior(wide[1][0].stop - wide[1][0].start, wide[1][1].stop - wide[1][1].start)
            pi, pj = [_grown(p, (N0, N1), wide[1]) for p in kept]
        else:
            pi, pj = prior(N0, N1)
        out = alloc(N0, N1)
        _, flags, stream = _lib.Side(pi, pj, *out.values(), device=self._device,
                                     mixed="track: the priors and the outputs must be all host arrays or all HIP tensors").tail(self._staged_flag())
        names = ('f', 'T', 'dx', 'dy', 'cost', 'df', 'si', 'sj', 'err', 'cost0', 'count', 'found')
        region = (self._handle, s0[0], s0[2], N0, s1[0], s1[2], N1)
        tail = [_lib.Side.ptr(pi), _lib.Side.ptr(pj), int(mode), float(lam), float(radius)] + [_lib.Side.ptr(out.get(n)) for n in names] + [flags, stream]
        try:
            if wide:
                _lib.grid().check(_lib.grid().wide_track(*region, widen, *tail), "grid wide_track")
            else:
                _lib.grid().check(_lib.grid().track(*region, *tail), "grid track")
        except _lib.NativeError as e:
            raise RuntimeError("track: %s" % e) from None
        if wide:
            return wide[2][0], wide[2][1], {n: _cropped(v, wide[1]) for n, v in out.items()}
        return s0, s1, out

    def _track(self, prior_dx, prior_dy, lam=None, radius=None, ROI=None, step=None, widen=0):
        self._grid_check("track")
        number = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))
        if lam is not None and not (number(lam) and 0.0 <= float(lam) < np.inf):
            raise ValueError("track: lam must be None (the nearest basin) or a finite number >= 0, not %r" % (lam,))
        if radius is not None and not (number(radius) and float(radius) >= 0.0):
            raise ValueError("track: radius must be None (no limit) or a number >= 0, not %r" % (radius,))
        mode = _lib.GRID_TRACK_NEAREST if lam is None else _lib.GRID_TRACK_PENALTY
        given = (prior_dy, prior_dx)                                # the library's order: row shift first
        on_device = [hasattr(p, "data_ptr") for p in given]
        if any(on_device) and not all(d or np.ndim(p) == 0 for p, d in zip(given, on_device)):
            raise ValueError("track: the priors must be both numpy arrays (or scalars) or both HIP tensors")
        dev = next((p.device for p, d in zip(given, on_device) if d), None)

        def prior(N0, N1):
            planes = []
            for p, d in zip(given, on_device):
                shape = tuple(p.shape) if d else np.shape(p)
                if shape not in ((), (N0, N1)):
                    raise ValueError("track: a prior must be a scalar or of shape %s, not %s" % ((N0, N1), shape))
                if d:
                    import torch
                    if p.dtype != torch.float64 or not p.is_cuda or p.device.index != self._device:
                        raise ValueError("track: a device prior must be a float64 HIP tensor on the model's device")
                    planes.append(p.expand(N0, N1).contiguous())
                elif dev is not None:
                    import torch
                    planes.append(torch.full((N0, N1), float(p), dtype=torch.float64, device=dev))
                else:
                    a = np.asarray(p)
                    if a.dtype.kind not in "fiu":
                        raise ValueError("track: a prior must be of a real number type, not %s" % a.dtype)
                    planes.append(np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=NPDOUBLE), (N0, N1))))   # (no copy of a float64 plane)
            return planes

        dbl = ['f', 'T', 'dx', 'dy', 'cost', 'cost0'] + (['df'] if self._kind == KIND_DF else [])
        ints = ('si', 'sj', 'err', 'count', 'found')

        def alloc(N0, N1):
            if dev is not None:
                import torch
                out = {n: torch.empty((N0, N1), dtype=torch.float64, device=dev) for n in dbl}
                out.update({n: torch.empty((N0, N1), dtype=torch.int32, device=dev) for n in ints})
                return out
            out = {n: _lib.pinned_empty((N0, N1), NPDOUBLE) for n in dbl}   # page-locked, as the result maps of match()
            out.update({n: _lib.pinned_empty((N0, N1), np.int32) for n in ints})
            return out

        s0, s1, out = self._grid_track(prior, mode, 0.0 if lam is None else lam, -1.0 if radius is None else radius, ROI, step, alloc, widen)
        if widen:
            out['region'] = (s0, s1)
        si, sj, err = out.pop('si'), out.pop('sj'), out.pop('err')
        if dev is not None:
            import torch
            out['shift'] = torch.stack([si, sj], dim=0)
            out['err'] = torch.clamp(err, min=0)
        else:
            out['shift'] = np.stack([si, sj], axis=0)
            out['err'] = np.maximum(err, 0)
        if self._marks_covered():
            out['covered'] = self._covered(s0, s1)
        return out

    def _grid_sequence(self, state, lam, trunc, ROI, step, alloc):
        """The one ``umpa_grid_sequence`` call.  ``state(U, N0, N1)`` gives the previous state (float64 ``[U, U, N0, N1]``, or
        None: a series starts) and ``alloc(U, N0, N1)`` the output arrays once the model and the region have passed: a
        dictionary of ``state`` (the next state, float64 ``[U, U, N0, N1]``), ``f``, ``T``, ``dx``, ``dy``, ``cost``, ``total``,
        ``cost0`` (and ``df``: dark-field model) as float64 ``[N0, N1]`` and ``si``, ``sj``, ``err``, ``moved`` as int32 -- all host
        arrays, or all HIP tensors that the library reads and fills on the current stream.  This call is given the staged
        stack, so it spends the one-shot flag.  Returns ``(s0, s1, arrays)``."""
        self._grid_check("sequence")
        s0, s1, N0, N1 = self._region(ROI, step, ROI_wins=True)
        U = 2 * self._max_shift - 1
        prev = state(U, N0, N1)
        out = alloc(U, N0, N1)
        _, flags, stream = _lib.Side(prev, *out.values(), device=self._device,
                                     mixed="sequence: the state and the outputs must be all host arrays or all HIP tensors").tail(self._staged_flag())
        names = ('f', 'T', 'dx', 'dy', 'cost', 'df', 'si', 'sj', 'err', 'total', 'cost0', 'moved')
        args = [self._handle, s0[0], s0[2], N0, s1[0], s1[2], N1, _lib.Side.ptr(prev), float(lam), float(trunc), _lib.Side.ptr(out.get('state'))]
        args += [_lib.Side.ptr(out.get(n)) for n in names] + [flags, stream]
        try:
            _lib.grid().check(_lib.grid().sequence(*args), "grid sequence")
        except _lib.NativeError as e:
            raise RuntimeError("sequence: %s" % e) from None
        return s0, s1, out

    def _sequence(self, state=None, lam=None, trunc=None, ROI=None, step=None, out=None):
        self._grid_check("sequence")
        if not _lib.GRID_SEQUENCE_MIN_MS <= self._max_shift <= _lib.GRID_SEQUENCE_MAX_MS:
            raise RuntimeError("sequence: max_shift must be %d to %d, not %d" % (_lib.GRID_SEQUENCE_MIN_MS, _lib.GRID_SEQUENCE_MAX_MS, self._max_shift))
        number = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))
        if not (number(lam) and 0.0 <= float(lam) < np.inf):
            raise ValueError("sequence: lam must be a finite number >= 0, not %r" % (lam,))
        if trunc is not None and not (number(trunc) and float(trunc) >= 0.0):
            raise ValueError("sequence: trunc must be None (no truncation) or a number >= 0, not %r" % (trunc,))
        given = [a for a in (state, out) if a is not None]
        on_device = [hasattr(a, "data_ptr") for a in given]
        if any(on_device) and not all(on_device):
            raise ValueError("sequence: state and out must be both numpy arrays or both HIP tensors")
        dev = given[0].device if any(on_device) else None

        def held(a, what, U, N0, N1):
            """`a` as the library takes a state: float64 [U, U, N0, N1], contiguous, on the call's side"""
            shape = tuple(a.shape) if dev is not None else np.shape(a)
            if shape != (U, U, N0, N1):
                raise ValueError("sequence: %s must be of shape %s, not %s" % (what, (U, U, N0, N1), shape))
            if dev is not None:
                import torch
                if a.dtype != torch.float64 or not a.is_cuda or a.device.index != self._device or not a.is_contiguous():
                    raise ValueError("sequence: a device %s must be a contiguous float64 HIP tensor on the model's device" % what)
                return a
            if np.asarray(a).dtype.kind not in "fiu":
                raise ValueError("sequence: %s must be of a real number type, not %s" % (what, np.asarray(a).dtype))
            return a

        def prev(U, N0, N1):
            if state is None:
                return None
            a = held(state, "state", U, N0, N1)
            return a if dev is not None else np.ascontiguousarray(a, dtype=NPDOUBLE)   # (no copy of a float64 array)

        dbl = ['f', 'T', 'dx', 'dy', 'cost', 'total', 'cost0'] + (['df'] if self._kind == KIND_DF else [])
        ints = ('si', 'sj', 'err', 'moved')

        def alloc(U, N0, N1):
            if out is not None:
                nxt = held(out, "out", U, N0, N1)
                if dev is None and not (isinstance(out, np.ndarray) and out.dtype == NPDOUBLE and out.flags.c_contiguous):
                    raise ValueError("sequence: a host out must be a C-contiguous float64 numpy array")
                if state is not None and _lib.Side.ptr(nxt) == _lib.Side.ptr(state):
                    raise ValueError("sequence: out must not be the state itself (the call reads the one while it writes the other)")
            if dev is not None:
                import torch
                res = {'state': out if out is not None else torch.empty((U, U, N0, N1), dtype=torch.float64, device=dev)}
                res.update({n: torch.empty((N0, N1), dtype=torch.float64, device=dev) for n in dbl})
                res.update({n: torch.empty((N0, N1), dtype=torch.int32, device=dev) for n in ints})
                return res
            res = {'state': out if out is not None else np.empty((U, U, N0, N1), dtype=NPDOUBLE)}
            res.update({n: _lib.pinned_empty((N0, N1), NPDOUBLE) for n in dbl})   # page-locked, as the result maps of match()
            res.update({n: _lib.pinned_empty((N0, N1), np.int32) for n in ints})
            return res

        s0, s1, res = self._grid_sequence(prev, lam, np.inf if trunc is None else trunc, ROI, step, alloc)
        si, sj, err = res.pop('si'), res.pop('sj'), res.pop('err')
        if dev is not None:
            import torch
            res['shift'] = torch.stack([si, sj], dim=0)
            res['err'] = torch.clamp(err, min=0)
        else:
            res['shift'] = np.stack([si, sj], axis=0)
            res['err'] = np.maximum(err, 0)
        if self._marks_covered():
            res['covered'] = self._covered(s0, s1)
        return res

    _general_grid = False

    @property
    def general_grid(self):
        """The opt-in switch of the grid consumers for everything the tiled paths do not take whole (extension;
        ``include/umpa_grid.h``: ``umpa_grid_set_general``), ``False`` by default.  While it is ``False``, ``match(search='grid')``,
        ``cost_volume``, ``basins``, ``track`` and ``sequence`` (and ``Tracker``, ``Sequence``, ``match_smooth``) refuse what they always
        refused, with the same texts.  Set to ``True``, they also take frames at different positions (``pos_list``, sample stepping)
        or of unequal shapes, a model forced onto the direct kernel, a masked model whose ``masked_grid`` is off or that the masked
        path does not admit, and steps and search ranges past the tiled limits: the library fills a table of finished costs
        by the reference's own window x frame sum -- ``cost(i, j, sx, sy)`` bit for bit, at about 38 times the tiled path's
        arithmetic per pixel -- and the same consumers run on it.  What a tiled path takes whole keeps going there.
        Where coverage is not trivial, ``match(search='grid')`` skips the pixels below the coverage threshold as ``match()`` does; the
        others compute every pixel (NaN costs where no frame contributes) and return one more key, ``covered``.  ``widen > 0``,
        ``coarse_to_fine`` and ``scale_space`` are refused on a model that goes this way: a finished cost is not linear in the
        windowed sums.  Not on the kernel dark-field model (it has no per-shift table), not on the CPU library."""
        return bool(self._general_grid)

    @general_grid.setter
    def general_grid(self, on):
        on = bool(on)
        if on and self._kind == KIND_DFKERNEL:
            raise RuntimeError("general_grid: the kernel dark-field model has no shift table")
        if on and not self._lib.is_hip:
            raise RuntimeError("general_grid: it runs on the HIP library only")
        if self._lib.is_hip and self._kind != KIND_DFKERNEL and getattr(self, "_handle", None) is not None:
            always = 2 if on and self._force & _lib.F_FORCE_DIRECT else 0
            _lib.grid().check(_lib.grid().set_general(self._handle, (1 | always) if on else 0), "grid set_general")
        self._general_grid = on

    _force = 0
    _use_staged = False
    _sam_staged = False        # the sample stack came from stage_sample: self._sam is not the stack the library matches
    _async = False
    _out_alloc = None           # hook (shape, dtype, zero) -> array for the result maps (farm.py: shared-memory result slots)

    def _alloc(self, shape, dtype, zero):
        if self._out_alloc is not None:
            return self._out_alloc(shape, dtype, zero)
        return _lib.pinned_empty(shape, dtype, zero=zero)

    def match_async(self, **kw):
        """``match()`` that returns as soon as the kernels and the downloads are enqueued (HIP only); the maps of the
        returned dictionary are valid after ``wait()``.  Lets a caller upload the next projection meanwhile."""
        self._async = True
        try:
            return self.match(**kw)
        finally:
            self._async = False

    def wait(self):
        self._lib.check(self._lib.wait(self._handle), "wait")

    def _staged_flag(self):
        """F_USE_STAGED once after stage_sample: the staged stack is adopted by the call that is given it"""
        if not self._use_staged:
            return 0
        self._use_staged = False
        return _lib.F_USE_STAGED

    def _match_flags(self):
        f = self._force
        if self._async:
            f |= _lib.F_ASYNC
        return f | self._staged_flag()

    def stage_sample(self, raw_frames, dark=None, flat=None):
        """Upload the NEXT sample stack while the current match is still running (extension; the reference builds a
        new model per projection, ``umpa_multi.py:149``).  ``raw_frames``: host frames of the model's shapes, float64 /
        float32 / uint16 (page-locked arrays -- ``_lib.pinned_empty`` -- make this return at once); ``dark`` / ``flat``:
        device float64 stacks (lists of 2-D HIP tensors) for the fused ``(raw - dark) / flat`` of ``umpa_multi.py:144``.
        The staged stack becomes the sample stack of the next call that reads the sample stack -- ``match()``,
        ``cost_volume()``, ``basins()``, ``track()``, ``sequence()``, ``match_smooth`` -- and stays it.  The last stack wins: another ``stage_sample`` or
        ``update_frames(sam_list=...)`` before that call replaces it.  The model keeps no host copy of a staged stack:
        ``uncertainty()`` then needs it as ``sam=``, or ``resident=True``, which reads the adopted stack on the device."""
        if not self._lib.is_hip or hasattr(self._sam[0], "data_ptr"):
            raise RuntimeError('stage_sample needs a model that owns device copies of host frames.')
        raw = [np.asarray(x) for x in raw_frames]
        if [tuple(x.shape) for x in raw] != [tuple(x.shape) for x in self._sam]:
            raise RuntimeError('stage_sample needs a stack of the shapes the model was built with.')
        code = {np.dtype(np.float64): 0, np.dtype(np.float32): 1, np.dtype(np.uint16): 2}.get(raw[0].dtype)
        if code is None or any(x.dtype != raw[0].dtype for x in raw):
            raise RuntimeError('raw frames must all be float64, float32 or uint16.')
        self._check_contiguous(raw)
        fs = _lib.FrameSet(raw)
        fd = _lib.FrameSet(list(dark)) if dark is not None else None
        ff = _lib.FrameSet(list(flat)) if flat is not None else None
        self._lib.check(self._lib.stage_sample(self._handle, fs.table, code, fd.table if fd else None,
                                               ff.table if ff else None), "stage_sample")
        self._staged_keep = (raw, dark, flat)                       # alive until the upload has been consumed
        self._use_staged = self._sam_staged = True

    def set_unwarp(self, unwarp_map):
        """Attach an ``umpa_amd.unwarp.UnwarpMap`` (or detach with None): while one is attached, ``stage_sample`` resamples
        every raw frame through it on the way into the sample buffer, then applies ``(u - dark) / flat``
        (``umpa_multi.py:130, :144``; ``include/umpa_unwarp.h``).  For models that own device copies of host frames, all of
        the map's shape, on the map's device.  ``match()`` on the frames the model was built with is not affected."""
        if not self._lib.is_hip:
            raise RuntimeError('set_unwarp needs the HIP library.')
        ulib = _lib.unwarp()
        if unwarp_map is not None and unwarp_map._handle is None:
            raise RuntimeError('the unwarp map was destroyed')
        ulib.check(ulib.attach(self._handle, unwarp_map._handle if unwarp_map is not None else None), "unwarp attach")
        self._unwarp = unwarp_map

    # -- properties (model.pyx:625-755)
    @property
    def extent(self):
        return self._calculate_extent()

    @property
    def ROI(self):
        return self._ROI

    @ROI.setter
    def ROI(self, new_ROI):
        self._set_ROI(new_ROI)

    @property
    def sh(self):
        s0, s1 = self._ROI
        return ((s0[1] - s0[0] - 1) // s0[2] + 1, (s1[1] - s1[0] - 1) // s1[2] + 1)

    @property
    def Na(self):
        return len(self._sam)

    @property
    def sam_list(self):
        return self._sam_list

    @property
    def ref_list(self):
        return self._ref_list

    @property
    def mask_list(self):
        return self._mask_list

    @property
    def shape_list(self):
        return self._shape_list

    @property
    def pos_list(self):
        return self._pos_list

    @property
    def window(self):
        return self._window

    @property
    def Nw(self):
        return self._Nw

    @Nw.setter
    def Nw(self, new_Nw):
        new_Nw = int(new_Nw)
        if new_Nw < 0:
            raise RuntimeError("Nw must be non-negative.")           # Model.cpp:242
        if new_Nw + self._max_shift + self.safe_crop > self._padding:
            raise RuntimeError("Nw=%d does not fit the padding %d fixed at construction "
                               "(the reference would read outside the frames)." % (new_Nw, self._padding))
        old = self._window
        win = self._make_window(new_Nw)
        rc = self._lib.set_window(self._handle, _lib._ptr(win, _lib._dp), new_Nw)
        if rc is not None and rc < 0:
            self._window = old
            raise RuntimeError(self._lib.error())
        self._Nw = new_Nw

    @property
    def max_shift(self):
        return self._max_shift

    @property
    def padding(self):
        return self._padding

    @property
    def assign_coordinates(self):
        return {0: 'sam', 1: 'ref'}[self._refshift]

    @assign_coordinates.setter
    def assign_coordinates(self, new_mode):
        opts = {'sam': 0, 'ref': 1}
        try:
            set_value = opts[new_mode]
        except (KeyError, TypeError):
            print('Option %s is not available, parameter was not changed.' % repr(new_mode))
        else:
            self._refshift = set_value
            self._lib.set_reference_shift(self._handle, set_value)

    @property
    def sub_pixel_mode(self):
        return self._subpx

    @sub_pixel_mode.setter
    def sub_pixel_mode(self, new_mode):
        self._subpx = int(new_mode)
        self._lib.set_subpx(self._handle, self._subpx)

    # -- packing shared by the subclasses (model.pyx:815-822, :881-889)
    def _unpack(self, result, with_df):
        values = result.pop('values')
        if result.pop('_planar', False):
            planes = values                                         # written plane by plane on the device
        else:
            # one pass over the interleaved array instead of one strided copy per map
            planes = np.ascontiguousarray(np.moveaxis(values[:, :, :5 if with_df else 4], 2, 0))
        result['f'], result['T'], result['dx'], result['dy'] = planes[0], planes[1], planes[2], planes[3]
        if with_df:
            result['df'] = planes[4]
        return result


class _UMPAModelPlain(UMPAModelBase):
    """What ``UMPAModelNoDF`` and ``UMPAModelDF`` share: their parameters are all outputs, ``Nparam`` of them, the last
    ``Nparam - 2`` being what ``cost()`` returns beside the cost."""
    safe_crop = 0

    def min(self, i, j):
        values = np.zeros((self.Nparam,), dtype=NPDOUBLE)
        self._min(i, j, values)
        return values

    def cost(self, i, j, sx, sy):
        """Cost, transmission and (dark-field model) dark-field at pixel (i, j) for the shift (sx rows, sy columns), rounded."""
        values = np.zeros(self.Nparam - 2)
        self._lib.check(self._lib.cost(self._handle, int(i), int(j), _cround(sx), _cround(sy),
                                       _lib._ptr(values, _lib._dp)), "cost")
        return tuple(values)

    def match(self, step=None, dxdy=None, ROI=None, num_threads=None, quiet=False, search='walk', widen=0):
        """``search='walk'`` (default): the reference's minimiser.  ``search='grid'`` (extension): the global minimum over
        all ``(2 max_shift - 1)^2`` integer shifts, then the same sub-pixel step around it (``include/umpa_grid.h``);
        no ``dxdy``; a model with masks only with ``masked_grid`` switched on, ``pos_list`` (sample stepping), unequal frame
        shapes and a forced direct kernel only with ``general_grid`` switched on.

        ``widen=b`` (1 to 8, with ``search='grid'``; also on ``cost_volume``, ``basins`` and ``track``): window widening
        (``include/umpa_grid.h``).  The shift table and the maps are averaged over the ``(2b + 1)^2`` dense pixels around each
        pixel before the search, which is the search of a model whose window is ``umpa_amd.widen.window(Nw, b)``, of
        half-width ``Nw + b`` -- on this model, without a new upload.  The result covers the requested pixels whose widened
        window fits the extent (``umpa_amd.widen.valid_region``) and has one more key, ``region``: the covered pixels as a
        row and a column ``(start, end, step)`` triple.  ``widen=0`` is the call without the keyword."""
        result = self._match(step=step, dxdy=dxdy, ROI=ROI, num_threads=num_threads, quiet=quiet, search=search, widen=widen)
        return self._unpack(result, self._kind == KIND_DF)

    def cost_volume(self, ROI=None, step=None, with_fit=False, widen=0):
        """The cost of EVERY integer shift of the search box at every pixel of the region (extension; the
        reference offers ``utils.get_cost``, a Python loop over ``cost()`` for one pixel): a dictionary with
        ``cost[U, U, N0, N1]``, ``U = 2 max_shift - 1``, where ``cost[si + max_shift - 1, sj + max_shift - 1, xi, xj]``
        is ``cost(i, j, si, sj)[0]`` of the region's pixel ``(xi, xj)`` (``si``: row shift, ``sj``: column shift) -- the
        numbers ``match()`` compares, bit for bit.  ``with_fit=True`` adds ``T`` and, for the dark-field model, ``df`` in
        the same layout.  ``ROI`` / ``step`` as for ``match()``; the model's own ROI is not changed.  A stack uploaded by
        ``stage_sample`` and not adopted yet is adopted by this call, as by ``match()``: the volume is that stack's.

        Mind the size: an array holds ``U * U * N0 * N1`` doubles -- 2.7 GB for a whole 2048 x 2048 image at
        ``max_shift=5`` -- so a ``ROI`` of the rows or the patch in question is the normal use.

        Models the plain tiled path takes whole only (no masks, no ``pos_list``, steps and search ranges within its
        limits); anything else raises ``RuntimeError``.  A model with masks is taken once ``masked_grid`` is switched on: every
        pixel of the region is computed (NaN where a window has no pair weight) and the result has one more key,
        ``covered``.  With ``general_grid`` switched on, everything else the walk takes is taken too -- ``pos_list``, unequal frame
        shapes, any masked model, a forced direct kernel, larger steps -- on a table filled by the explicit window x frame sum;
        where coverage is not trivial the result has ``covered`` as well.  ``widen``: as for ``match()``; not on a masked model
        nor on the general table."""
        return self._cost_volume(ROI=ROI, step=step, with_fit=with_fit, widen=widen)

    def basins(self, k=4, ROI=None, step=None, widen=0):
        """Per pixel, the ``k`` lowest local minima ("basins") of the cost over the search box (extension;
        ``include/umpa_grid.h`` has the definition): a shift is a basin iff its cost is below ``+Inf`` and none of its up
        to eight neighbours inside the box has a lower cost, or an equal one earlier in scan order (rows first, then
        columns).  Basins are ranked by cost, then scan order; rank 0 is the integer minimum of ``match(search='grid')``.
        Returns a dictionary of

          ``dx``, ``dy``, ``f``, ``T`` (``df``: dark-field model)  float64 ``[k, N0, N1]``: what ``match(search='grid')``
                    would return had rank ``r`` been the minimum -- the model's sub-pixel step on the 4x4 neighbourhood of
                    the basin (``dy``: row shift, ``dx``: column shift), ``T`` / ``df`` of the integer shift;
          ``cost``  float64 ``[k, N0, N1]``: the cost of the integer shift, ``cost_volume()``'s number;
          ``shift`` int32 ``[k, 2, N0, N1]``: the integer shift, row shift first;
          ``err``   int32 ``[k, N0, N1]``: 1 the fit succeeded, 0 the 4x4 neighbourhood leaves the search range (``dx``,
                    ``dy`` are the integer shift, ``f`` its cost), -1 the pixel has no basin of this rank (zeros);
          ``count`` int32 ``[N0, N1]``: the number of basins of the pixel, which may exceed ``k``.

        ``k``: 1 to 8.  ``ROI`` / ``step`` as for ``cost_volume()``; the model's own ROI is not changed; a stack uploaded by
        ``stage_sample`` is adopted as by ``cost_volume()``.  Models ``cost_volume()`` takes only; anything else raises
        ``RuntimeError``.  ``umpa_amd.basins`` has helpers that pick among the ranks.  ``widen``: as for ``match()``."""
        return self._basins(k=k, ROI=ROI, step=step, widen=widen)

    def track(self, prior_dx, prior_dy, lam=None, radius=None, ROI=None, step=None, widen=0):
        """Tracked search (extension; ``include/umpa_grid.h``: ``umpa_grid_track`` has the definition): per pixel, among ALL
        basins of the cost over the search box -- not only the eight ``basins()`` can keep -- the one a prior shift
        ``(prior_dy rows, prior_dx columns)`` selects, finished like ``match(search='grid')`` finishes its minimum.  One pass on
        the device, one set of maps back.

          ``lam=None``    the basin nearest the prior (then the cheaper one, then scan order): ``basins.nearest`` over all basins;
          ``lam=number``  the basin with the smallest ``cost + lam * d2``, ``d2`` the squared distance of its integer shift from
                          the prior; ``lam=0`` is ``match(search='grid')``;
          ``radius``      only basins with ``d2 <= radius ** 2`` are admissible (``None``: all).

        The priors are in the units of ``dx`` / ``dy`` of ``match()`` under either ``assign_coordinates``, so an earlier
        result's maps are priors as they stand (``umpa_amd.track.prior_from`` marks its failed pixels).  Scalars or
        ``[N0, N1]`` arrays of the region; numpy arrays, or float64 HIP tensors on the model's device -- then the maps come back
        as HIP tensors too.  A NaN prior leaves the pixel to the data term (the grid search's answer).

        Returns the dictionary of ``match()`` -- ``dx``, ``dy``, ``f``, ``T`` (``df``), ``err`` -- plus ``cost`` (of the chosen
        integer shift), ``cost0`` (the lowest basin cost of the pixel: ``cost > cost0`` says the prior overruled the data
        term), ``shift`` int32 ``[2, N0, N1]`` (row shift first), ``count`` (all basins) and ``found`` (the admissible ones).
        ``err`` is 1 where the sub-pixel fit succeeded and 0 otherwise, as ``match()`` has it; ``found == 0`` tells a pixel
        without an admissible basin (zeros) from one whose 4x4 neighbourhood leaves the search range.

        ``ROI`` / ``step``, the staged stack and the admitted models as for ``basins()``.  ``widen``: as for ``match()``; the
        priors then have the shape of the result (the kept region) or are scalars."""
        return self._track(prior_dx, prior_dy, lam=lam, radius=radius, ROI=ROI, step=step, widen=widen)

    def sequence(self, state=None, lam=None, trunc=None, ROI=None, step=None, out=None):
        """Sequence search (extension; ``include/umpa_grid.h``: ``umpa_grid_sequence`` has the definition): one forward step of
        a dynamic programme over a series of projections.  ``state`` holds, per pixel, an accumulated cost for every shift of
        the search box -- float64 ``[U, U, N0, N1]``, ``U = 2 max_shift - 1``, laid out like ``cost_volume()`` -- or is ``None``
        where a series starts.  This projection's cost of a shift is added to the cheapest predecessor, where moving from
        shift ``s'`` to ``s`` costs ``lam * |s - s'|^2`` (rows, then columns: the two-stage form of the header) and never more
        than ``trunc`` above the best predecessor (``None``: no truncation); the minimum of the state is taken off, so that
        the numbers stay on the scale of one projection's costs.  The shift with the lowest sum is finished like
        ``match(search='grid')`` finishes its minimum, on this projection's costs.

        Returns the dictionary of ``match()`` -- ``dx``, ``dy``, ``f``, ``T`` (``df``), ``err`` -- plus ``cost`` (this projection's
        cost of the chosen integer shift), ``total`` (its accumulated cost), ``cost0`` (the lowest cost of this projection
        alone), ``shift`` int32 ``[2, N0, N1]`` (row shift first), ``moved`` (int32: 1 where the series overruled this
        projection's own minimum) and ``state``, the state to hand to the next projection's call.  ``lam=0`` and
        ``state=None`` both give the maps of ``match(search='grid')``.

        ``state`` (and ``out``, an array the next state is written into instead of a new one) are numpy arrays, or float64
        HIP tensors on the model's device -- then everything comes back as HIP tensors.  ``ROI`` / ``step``, the staged stack
        and the admitted models as for ``track()``; ``max_shift`` 2 to 8.  ``umpa_amd.Sequence`` keeps the state of a step
        series on the device."""
        return self._sequence(state=state, lam=lam, trunc=trunc, ROI=ROI, step=step, out=out)

    def uncertainty(self, result, noise_var=None, ROI=None, step=None, sam=None, resident=False, shift=None):
        """The per-pixel uncertainty maps of ``result = self.match(...)`` (extension): ``umpa_amd.sigma.uncertainty``.
        ``resident=True``: on the model's own device frames -- masked models, staged stacks, no upload."""
        from . import sigma
        return sigma.uncertainty(self, result, noise_var=noise_var, ROI=ROI, step=step, sam=sam, resident=resident, shift=shift)


    _masked_grid = False

    @property
    def masked_grid(self):
        """The opt-in switch of the grid consumers for a model WITH masks (extension; ``include/umpa_grid.h``:
        ``umpa_grid_set_masked``), ``False`` by default.  While it is ``False``, ``match(search='grid')``, ``cost_volume``,
        ``basins``, ``track`` and ``sequence`` (and ``Tracker``, ``Sequence``, ``match_smooth``) refuse a masked model as they
        always did.  Set to ``True``, they run on the masked tiled path's table of finished costs: ``match(search='grid')``
        skips the pixels below the coverage threshold as ``match()`` does; the others compute every pixel and return one more
        key, ``covered`` -- a numpy bool ``[N0, N1]``, ``coverage >= threshold`` with ``match()``'s threshold -- for the caller
        to drop the rest.  ``widen > 0``, ``coarse_to_fine`` and ``scale_space`` stay refused: a finished cost is not linear in
        the windowed sums.  On a model without masks the switch stays ``False`` and changes nothing."""
        return bool(self._masked_grid)

    @masked_grid.setter
    def masked_grid(self, on):
        on = bool(on) and self._mask is not None
        if self._mask is not None:
            _lib.grid().check(_lib.grid().set_masked(self._handle, int(on)), "grid set_masked")
        self._masked_grid = on


class UMPAModelNoDF(_UMPAModelPlain):
    """Mirror of ``UMPAModelNoDF`` (``model.pyx:758-822``)."""
    Nparam = 4
    _kind = KIND_NODF


class UMPAModelDF(_UMPAModelPlain):
    """Mirror of ``UMPAModelDF`` (``model.pyx:824-896``)."""
    Nparam = 5
    _kind = KIND_DF

    @property
    def Im(self):
        """Mean ref frame amplitude: never set by the reference either (``Model.h:148``)."""
        return 0.0


class UMPAModelDFKernel(UMPAModelBase):
    """Mirror of ``UMPAModelDFKernel`` (``model.pyx:899-997``): the reference blurred on the fly by a
    per-pixel 17x17 Gaussian ``exp(-a i^2 - b ij - c j^2)``; ``abc`` is an input.  Runs on the general
    direct kernel (289 taps per window pixel, as heavy as in the reference)."""
    Nparam = 7
    safe_crop = 8
    _kind = KIND_DFKERNEL

    def min(self, i, j, a, b, c):
        values = np.zeros((self.Nparam,), dtype=NPDOUBLE)
        values[4], values[5], values[6] = a, b, c
        self._min(i, j, values)
        return values

    def cost(self, i, j, sx, sy, a, b, c):
        values = np.zeros(5)
        values[2], values[3], values[4] = a, b, c
        self._lib.check(self._lib.cost(self._handle, int(i), int(j), _cround(sx), _cround(sy),
                                       _lib._ptr(values, _lib._dp)), "cost")
        return (values[0], values[1])

    def match(self, step=None, abc=None, dxdy=None, ROI=None, num_threads=None, quiet=False, search='walk'):
        if search not in ('walk', 'grid'):
            raise ValueError("search must be 'walk' or 'grid', not %r" % (search,))
        if search == 'grid':
            self._grid_check("search='grid'")
        s0, s1 = self._convert_ROI_slice(ROI, step)
        self._set_ROI((s0, s1))
        N0, N1 = self._counts(s0, s1)
        sh = (N0, N1)
        if abc is None:
            raise RuntimeError('abc array has to be provided')
        elif abc.shape != sh + (3,):
            raise RuntimeError('Wrong array shape for abc: %s, should be %s' % (abc.shape, sh + (3,)))
        values = np.zeros(sh + (self.Nparam,), dtype=np.float64)
        values[:, :, -3:] = abc
        result = self._match(step=step, input_values=values, dxdy=dxdy, ROI=ROI,
                             num_threads=num_threads, quiet=quiet)
        return self._unpack(result, False)

    def uncertainty(self, result, noise_var=None, ROI=None, step=None, sam=None, resident=False, shift=None):
        raise RuntimeError("uncertainty: the kernel dark-field model is not supported")
