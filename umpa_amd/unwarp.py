"""
Detector distortion correction ("unwarp"): ``libumpa_unwarp.so`` (``include/umpa_unwarp.h``, where the operation is
defined expression by expression).

The reference's batch script resamples every raw frame through a calibrated distortion map before it flat-corrects and
matches it (``UMPA/umpa_multi.py:127-130``: "Do unwarp: slowest step by far!").  An ``UnwarpMap`` holds such a map in
GPU memory and applies it

  * stand-alone, ``map.apply(stack, dark, flat)``: what a user runs once on references, flats and the dark frame, which
    are expected in unwarped geometry;
  * fused into the upload of every projection: ``model.set_unwarp(map)``, ``StreamingMatcher(..., unwarp=map)``,
    ``ProjectionFarm(..., unwarp=map)``.

HIP only: there is no CPU fallback (``valid`` is the one thing computed on the host: it reads the map, not a frame).
"""
import ctypes as C

import numpy as np

from . import _lib

__all__ = ["UnwarpMap"]

INTERP = {"linear": 0, "cubic": 1}
_RAW_CODE = {np.dtype(np.float64): 0, np.dtype(np.float32): 1, np.dtype(np.uint16): 2}


class UnwarpMap:
    """A backward map of an ``H x W`` detector: output pixel ``(i, j)`` reads the raw frame at ``(i + d0[i, j],
    j + d1[i, j])``, interpolated (``interp='cubic'``: Catmull-Rom, the default; ``'linear'``: bilinear), taps clamped to
    the frame's edge.  ``d0`` / ``d1`` are stored as float32."""

    def __init__(self, d0, d1, interp="cubic", device=0):
        self._handle = None
        if interp not in INTERP:
            raise ValueError("interp must be 'cubic' or 'linear', not %r" % (interp,))
        d0 = np.ascontiguousarray(d0, dtype=np.float32)
        d1 = np.ascontiguousarray(d1, dtype=np.float32)
        if d0.ndim != 2 or d0.shape != d1.shape:
            raise ValueError("d0 and d1 must be 2-D arrays of one shape, not %r and %r" % (d0.shape, d1.shape))
        self._d0, self._d1 = d0, d1
        self._interp = interp
        self._device = int(device)
        self._valid = None
        self._lib = _lib.unwarp()
        fp = C.POINTER(C.c_float)
        h = self._lib.map_create(d0.shape[0], d0.shape[1], d0.ctypes.data_as(fp), d1.ctypes.data_as(fp), INTERP[interp], self._device)
        if not h:
            raise RuntimeError("could not create the unwarp map: %s" % self._lib.error())
        self._handle = h

    def destroy(self):
        """Give the map's handle up now (models it is attached to keep unwarping until they detach or die)."""
        h, self._handle = getattr(self, "_handle", None), None
        if h:
            self._lib.map_destroy(h)

    __del__ = destroy

    @classmethod
    def from_coordinates(cls, src0, src1, interp="cubic", device=0):
        """``src0`` / ``src1``: the absolute source row / column of every output pixel.  The pixel grid is subtracted in
        float64, the displacement then rounded to float32."""
        d0, d1 = cls.displacements(src0, src1)
        return cls(d0, d1, interp=interp, device=device)

    @staticmethod
    def displacements(src0, src1):
        src0, src1 = np.asarray(src0, dtype=np.float64), np.asarray(src1, dtype=np.float64)
        if src0.ndim != 2 or src0.shape != src1.shape:
            raise ValueError("src0 and src1 must be 2-D arrays of one shape, not %r and %r" % (src0.shape, src1.shape))
        H, W = src0.shape
        d0 = src0 - np.arange(H, dtype=np.float64)[:, None]
        d1 = src1 - np.arange(W, dtype=np.float64)[None, :]
        return d0.astype(np.float32), d1.astype(np.float32)

    @classmethod
    def identity(cls, shape, interp="cubic", device=0):
        H, W = (int(s) for s in shape)
        return cls(np.zeros((H, W), np.float32), np.zeros((H, W), np.float32), interp=interp, device=device)

    @property
    def shape(self):
        return self._d0.shape

    @property
    def interp(self):
        return self._interp

    @property
    def device(self):
        return self._device

    @property
    def planes(self):
        """``(d0, d1)``, float32"""
        return self._d0, self._d1

    @property
    def valid(self):
        """bool ``[H, W]``: every tap of the pixel's footprint lies inside the frame, nothing was clamped."""
        if self._valid is None:
            self._valid = footprint_valid(self._d0, self._d1, self._interp)
        return self._valid

    def apply(self, stack, dark=None, flat=None):
        """``stack``: ``[K, H, W]`` (or ``[H, W]``) float64 / float32 / uint16 host frames; ``dark`` / ``flat``: float64,
        broadcast to the stack.  Returns the unwarped, then ``(u - dark) / flat`` corrected frames as float64 ``[K, H, W]``."""
        if self._handle is None:
            raise RuntimeError("the unwarp map was destroyed")
        stack = np.asarray(stack)
        if stack.ndim == 2:
            stack = stack[None]
        if stack.ndim != 3 or stack.shape[1:] != self.shape:
            raise ValueError("a stack of %r frames for a map of %r" % (stack.shape, self.shape))
        code = _RAW_CODE.get(stack.dtype)
        if code is None:
            raise RuntimeError("raw frames must be float64, float32 or uint16.")
        stack = np.ascontiguousarray(stack)
        K = stack.shape[0]

        def table(a):
            if a is None:
                return None, None
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), stack.shape))
            return a, _lib.FrameSet(list(a))

        dk, dkt = table(dark)
        fl, flt = table(flat)
        out = np.empty(stack.shape, dtype=np.float64)
        rawt, outt = _lib.FrameSet(list(stack)), _lib.FrameSet(list(out))
        self._lib.check(self._lib.frames(self._handle, rawt.table, code, K, dkt.table if dkt else None,
                                         flt.table if flt else None, outt.table, 0, None), "unwarp frames")
        return out

    def apply_device(self, raw, out, dark=None, flat=None, stream=None):
        """Device arrays (lists of 2-D HIP tensors on the map's device; ``raw``: float64 / float32 / uint16, the others
        float64): enqueues one kernel per frame on ``stream`` (a HIP stream handle; None: the null stream)."""
        import torch
        code = {torch.float64: 0, torch.float32: 1, getattr(torch, "uint16", None): 2}.get(raw[0].dtype)
        if code is None:
            raise RuntimeError("raw frames must be float64, float32 or uint16.")
        for group in (raw, out, dark, flat):
            if group is not None and (len(group) != len(raw) or any(tuple(t.shape) != self.shape or not t.is_contiguous() for t in group)):
                raise ValueError("every frame must be a contiguous %r tensor, one per raw frame" % (self.shape,))
        tabs = [_lib.FrameSet(list(g)) if g is not None else None for g in (raw, dark, flat, out)]
        self._lib.check(self._lib.frames(self._handle, tabs[0].table, code, len(raw), tabs[1].table if tabs[1] else None,
                                         tabs[2].table if tabs[2] else None, tabs[3].table, _lib.F_DEVICE_IO, stream), "unwarp frames")


def footprint_valid(d0, d1, interp):
    """Where the footprint of ``include/umpa_unwarp.h`` (rows ``i0 .. i0 + 1`` / ``i0 - 1 .. i0 + 2`` of ``i0 =
    floor(i + d0)``, columns alike) stays inside the frame."""
    H, W = d0.shape
    lo, hi = (0, 1) if interp == "linear" else (-1, 2)
    i0 = np.floor(np.arange(H, dtype=np.float64)[:, None] + d0.astype(np.float64))
    j0 = np.floor(np.arange(W, dtype=np.float64)[None, :] + d1.astype(np.float64))
    return (i0 + lo >= 0) & (i0 + hi <= H - 1) & (j0 + lo >= 0) & (j0 + hi <= W - 1)
