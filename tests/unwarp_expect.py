"""The expectation of the unwarp tests: include/umpa_unwarp.h's expressions restated in numpy, operation by operation in
the header's order, np.float64 throughout (every numpy operation rounds once; nothing here can fuse a multiply and an add).
Written from the header's text, not from the kernel.  Also the maps and stacks the CPU and GPU tests share."""
import numpy as np

H, W, K = 37, 71, 2                     # the GPU tests' frames: odd width, no multiple of a wave, more than one block


def _weights(t):
    """Keys' cubic, a = -0.5, Horner form: w[-1], w[0], w[1], w[2]"""
    two = np.float64(2.0)
    wm = ((-t + two) * t - np.float64(1.0)) * t / two
    w0 = ((np.float64(3.0) * t - np.float64(5.0)) * t * t + two) / two
    w1 = ((np.float64(-3.0) * t + np.float64(4.0)) * t + np.float64(1.0)) * t / two
    w2 = (t - np.float64(1.0)) * t * t / two
    return wm, w0, w1, w2


def reference(raw, d0, d1, interp, dark=None, flat=None):
    """raw [K, H, W] (or [H, W]) of uint16 / float32 / float64; d0, d1 [H, W] float32; dark, flat broadcastable float64 or None.
    Returns float64 of raw's shape."""
    raw = np.asarray(raw)
    single = raw.ndim == 2
    v = raw.astype(np.float64)                                        # exact for the three dtypes
    if single:
        v = v[None]
    h, w = v.shape[1:]
    d0 = np.asarray(d0, dtype=np.float32).astype(np.float64)
    d1 = np.asarray(d1, dtype=np.float32).astype(np.float64)
    y = np.arange(h, dtype=np.float64)[:, None] + d0
    x = np.arange(w, dtype=np.float64)[None, :] + d1
    i0, j0 = np.floor(y), np.floor(x)
    fy, fx = y - i0, x - j0

    def tap(a, b):
        ii = np.clip(i0 + a, 0, h - 1).astype(np.int64)
        jj = np.clip(j0 + b, 0, w - 1).astype(np.int64)
        return v[:, ii, jj]

    one = np.float64(1.0)
    if interp == "linear":
        u = (one - fy) * ((one - fx) * tap(0, 0) + fx * tap(0, 1)) + fy * ((one - fx) * tap(1, 0) + fx * tap(1, 1))
    elif interp == "cubic":
        wx, wy = _weights(fx), _weights(fy)
        u = None
        for a in range(4):
            r = wx[0] * tap(a - 1, -1)
            r = r + wx[1] * tap(a - 1, 0)
            r = r + wx[2] * tap(a - 1, 1)
            r = r + wx[3] * tap(a - 1, 2)
            u = wy[0] * r if a == 0 else u + wy[a] * r
    else:
        raise ValueError(interp)
    if dark is not None:
        u = u - np.asarray(dark, dtype=np.float64)
    if flat is not None:
        u = u / np.asarray(flat, dtype=np.float64)
    return u[0] if single else u


def footprint_valid_bruteforce(d0, d1, interp):
    """pixel by pixel, tap by tap: is every tap index inside the frame before clamping?"""
    h, w = d0.shape
    taps = (0, 1) if interp == "linear" else (-1, 0, 1, 2)
    out = np.zeros((h, w), dtype=bool)
    for i in range(h):
        for j in range(w):
            i0 = int(np.floor(np.float64(i) + np.float64(d0[i, j])))
            j0 = int(np.floor(np.float64(j) + np.float64(d1[i, j])))
            out[i, j] = all(0 <= i0 + a <= h - 1 for a in taps) and all(0 <= j0 + b <= w - 1 for b in taps)
    return out


# ----------------------------------------------------------------------------- maps

def radial_map(h, w, amplitude=3.0, seed=7):
    """A smooth radial (barrel-like) distortion about a seeded, off-centre point, at most `amplitude` pixels, plus a small
    seeded shear: generic fractional parts everywhere."""
    rng = np.random.default_rng(seed)
    ci, cj = (h - 1) / 2.0 + rng.uniform(-2, 2), (w - 1) / 2.0 + rng.uniform(-2, 2)
    ii, jj = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    ri, rj = (ii - ci) / (h / 2.0), (jj - cj) / (w / 2.0)
    r2 = ri * ri + rj * rj
    k = rng.uniform(0.6, 0.9)
    d0 = k * r2 * ri + 0.137 * rj + 0.0113
    d1 = k * r2 * rj - 0.211 * ri + 0.0271
    scale = amplitude / max(np.abs(d0).max(), np.abs(d1).max())
    return (d0 * scale).astype(np.float32), (d1 * scale).astype(np.float32)


def maps(h=H, w=W):
    """name -> (d0, d1): the five maps of the arithmetic test"""
    z = np.zeros((h, w), np.float32)
    r0, r1 = radial_map(h, w)
    # coordinates that land exactly on the last row and the last column: fy = fx = 0 at i0 = H - 1, j0 = W - 1 (and exact
    # integers elsewhere: every other pixel reads its mirror image)
    ii, jj = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    last0 = ((h - 1) - ii - ii).astype(np.float32)                     # source row H - 1 - i: row 0 reads the last row
    last1 = ((w - 1) - jj - jj).astype(np.float32)
    return {
        "identity": (z, z),
        "shift": (z + np.float32(2.0), z - np.float32(3.0)),
        "radial": (r0, r1),
        "radial_x4": (r0 * np.float32(4.0), r1 * np.float32(4.0)),
        "last_row_col": (last0, last1),
    }


def stack(dtype, h=H, w=W, k=K, seed=11, nan_at=None):
    """A speckle-like raw stack (counts around 20000) of the given dtype."""
    rng = np.random.default_rng(seed)
    a = 20000.0 * (1.0 + 0.3 * rng.standard_normal((k, h, w)))
    a = np.clip(a, 100.0, 60000.0)
    if np.dtype(dtype) == np.uint16:
        a = np.rint(a).astype(np.uint16)
    else:
        a = a.astype(dtype)
    if nan_at is not None:
        a[nan_at] = np.nan
    return np.ascontiguousarray(a)


def dark_flat(h=H, w=W, k=K, seed=13):
    rng = np.random.default_rng(seed)
    dark = 100.0 + rng.uniform(0, 2, size=(k, h, w))
    flat = 0.9 + 0.2 * rng.uniform(size=(k, h, w))
    return dark, flat
