"""
tests/ddf_expect.py -- TEST INFRASTRUCTURE: a numpy restatement of include/umpa_ddf.h and of umpa_amd/ddf.py's search.

The kernel, the blur in np.longdouble with its rounding bound, the fold, the width / angle conversion and the search loop
over the CPU checker's plain model (oracle.cpu_model.port.UMPAModelNoDF).  Nothing here imports umpa_amd.ddf.
"""
import functools
import os

import numpy as np

TAPS, HALF = 17, 8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "K_ddf.npz")

# the kernels of the identity check and of the blur tests
KERNELS = [(0.1, 0.0, 0.1), (0.5, 0.2, 0.3), (2.0, -0.5, 0.08), (0.03, 0.0, 0.03)]
BLUR_KERNELS = [(0.1, 0.0, 0.1), (0.5, 0.2, 0.3), (2.0, -0.5, 0.08), (50.0, 0.0, 50.0), (0.005, 0.0, 0.005)]


def admissible(a, b, c):
    return bool(np.isfinite([a, b, c]).all() and a > 0 and c > 0 and 4 * a * c - b * b > 0)


def kernel(a, b, c):
    """g[k, l] = exp(-a (k-8)^2 - b (k-8)(l-8) - c (l-8)^2) / S, S summed with l fastest (Model.cpp:88-117)."""
    e = np.empty((TAPS, TAPS))
    norm = 0.0
    for k in range(TAPS):
        for l in range(TAPS):
            i, j = float(k - HALF), float(l - HALF)
            e[k, l] = np.exp(-a * i * i - b * i * j - c * j * j)
            norm += e[k, l]
    return e / norm


def blur_exact(frame, g):
    """(out, bound): the blur of one [H, W] frame in np.longdouble (border: the input) and the header's bound
    291 * 2^-53 * sum g |in| (0 on the border)."""
    frame = np.asarray(frame, dtype=np.float64)
    H, W = frame.shape
    assert H >= TAPS and W >= TAPS
    x = frame.astype(np.longdouble)
    ax = np.abs(x)
    acc = np.zeros((H - 2 * HALF, W - 2 * HALF), dtype=np.longdouble)
    mag = np.zeros_like(acc)
    for k in range(TAPS):
        for l in range(TAPS):
            gv = np.longdouble(g[k, l])
            acc += gv * x[k:k + H - 2 * HALF, l:l + W - 2 * HALF]
            mag += np.abs(gv) * ax[k:k + H - 2 * HALF, l:l + W - 2 * HALF]
    out = x.copy()
    out[HALF:H - HALF, HALF:W - HALF] = acc
    bound = np.zeros((H, W), dtype=np.longdouble)
    bound[HALF:H - HALF, HALF:W - HALF] = np.longdouble(291.0) * np.longdouble(2.0) ** -53 * mag
    return out, bound


def blur(frames, abc):
    """[K, H, W] float64: the longdouble blur rounded to double."""
    g = kernel(*abc)
    return np.stack([blur_exact(f, g)[0].astype(np.float64) for f in frames])


def fold(planes):
    """planes: one dict per candidate with f, T, dx, dy (float64) and err (int32) -> dict index, f, T, dx, dy, err."""
    first = planes[0]
    best = {k: np.array(first[k], dtype=np.float64) for k in ("f", "T", "dx", "dy")}
    index = np.where(first["err"] == 1, 0, -1).astype(np.int32)
    for m in range(1, len(planes)):
        p = planes[m]
        with np.errstate(invalid="ignore"):
            take = (p["err"] == 1) & ((index < 0) | (p["f"] < best["f"]))
        for k in best:
            best[k][take] = p[k][take]
        index[take] = m
    best["index"] = index
    best["err"] = (index >= 0).astype(np.int32)
    return best


def fold_brute(planes):
    """The same, pixel by pixel: walk the candidates in order, a valid one replaces the holder iff there is none yet or its
    cost is strictly below the holder's (so a holder with a NaN cost is never replaced, a NaN never replaces)."""
    sh = planes[0]["err"].shape
    out = {k: np.empty(sh) for k in ("f", "T", "dx", "dy")}
    out["index"] = np.empty(sh, dtype=np.int32)
    for p in np.ndindex(*sh):
        idx = -1
        for m, pl in enumerate(planes):
            if pl["err"][p] == 1 and (idx < 0 or pl["f"][p] < planes[idx]["f"][p]):
                idx = m
        src = planes[idx if idx >= 0 else 0]
        for k in ("f", "T", "dx", "dy"):
            out[k][p] = src[k][p]
        out["index"][p] = idx
    out["err"] = (out["index"] >= 0).astype(np.int32)
    return out


def hand_made_planes(seed=11, M=6, shape=(7, 9)):
    """Candidate planes with equal costs, NaN costs and failed pixels in every position of the order."""
    rng = np.random.default_rng(seed)
    planes = []
    for m in range(M):
        f = rng.integers(0, 4, size=shape).astype(np.float64)         # few distinct values: many ties
        f[rng.random(shape) < 0.15] = np.nan
        planes.append(dict(f=f, T=rng.random(shape) + m, dx=rng.random(shape) - m, dy=rng.random(shape) * m,
                           err=(rng.random(shape) < 0.7).astype(np.int32)))
    planes[0]["err"][0, :] = 0                                        # the first candidate fails on a row ...
    for p in planes:
        p["err"][1, :3] = 0                                           # ... and all of them on a patch
    planes[0]["f"][2, 0], planes[0]["err"][2, 0] = np.nan, 1          # a NaN holder is never replaced
    return planes


def kernel_from_sigma(s_major, s_minor, theta):
    """A = R diag(1 / s_major^2, 1 / s_minor^2) R', R's first column (cos theta, sin theta) in (row, column); a = A00 / 2,
    b = A01, c = A11 / 2."""
    R = np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])
    A = R @ np.diag([1.0 / s_major ** 2, 1.0 / s_minor ** 2]) @ R.T
    return A[0, 0] / 2, A[0, 1], A[1, 1] / 2


def sigma_from_kernel(a, b, c):
    """By numpy's eigen-decomposition of the covariance, one pixel: (s_major, s_minor, theta in [0, pi))."""
    cov = np.linalg.inv(np.array([[2.0 * a, b], [b, 2.0 * c]]))
    w, v = np.linalg.eigh(cov)                                        # ascending
    major = v[:, 1]
    theta = np.arctan2(major[1], major[0]) % np.pi
    if abs(w[1] - w[0]) <= 1e-14 * w[1]:
        theta = 0.0
    return np.sqrt(w[1]), np.sqrt(w[0]), theta


def shifted(roi):
    """the plain model's region of the kernel model's region"""
    (a0, b0, c0), (a1, b1, c1) = roi
    return ((a0 + HALF, b0 + HALF, c0), (a1 + HALF, b1 + HALF, c1))


def full_roi(shape, Nw, max_shift):
    pad = Nw + max_shift + HALF
    return ((0, shape[0] - 2 * pad, 1), (0, shape[1] - 2 * pad, 1))


def nodf_on_blurred(ns, sam, ref, abc, Nw, max_shift, roi=None, assign="sam", subpx=-1, debug=True):
    """The right-hand side of the identity: the plain model of namespace `ns` on the blurred reference, over the kernel
    model's region `roi` shifted by 8."""
    if roi is None:
        roi = full_roi(sam[0].shape, Nw, max_shift)
    m = ns.UMPAModelNoDF(list(sam), list(blur(ref, abc)), window_size=Nw, max_shift=max_shift)
    m.debug = debug
    m.assign_coordinates = assign
    m.sub_pixel_mode = subpx
    return m.match(ROI=shifted(roi), quiet=True)


def dfkernel_uniform(ns, sam, ref, abc, Nw, max_shift, roi=None, assign="sam", subpx=-1, debug=True):
    """The left-hand side: the kernel model of `ns` with the same (a, b, c) at every pixel."""
    if roi is None:
        roi = full_roi(sam[0].shape, Nw, max_shift)
    m = ns.UMPAModelDFKernel(list(sam), list(ref), window_size=Nw, max_shift=max_shift)
    m.debug = debug
    m.assign_coordinates = assign
    m.sub_pixel_mode = subpx
    n0, n1 = len(range(*roi[0])), len(range(*roi[1]))
    abc_map = np.empty((n0, n1, 3))
    abc_map[...] = abc
    return m.match(abc=abc_map, ROI=roi, quiet=True)


def search(sam, ref, candidates, Nw, max_shift, roi=None, assign="sam", subpx=-1, debug=True):
    """The search loop over oracle.cpu_model.port.UMPAModelNoDF: (fold result, per-candidate results)."""
    from oracle import cpu_model
    per = [nodf_on_blurred(cpu_model.port, sam, ref, tuple(c), Nw, max_shift, roi, assign, subpx, debug) for c in candidates]
    return fold(per), per


# ----------------------------------------------------------------------------- the identity's stack, the golden file

IDENTITY = dict(H=64, W=72, K=3, Nw=2, max_shift=4, seed=5, amplitude=2.0)
STEPPED = ((3, 33, 3), (2, 40, 2))
# what tests/golden/make_golden_ddf.py records: (kernel, assign_coordinates, sub_pixel_mode, ROI or None)
GOLDEN_VARIANTS = [(KERNELS[0], "sam", -1, None), (KERNELS[1], "ref", -1, STEPPED), (KERNELS[2], "sam", 1, None)]


@functools.lru_cache(maxsize=None)
def identity_stack():
    from umpa_amd import synth
    p = IDENTITY
    sam, ref, _ = synth.make_stack(p["H"], p["W"], p["K"], p["max_shift"], seed=p["seed"], amplitude=p["amplitude"])
    sam.setflags(write=False)
    ref.setflags(write=False)
    return sam, ref


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def golden_maps(n):
    g = golden()
    pre = "v%d_" % n
    return {k[len(pre):]: g[k] for k in g if k.startswith(pre)}


# ----------------------------------------------------------------------------- the recovery case

RECOVERY = dict(H=80, W=96, K=4, Nw=2, max_shift=4)
RECOVERY_SIGMAS = [(0.6, 0.6, 0.0), (2.0, 0.6, 0.0), (2.0, 0.6, np.pi / 4), (2.0, 0.6, np.pi / 2), (2.0, 0.6, 3 * np.pi / 4),
                   (1.5, 1.5, 0.0)]
RECOVERY_TRUE = (2, 4)                                                # left half, right half


@functools.lru_cache(maxsize=None)
def recovery_case():
    """(sam, ref, candidates): references 1 + 0.3 g / std(g), g = Gaussian-filtered noise (sigma 1.2); the sample is 0.8
    times the reference blurred with candidate 2 on the left half and candidate 4 on the right half, moved so that dy = 1
    and dx = -1 (sam[i, j] = ref[i + dy, j + dx]), plus N(0, 0.004)."""
    from scipy.ndimage import gaussian_filter
    p = RECOVERY
    rng = np.random.default_rng(7)
    ref = np.empty((p["K"], p["H"], p["W"]))
    for k in range(p["K"]):
        g = gaussian_filter(rng.standard_normal((p["H"], p["W"])), 1.2)
        ref[k] = 1.0 + 0.3 * g / g.std()
    cand = np.array([kernel_from_sigma(*s) for s in RECOVERY_SIGMAS])
    left, right = blur(ref, tuple(cand[RECOVERY_TRUE[0]])), blur(ref, tuple(cand[RECOVERY_TRUE[1]]))
    mixed = np.where(np.arange(p["W"])[None, None, :] < p["W"] // 2, np.roll(left, (-1, 1), axis=(1, 2)), np.roll(right, (-1, 1), axis=(1, 2)))
    sam = 0.8 * mixed + 0.004 * rng.standard_normal(ref.shape)
    for x in (sam, ref, cand):
        x.setflags(write=False)
    return sam, ref, cand


def recovery_truth():
    """The true candidate of every pixel of the kernel model's extent, and the mask of the pixels more than Nw + 2 columns
    from the seam."""
    p = RECOVERY
    pad = p["Nw"] + p["max_shift"] + HALF
    cols = pad + np.arange(p["W"] - 2 * pad)
    rows = p["H"] - 2 * pad
    truth = np.where(cols < p["W"] // 2, RECOVERY_TRUE[0], RECOVERY_TRUE[1])
    seam = p["W"] // 2 - 0.5
    far = np.abs(cols - seam) > p["Nw"] + 2
    return np.broadcast_to(truth, (rows, cols.size)), np.broadcast_to(far, (rows, cols.size))


@functools.lru_cache(maxsize=None)
def recovery_search():
    sam, ref, cand = recovery_case()
    return search(sam, ref, cand, RECOVERY["Nw"], RECOVERY["max_shift"])
