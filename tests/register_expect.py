"""
The registration sums of include/umpa_register.h in extended precision, the host-side fit, and the error bounds the tests
compare with.  Nothing here is taken from what the code under test returns.

  sums(a, b, w, S, boundary)      P, Q, A over the box and, for every entry, the bound (n + 2) * 2^-53 * sum |terms| that
                                  holds for a float64 evaluation in ANY order, fused or not (n pixels summed; n - 1
                                  additions and at most two roundings inside a term, e.g. (w * a) * b)
  distance(...)                   D, alpha and dD = dA + 2 |P| / (Q + eps) dP + P^2 / (Q + eps)^2 dQ
  expect(a, b, w, S, boundary)    all of it plus the integer minimum, the sub-pixel shift and its tolerance
                                  tol = 4 * max(dD over the 3 x 3) / lambda_min  (lambda_min: smallest eigenvalue of the
                                  fitted Hessian; the factor 4 covers the second-order terms)
  fft_bound(a, b, w)              how far the reference's three-FFT evaluation of D may be from the exact one

Extended precision is np.longdouble where its eps is below 2^-60 (x87: 2^-63), else mpmath at 100 bits.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "J_register.npz")
U = 2.0 ** -53
EPSILON = 1e-10
INTERIOR, BORDER, NO_FINITE = 0, 1, 2

# ----------------------------------------------------------------------------- fixtures
# (shape, seed, shift d of b against a): b = 0.85 * a(. - d) + noise, a Fourier-shifted copy
PAIRS = [((70, 83), 5, (2.37, -3.58)), ((64, 64), 6, (-4.21, 1.64)), ((37, 130), 7, (0.45, 5.72))]


def fourier_shift(a, d):
    """a(. - d), periodic"""
    f0 = np.fft.fftfreq(a.shape[0])[:, None]
    f1 = np.fft.fftfreq(a.shape[1])[None, :]
    return np.real(np.fft.ifft2(np.fft.fft2(a) * np.exp(-2j * np.pi * (f0 * d[0] + f1 * d[1]))))


def make_pair(shape, seed, d):
    """the generator's construction (tests read the arrays from the fixture file)"""
    from umpa_amd.synth import make_stack
    a = np.ascontiguousarray(make_stack(shape[0], shape[1], 1, 4, seed=seed)[1][0])
    rng = np.random.default_rng(seed)
    b = 0.85 * fourier_shift(a, d) + 0.01 * rng.standard_normal(shape)
    return a, np.ascontiguousarray(b)


def weights(shape, seed, zero_fraction=0.02):
    """a weight plane with a zero block and 2 % random zeros; uniform random numbers only (bit-reproducible everywhere)"""
    rng = np.random.default_rng(1000 + seed)
    w = 0.25 + rng.random(shape)
    w[rng.random(shape) < zero_fraction] = 0.0
    w[shape[0] // 3:shape[0] // 3 + 9, shape[1] // 4:shape[1] // 4 + 11] = 0.0
    return w


def make_diffuser_stack():
    from umpa_amd.synth import make_stack
    a = make_stack(48, 52, 1, 4, seed=11)[1][0]
    rng = np.random.default_rng(11)
    ds = [(0.0, 0.0), (1.37, -2.21), (-3.61, 0.83), (2.58, 4.42)]
    return np.stack([a] + [(1.0 - 0.03 * k) * fourier_shift(a, d) + 0.01 * rng.standard_normal(a.shape) for k, d in enumerate(ds) if k])


def make_transmission_maps():
    """2 x 2 overlapping crops (60 x 72) of one smooth-plus-texture image at known offsets with sub-pixel errors"""
    from scipy.ndimage import gaussian_filter, map_coordinates
    rng = np.random.default_rng(21)
    Hb, Wb = 96, 112
    yy, xx = np.meshgrid(np.arange(Hb, dtype=np.float64), np.arange(Wb, dtype=np.float64), indexing="ij")
    smooth = 0.8 - 0.25 * np.exp(-((yy - 45.0) ** 2 + (xx - 52.0) ** 2) / 600.0)
    tex = gaussian_filter(rng.standard_normal((Hb, Wb)), 2.0)
    img = smooth + 0.08 * tex / tex.std()
    pos = np.array([[0.0, 0.0], [0.0, 12.0], [10.0, 0.0], [10.0, 12.0]])
    err = np.array([[0.0, 0.0], [0.63, -1.27], [-1.42, 0.81], [1.18, 1.56]])
    h, w = 60, 72
    T = []
    for p, e in zip(pos, err):
        cy, cx = np.meshgrid(np.arange(h) + 10.0 + p[0] + e[0], np.arange(w) + 12.0 + p[1] + e[1], indexing="ij")
        T.append(map_coordinates(img, [cy, cx], order=3, mode="nearest") + 0.002 * rng.standard_normal((h, w)))
    return np.array(T), pos, err


_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN))
    return _golden


def pair(n):
    g = golden()
    return g["p%d_a" % n], g["p%d_b" % n], weights(PAIRS[n][0], PAIRS[n][1])


def as_dtype(x, dtype):
    """the frame in one of the three dtypes of the library (uint16: scaled so that the speckle uses the range)"""
    if dtype == np.uint16:
        return np.ascontiguousarray(np.clip(np.rint(x * 20000.0), 0, 65535).astype(np.uint16))
    return np.ascontiguousarray(x.astype(dtype))


def synthetic(shape, shifts, seed):
    """a (H x W) and one b per shift: periodic, bilinearly shifted, scaled, noisy copies (made on the spot)"""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(seed)
    g = gaussian_filter(rng.standard_normal(shape), 1.5, mode="wrap")
    a = 1.0 + 0.3 * g / g.std()
    bs = []
    for k, d in enumerate(shifts):
        f = np.floor(d).astype(int)
        t = np.asarray(d) - f
        b = np.zeros(shape)
        for c0, w0 in ((0, 1 - t[0]), (1, t[0])):
            for c1, w1 in ((0, 1 - t[1]), (1, t[1])):
                b += w0 * w1 * np.roll(a, (f[0] + c0, f[1] + c1), axis=(0, 1))
        bs.append((0.9 - 0.05 * k) * b + 0.01 * rng.standard_normal(shape))
    return a, np.array(bs)


# ----------------------------------------------------------------------------- extended precision

def extended_over_double():
    """unit roundoff of the extended arithmetic over that of float64: what a bound d* of sums() shrinks by when it is to
    bound the helper's own error instead of a float64 evaluation's"""
    eps = float(np.finfo(np.longdouble).eps)
    return (eps if eps < 2.0 ** -60 else 2.0 ** -99) / 2.0 ** -52


def _extended():
    if np.finfo(np.longdouble).eps < 2.0 ** -60:
        return np.longdouble, np.abs
    import mpmath
    mpmath.mp.prec = 100
    to = np.frompyfunc(lambda v: mpmath.mpf(float(v)), 1, 1)
    return (lambda x: to(np.asarray(x, dtype=np.float64))), np.frompyfunc(abs, 1, 1)


def sums(a, b, w, S, boundary):
    """(P, Q, A, dP, dQ, dA) as float64 [U0, U1]; a, b, w: 2-D"""
    cast, absf = _extended()
    S0, S1 = S
    H, W = a.shape
    a, b = cast(a), cast(b)
    w = cast(np.ones((H, W))) if w is None else cast(w)
    wa, waa = w * a, w * a * a
    out = np.zeros((6, 2 * S0 + 1, 2 * S1 + 1))
    for ri in range(-S0, S0 + 1):
        for rj in range(-S1, S1 + 1):
            if boundary == "wrap":
                br = np.roll(b, (ri, rj), axis=(0, 1))                 # br[x] = b[x - r]
                terms = (wa * br, w * br * br, waa)
            else:
                ys = slice(max(0, ri), min(H, H + ri))
                xs = slice(max(0, rj), min(W, W + rj))
                br = b[max(0, -ri):min(H, H - ri), max(0, -rj):min(W, W - rj)]
                terms = (wa[ys, xs] * br, w[ys, xs] * br * br, waa[ys, xs])
            n = terms[0].size
            for k, t in enumerate(terms):
                out[k, ri + S0, rj + S1] = float(t.sum())
                out[3 + k, ri + S0, rj + S1] = (n + 2) * U * float(absf(t).sum())
    return tuple(out)


def distance(P, Q, A, eps, dP=0.0, dQ=0.0, dA=0.0):
    with np.errstate(divide="ignore", invalid="ignore"):
        D = A - P * P / (Q + eps)
        alpha = P / (Q + eps)
        dD = dA + 2 * np.abs(P) / (Q + eps) * dP + P * P / (Q + eps) ** 2 * dQ
    return D, alpha, dD


# ----------------------------------------------------------------------------- the host-side fit

def fit(z):
    """Least-squares paraboloid through z[u + 1, v + 1] (a 6-column design matrix, solved by lstsq): (offset, value, kind,
    lambda_min); falls back to the two 1-D parabolas where the paraboloid is no minimum."""
    u, v = np.meshgrid([-1.0, 0.0, 1.0], [-1.0, 0.0, 1.0], indexing="ij")
    M = np.stack([np.ones(9), u.ravel(), v.ravel(), u.ravel() ** 2, v.ravel() ** 2, (u * v).ravel()], axis=1)
    c = np.linalg.lstsq(M, np.asarray(z, dtype=np.float64).ravel(), rcond=None)[0]
    h = np.array([[c[3], 0.5 * c[5]], [0.5 * c[5], c[4]]])
    lam = np.linalg.eigvalsh(h)[0]
    if c[3] > 0 and c[4] > 0 and np.linalg.det(h) > 0:
        x = -np.linalg.solve(2 * h, c[1:3])
        return x, c[0] + 0.5 * (c[1] * x[0] + c[2] * x[1]), "2d", lam
    off, val = [], []
    for line in (z[:, 1], z[1, :]):
        p = np.polyfit([-1.0, 0.0, 1.0], line, 2)
        if p[0] > 0:
            off.append(-0.5 * p[1] / p[0]); val.append(p[2] - 0.25 * p[1] ** 2 / p[0])
        else:
            off.append(0.0); val.append(line[1])
    return np.array(off), max(val), "1d", lam


def locate(D, alpha, dD=None):
    """(shift, alpha, mindist, status, imin, tol) of one box"""
    S0, S1 = D.shape[0] // 2, D.shape[1] // 2
    fin = np.isfinite(D)
    if not fin.any():
        return np.array([np.nan, np.nan]), np.nan, np.nan, NO_FINITE, None, np.nan
    i, j = np.unravel_index(np.argmin(np.where(fin, D, np.inf)), D.shape)
    r = np.array([i - S0, j - S1], dtype=np.float64)
    if i in (0, D.shape[0] - 1) or j in (0, D.shape[1] - 1) or not fin[i - 1:i + 2, j - 1:j + 2].all():
        return r, alpha[i, j], D[i, j], BORDER, (i, j), 0.0
    off, val, kind, lam = fit(D[i - 1:i + 2, j - 1:j + 2])
    tol = np.inf if dD is None or not lam > 0 else 4.0 * dD[i - 1:i + 2, j - 1:j + 2].max() / lam
    return r + off, alpha[i, j], val, INTERIOR, (i, j), tol


_cache = {}


def expect(a, b, w, S, boundary, key=None):
    """dict of everything for one pair; cached under `key` (inputs must then not change)"""
    if key is not None and key in _cache:
        return _cache[key]
    P, Q, A, dP, dQ, dA = sums(a, b, w, S, boundary)
    eps = EPSILON if (w is not None or boundary == "overlap") else 0.0
    D, alpha, dD = distance(P, Q, A, eps, dP, dQ, dA)
    shift, al, mind, status, imin, tol = locate(D, alpha, dD)
    e = dict(P=P, Q=Q, A=A, dP=dP, dQ=dQ, dA=dA, D=D, alpha=alpha, dD=dD, shift=shift, alpha_min=al, mindist=mind,
             status=status, imin=imin, tol=tol)
    if key is not None:
        _cache[key] = e
    return e


def wrap_centred(x, size):
    """x modulo size per axis, into [-size / 2, size / 2)"""
    x, size = np.asarray(x, dtype=np.float64), np.asarray(size, dtype=np.float64)
    return x - size * np.floor(x / size + 0.5)


def get_diff_pos(refs, S=(8, 8)):
    return np.round(np.array([wrap_centred(-expect(refs[0], r, None, S, "wrap")["shift"], refs.shape[1:]) for r in refs]), 2)


# ----------------------------------------------------------------------------- the reference's FFT evaluation

def fft_bound(a, b, w=None):
    """Bound on |D_fft - D_exact| per shift for D evaluated as the reference does, with three transforms of length
    N = H * W, as (dP, dQ, dA) to be propagated through D = A - P^2 / (Q + eps) like the sums' bounds.
    With g = eta log2(N), eta = mu + gamma_4 (sqrt(2) + mu) ~ 6.7 u (Higham, Accuracy and Stability of Numerical
    Algorithms, section 24.1), for the correlation c = ifft(fft(x) conj(fft(y))):
      * a forward transform is normwise backward stable, fl(F x) = F (x + dx) with |dx|_2 <= g |x|_2, so the two of them
        perturb the inputs: |corr(dx, y)[r]| <= |dx|_2 |y|_2 <= g |x|_2 |y|_2 each (Cauchy-Schwarz);
      * the complex product perturbs every Fourier coefficient by a relative 4 u: |ifft(c^ e)[r]| <= 4 u |x|_2 |y|_2 (Parseval);
      * every output of the inverse transform is a sum of the N coefficients c^_k, each multiplied by at most log2(N)
        rounded twiddle factors and passed through log2(N) rounded additions: |dc[r]| <= g |c^|_1 / N, componentwise.
        (The normwise bound g |c|_2 would cost a factor sqrt(N) per shift: the spectrum is dominated by its mean term.)
    So |dc[r]| <= (2 g + 4 u) |x|_2 |y|_2 + g |c^|_1 / N, with the spectrum's 1-norm computed here.
    A, and Q in the unweighted case, are plain sums of N positive terms, bounded by h u |.| with h the longest chain of
    additions: the unweighted norms are dot products (numpy.vdot) in an order that is the library's, h = N (any order);
    the weighted first term is numpy.sum, pairwise in blocks of at most
    128 terms, h = 128 + log2(N).
    Observed against the fixtures: 0.5 - 1.2e-14 of max |cc|; this bound comes out at about 1e-12 of max |cc|.  Above
    1e-11 it would be a mistake here (the test asserts that)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    N = a.size
    g = 6.7 * U * np.log2(N)
    n2 = lambda x: float(np.sqrt((x * x).sum()))

    def corr(x, y):
        spectrum1 = float(np.abs(np.fft.fft2(x) * np.conj(np.fft.fft2(y))).sum())
        return (2 * g + 4 * U) * n2(x) * n2(y) + g * spectrum1 / N

    h = N
    if w is None:
        return corr(a, b), h * U * n2(b) ** 2, h * U * n2(a) ** 2
    return corr(w * a, b), corr(w, b * b), (128 + np.log2(N)) * U * float((w * a * a).sum())
