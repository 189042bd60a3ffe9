"""
The expectation of the integration tests: include/umpa_integrate.h restated in numpy, expression by expression and in the
header's evaluation order, so that every stage of the V-cycle (which contains no reduction) has the bit pattern the
library must produce; the whole preconditioned CG with extended-precision dots; a dense reference solve; the cases.

numpy only (scipy.ndimage.label for the components of the dense reference).
"""
import numpy as np

OMEGA = 0.8
NU = 2
COARSE_SWEEPS = 30
COARSEST = 4
CONVERGED, MAXITER, BREAKDOWN = 0, 1, 2

SHAPES = [(33, 47), (64, 64), (37, 130), (17, 300)]
SMALL = [(2, 2), (2, 9), (5, 2)]


# ----------------------------------------------------------------------------- the elementwise expressions

def _nb(a, mode):
    """the left, right, upper and lower neighbour of every pixel; outside the grid 0 ('zero') or the pixel itself ('self')"""
    p = np.pad(a, 1, mode="constant" if mode == "zero" else "edge")
    return p[1:-1, :-2], p[1:-1, 2:], p[:-2, 1:-1], p[2:, 1:-1]


def weights0(gx, gy, w):
    """the pixel weights a solve uses: w where w > 0, else 0; without w, 1 where both gradients are finite"""
    if w is None:
        return (np.isfinite(gx) & np.isfinite(gy)).astype(np.float64)
    w = np.asarray(w, dtype=np.float64)
    return np.where(w > 0, w, 0.0)


def edge_weights(w):
    l, r, u, d = _nb(w, "zero")
    return np.minimum(l, w), np.minimum(w, r), np.minimum(u, w), np.minimum(w, d)


def diag(w):
    wl, wr, wu, wd = edge_weights(w)
    return ((wl + wr) + wu) + wd


def rhs(w, gx, gy):
    wl, wr, wu, wd = edge_weights(w)
    gxl, gxr, _, _ = _nb(gx, "zero")
    _, _, gyu, gyd = _nb(gy, "zero")
    with np.errstate(invalid="ignore", over="ignore"):
        tl = np.where(wl > 0, wl * (0.5 * (gxl + gx)), 0.0)
        tr = np.where(wr > 0, wr * (0.5 * (gx + gxr)), 0.0)
        tu = np.where(wu > 0, wu * (0.5 * (gyu + gy)), 0.0)
        td = np.where(wd > 0, wd * (0.5 * (gy + gyd)), 0.0)
    return ((tl - tr) + tu) - td


def apply_L(w, x):
    wl, wr, wu, wd = edge_weights(w)
    xl, xr, xu, xd = _nb(x, "self")
    return ((wl * (x - xl) + wr * (x - xr)) + wu * (x - xu)) + wd * (x - xd)


def sweep0(d, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(d > 0, OMEGA * (b / d), 0.0)


def sweep(w, d, x, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(d > 0, x + OMEGA * ((b - apply_L(w, x)) / d), x)


def jacobi0(d, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(d > 0, b / d, 0.0)


def coarse_shape(shape):
    return ((shape[0] + 1) // 2, (shape[1] + 1) // 2)


def _pweights(n):
    """the 1-D prolongation weights of the fine nodes 2 I - 1, 2 I, 2 I + 1 on the coarse node I (0: no such node)"""
    nc = (n + 1) // 2
    I = np.arange(nc)
    pm = np.where(I >= 1, 0.5, 0.0)
    p0 = np.ones(nc)
    pp = np.where(2 * I + 1 < n, np.where(I + 1 < nc, 0.5, 1.0), 0.0)
    return pm, p0, pp


def restrict(r):
    """P' r: rows of three first (left, centre, right), then the three rows (upper, centre, lower)"""
    H, W = r.shape
    Hc, Wc = coarse_shape(r.shape)
    p = np.zeros((2 * Hc + 2, 2 * Wc + 2))
    p[1:H + 1, 1:W + 1] = r
    am, a0, ap = (v[:, None] for v in _pweights(H))
    bm, b0, bp = (v[None, :] for v in _pweights(W))
    s = [(bm * p[k:k + 2 * Hc:2, 0:2 * Wc:2] + b0 * p[k:k + 2 * Hc:2, 1:2 * Wc + 1:2]) + bp * p[k:k + 2 * Hc:2, 2:2 * Wc + 2:2]
         for k in range(3)]
    return (am * s[0] + a0 * s[1]) + ap * s[2]


def prolong(e, shape):
    """P e: along the rows first, then along the columns; an odd node averages, the last node of an even axis copies"""
    H, W = shape
    Hc, Wc = e.shape
    v = np.empty((Hc, W))
    v[:, 0::2] = e
    for j in range(1, W, 2):
        J = j // 2
        v[:, j] = 0.5 * (e[:, J] + e[:, J + 1]) if J + 1 < Wc else e[:, J]
    out = np.empty((H, W))
    out[0::2] = v
    for i in range(1, H, 2):
        I = i // 2
        out[i] = 0.5 * (v[I] + v[I + 1]) if I + 1 < Hc else v[I]
    return out


def coarsen(w):
    return restrict(w) / restrict(np.ones_like(w))


def levels(w):
    """[(w, d)] from the fine grid down to the first level with min(H, W) <= COARSEST"""
    out = [(w, diag(w))]
    while min(out[-1][0].shape) > COARSEST:
        wc = coarsen(out[-1][0])
        out.append((wc, diag(wc)))
    return out


def vcycle(lv, r, l=0, trace=None):
    """z = M r on the hierarchy of levels(w)"""
    w, d = lv[l]
    if l == len(lv) - 1:
        x = sweep0(d, r)
        for _ in range(COARSE_SWEEPS - 1):
            x = sweep(w, d, x, r)
        return x
    x = sweep0(d, r)
    for _ in range(NU - 1):
        x = sweep(w, d, x, r)
    rc = restrict(r - apply_L(w, x))
    if trace is not None:
        trace.append(rc)
    x = x + prolong(vcycle(lv, rc, l + 1, trace), w.shape)
    for _ in range(NU):
        x = sweep(w, d, x, r)
    return x


# ----------------------------------------------------------------------------- the solve

def ldot(a, b):
    return float((a.astype(np.longdouble) * b.astype(np.longdouble)).sum())


def lnorm(a):
    a = a.astype(np.longdouble)
    return float(np.sqrt((a * a).sum()))


def true_residual(w, b, x):
    """|b - L x|_2 / |b|_2 in extended precision, and the rounding bound of a double evaluation of it, relative to |b|:
    each of the n squares and the sum within (n + 2) 2^-53 of sum r^2, the residual's own elements within a few ulp of
    the magnitudes that cancel in them (8 operations and the gauge subtraction: 2^-53 * 12 * (|b| + sum w_e (|x_p| + |x_q|)))"""
    r = b - apply_L(w, x)
    bn = lnorm(b)
    n = b.size
    wl, wr, wu, wd = edge_weights(w)
    xl, xr, xu, xd = _nb(np.abs(x), "self")
    mag = np.abs(b) + wl * (np.abs(x) + xl) + wr * (np.abs(x) + xr) + wu * (np.abs(x) + xu) + wd * (np.abs(x) + xd)
    dr = 12.0 * 2.0 ** -53 * lnorm(mag)
    rn = lnorm(r)
    return rn / bn, (rn * (n + 2) * 2.0 ** -53 + dr) / bn


def pcg(gx, gy, w=None, tol=1e-10, maxiter=500, jacobi=False):
    """(phi with the gauge removed and NaN at d = 0, iterations, true relative residual, status)"""
    w0 = weights0(gx, gy, w)
    lv = levels(w0) if not jacobi else None
    d = diag(w0)
    b = rhs(w0, gx, gy)
    M = (lambda r: jacobi0(d, r)) if jacobi else (lambda r: vcycle(lv, r))
    x = np.zeros_like(b)
    bn = np.sqrt(ldot(b, b))
    it, status = 0, MAXITER
    if bn == 0.0:
        status = CONVERGED
    else:
        r = b.copy()
        z = M(r)
        p = z.copy()
        rz = ldot(r, z)
        while it < maxiter:
            Ap = apply_L(w0, p)
            pAp = ldot(p, Ap)
            if not (pAp > 0 and np.isfinite(pAp)):
                status = BREAKDOWN
                break
            alpha = rz / pAp
            x = x + alpha * p
            r = r - alpha * Ap
            it += 1
            reset = False
            if np.sqrt(ldot(r, r)) <= tol * bn:
                r = b - apply_L(w0, x)
                if np.sqrt(ldot(r, r)) <= tol * bn:
                    status = CONVERGED
                    break
                reset = True
            z = M(r)
            rzn = ldot(r, z)
            beta = 0.0 if reset else rzn / rz
            p = z + beta * p
            rz = rzn
    resid = 0.0 if bn == 0.0 else np.sqrt(ldot(b - apply_L(w0, x), b - apply_L(w0, x))) / bn
    on = d > 0
    mean = float(x[on].astype(np.longdouble).sum() / max(1, on.sum()))
    return np.where(on, x - mean, np.nan), it, resid, status


# ----------------------------------------------------------------------------- the dense reference

def assemble(w0):
    H, W = w0.shape
    n = H * W
    wl, wr, wu, wd = edge_weights(w0)
    L = np.zeros((n, n))
    idx = np.arange(n).reshape(H, W)
    L[idx, idx] = diag(w0)
    L[idx[:, 1:], idx[:, :-1]] = -wl[:, 1:]
    L[idx[:, :-1], idx[:, 1:]] = -wr[:, :-1]
    L[idx[1:], idx[:-1]] = -wu[1:]
    L[idx[:-1], idx[1:]] = -wd[:-1]
    return L


def components(w0):
    from scipy import ndimage
    lab, n = ndimage.label(w0 > 0)
    return lab, n


def demean(phi, w0):
    """phi minus the mean of each connected component of the positive-weight graph; NaN where d = 0"""
    lab, n = components(w0)
    out = np.full(phi.shape, np.nan)
    on = diag(w0) > 0
    for c in range(1, n + 1):
        m = (lab == c) & on
        if m.any():
            out[m] = phi[m] - phi[m].mean()
    return out


_dense, _golden = {}, {}


def dense_live(name):
    """the dense least-squares solution of a case, component-demeaned, solved once per process"""
    if name not in _dense:
        gx, gy, w, _ = case(name)
        w0 = weights0(gx, gy, w)
        b = rhs(w0, gx, gy)
        sol, _, _, sv = np.linalg.lstsq(assemble(w0), b.ravel(), rcond=None)
        _dense[name] = demean(sol.reshape(b.shape), w0)
        _dense[name, "sv"] = sv
    return _dense[name]


def dense_error(name):
    """what a dense solve of a case is good for: 4 cond(L) 2^-53 max |Phi|, cond(L) from the singular values lstsq kept
    (those above its own cut-off; the others span the constants of the components)"""
    ref = dense_live(name)
    sv = _dense[name, "sv"]
    kept = sv[sv > sv.max() * sv.size * 2.0 ** -52]
    return float(4.0 * (kept.max() / kept.min()) * 2.0 ** -53 * np.nanmax(np.abs(ref)))


def _golden_dir():
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def dense(name):
    """the same solution as recorded in tests/golden/integrate_dense.npz (tests/golden/make_golden_integrate.py)"""
    import os
    if "dense" not in _golden:
        _golden["dense"] = np.load(os.path.join(_golden_dir(), "integrate_dense.npz"))
    return _golden["dense"][name]


def observed():
    """tests/golden/integrate_observed.json: case -> {'deviation', 'iterations'} of the restated solve"""
    import json
    import os
    if "observed" not in _golden:
        _golden["observed"] = json.load(open(os.path.join(_golden_dir(), "integrate_observed.json")))
    return _golden["observed"]


def deviation(phi, name, ref=None):
    """the worst component-demeaned deviation of a result from the dense solution of a case"""
    gx, gy, w, _ = case(name)
    w0 = weights0(gx, gy, w)
    ref = dense(name) if ref is None else ref
    on = np.isfinite(ref)
    assert (np.isfinite(phi) == on).all()
    got = demean(np.where(on, phi, 0.0), w0)
    return float(np.abs(got[on] - ref[on]).max())


# ----------------------------------------------------------------------------- the cases

def smooth_phi(shape, seed):
    """a smooth map with a range of about 5"""
    H, W = shape
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    phi = np.zeros(shape)
    for _ in range(4):
        a, fi, fj, pi_, pj = rng.uniform(0.5, 1.0), rng.uniform(0.5, 2.5), rng.uniform(0.5, 2.5), rng.uniform(0, 6.3), rng.uniform(0, 6.3)
        phi += a * np.sin(2 * np.pi * fi * i + pi_) * np.cos(2 * np.pi * fj * j + pj)
    return phi * (5.0 / (phi.max() - phi.min()))


def gradients(phi, seed, noise=0.01):
    rng = np.random.default_rng(seed + 1000)
    gx = np.gradient(phi, axis=1) + noise * rng.standard_normal(phi.shape)
    gy = np.gradient(phi, axis=0) + noise * rng.standard_normal(phi.shape)
    return gx, gy


def hole_weights(shape, seed):
    """5 % random zeros, a zero block of about H/6 x W/5, one full zero column, 10 % of the pixels at 0.3"""
    H, W = shape
    rng = np.random.default_rng(seed + 2000)
    w = np.ones(shape)
    w[rng.random(shape) < 0.10] = 0.3
    w[rng.random(shape) < 0.05] = 0.0
    bh, bw = max(1, H // 6), max(1, W // 5)
    i0, j0 = H // 3, W // 4
    w[i0:i0 + bh, j0:j0 + bw] = 0.0
    if W >= 8:
        w[:, (2 * W) // 3] = 0.0
    return w


_cases = {}


def case(name):
    """name = '<H>x<W>_<ones|holes>': (gx, gy, w, phi); NaN gradients wherever the weight is 0"""
    if name not in _cases:
        dims, kind = name.split("_")
        shape = tuple(int(v) for v in dims.split("x"))
        seed = shape[0] * 1000 + shape[1]
        phi = smooth_phi(shape, seed)
        gx, gy = gradients(phi, seed)
        if kind == "ones":
            w = np.ones(shape)
        else:
            w = hole_weights(shape, seed)
            gx[w == 0] = np.nan
            gy[w == 0] = np.nan
        for a in (gx, gy, w, phi):
            a.setflags(write=False)
        _cases[name] = (gx, gy, w, phi)
    return _cases[name]


def case_name(shape, kind):
    return "%dx%d_%s" % (shape[0], shape[1], kind)
