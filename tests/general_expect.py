"""
tests/general_expect.py -- the inputs and expectations of the grid consumers on the general table (model.general_grid,
umpa_grid_set_general), built WITHOUT the code under test.

The expected volumes are oracle/hp_cost.hp_cells' (numpy.longdouble, with the a-priori bound of an fp64 evaluation).  hp_cells
takes all frames at position (0, 0) and all of them contributing, so the frames are embedded in a common canvas at their
positions, the pixels are grouped by the set of frames that contribute to them (a frame contributes to a pixel iff the pixel
keeps `padding` from its edges: lib/Model.cpp:428-433) and each group is evaluated on its subset of the frames -- inside a
contributing frame every window lies in the frame, so the canvas outside it is never read.  Without masks the model divides
the cost by its OWN frame count, hp_cells by the subset's: cost and bound are scaled by |S| / Na.  With masks both divide by
the sum of the pair weights.  A pixel no frame contributes to has 0 / 0: NaN.

Inputs:
  D  tests/golden/D_stepping.npz: 4 frames of 64x72, 64x72, 60x76, 64x72 at (0,0), (0,12), (10,0), (10,12), Nw 2, max_shift 4,
     extent 62 x 72; the masks of the masked cases: per frame ``default_rng(15).random(shape) >= 0.05``, drawn in frame order.
  E  a 2 x 2 stepping stack of equal shapes (umpa_amd.synth.make_stack), so that stage_sample, Tracker and Sequence apply.
  P  grid_expect.STACKS["64x72x3"], all frames at (0, 0): the model forced onto the direct kernel.
  edge stacks of a few dozen rows: Nw 1 and 8, max_shift 2 and 8, 1 and 26 frames, 64, 65 and 70 columns.
"""
import functools

import numpy as np

from conftest import Case

import grid_expect as GE

LD = np.longdouble
MODES = [(0, "sam"), (0, "ref"), (1, "sam"), (1, "ref")]
# what the issue's author counted on D on a CPU: distinct contributing-frame sets, pixels no frame contributes to,
# single-frame pixels
D_SETS, D_DEAD, D_SINGLE = 11, 36, 524


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ----------------------------------------------------------------------------- geometry

def extent_of(shapes, pos, pad):
    H = max(p[0] + s[0] for p, s in zip(pos, shapes))
    W = max(p[1] + s[1] for p, s in zip(pos, shapes))
    return H - 2 * pad, W - 2 * pad


def contributes(shapes, pos, pad):
    """[Na, N0, N1] bool: frame k contributes to output pixel (xi, xj) (image pixel (pad + xi, pad + xj))"""
    N0, N1 = extent_of(shapes, pos, pad)
    i, j = np.meshgrid(np.arange(N0) + pad, np.arange(N1) + pad, indexing="ij")
    out = np.zeros((len(shapes), N0, N1), dtype=bool)
    for k, ((H, W), (pi, pj)) in enumerate(zip(shapes, pos)):
        li, lj = i - pi, j - pj
        out[k] = ~((li - pad < 0) | (li + pad > H) | (lj - pad < 0) | (lj + pad > W))
    return out


def frame_sets(shapes, pos, pad):
    """[N0, N1] int: the contributing frames of a pixel as a bit set"""
    c = contributes(shapes, pos, pad)
    return (c * (1 << np.arange(len(shapes)))[:, None, None]).sum(axis=0)


def canvas(frames, pos):
    """[Na, H, W]: every frame at its position in the image the frames tile, zeros elsewhere"""
    H = max(p[0] + f.shape[0] for p, f in zip(pos, frames))
    W = max(p[1] + f.shape[1] for p, f in zip(pos, frames))
    out = np.zeros((len(frames), H, W))
    for k, (f, (pi, pj)) in enumerate(zip(frames, pos)):
        out[k, pi:pi + f.shape[0], pj:pj + f.shape[1]] = f
    return out


def covered_of(shapes, pos, pad, masks=None):
    """``coverage >= thr`` as ``match()`` forms it (model.pyx:499-529, :431): the coverage of a pixel is the sum over the
    contributing frames of the mask at the pixel (1 without masks); thr = 0.1 max / Na"""
    c = contributes(shapes, pos, pad).astype(np.float64)
    if masks is not None:
        N0, N1 = c.shape[1:]
        c = c * canvas(masks, pos)[:, pad:pad + N0, pad:pad + N1]
    cov = c.sum(axis=0)
    return cov >= 0.1 * cov.max() / len(shapes)


def hp_of(sam, ref, pos, Nw, ms, kind, assign, masks=None, pixels=None):
    """The extended-precision volumes of a stack of frames at positions `pos`: cost, T, df (None without dark-field) and
    bound as [U, U, ...pixels] longdouble arrays (`pixels` = (xi, xj) output pixels; default: all of them), NaN where no frame
    contributes; plus `sets` (the pixels' frame sets).  Read-only."""
    from oracle import hp_cost
    pad, U, Na = Nw + ms, 2 * ms - 1, len(sam)
    shapes = [f.shape for f in sam]
    N0, N1 = extent_of(shapes, pos, pad)
    if pixels is None:
        pixels = np.meshgrid(np.arange(N0), np.arange(N1), indexing="ij")
    xi, xj = (np.asarray(v) for v in pixels)
    sets = frame_sets(shapes, pos, pad)[xi, xj]
    cs, cr = canvas(sam, pos), canvas(ref, pos)
    cm = canvas(masks, pos) if masks is not None else None
    sh = np.arange(U) - ms + 1
    out = {k: np.full((U, U) + xi.shape, np.nan, dtype=LD) for k in ("cost", "T", "bound")}
    out["df"] = np.full((U, U) + xi.shape, np.nan, dtype=LD) if kind else None
    for s in np.unique(sets):
        if s == 0:
            continue
        sub = [k for k in range(Na) if s >> k & 1]
        sel = sets == s
        pi, pj = xi[sel] + pad, xj[sel] + pad
        shape = (U, U, pi.size)
        si = np.broadcast_to(sh.reshape(U, 1, 1), shape)
        sj = np.broadcast_to(sh.reshape(1, U, 1), shape)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            r = hp_cost.hp_cells(kind, cs[sub], cr[sub], GE.window(Nw), np.broadcast_to(pi, shape), np.broadcast_to(pj, shape), si, sj,
                                 assign, mask=cm[sub] if cm is not None else None)
        f = LD(1) if masks is not None else LD(len(sub)) / LD(Na)
        out["cost"][:, :, sel] = r["cost"].reshape(shape) * f
        out["bound"][:, :, sel] = r["bound"].reshape(shape) * f
        out["T"][:, :, sel] = r["T"].reshape(shape)
        if kind:
            out["df"][:, :, sel] = r["df"].reshape(shape)
    out["sets"] = sets
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


def near_tie_share(v):
    """the share of grid_expect.near_tie among the pixels with a finite cost (masked_grid_expect.near_tie's rule)"""
    import masked_grid_expect as ME
    fin = np.isfinite(v["cost"].astype(np.float64))
    U = fin.shape[0]
    some = fin.reshape((U * U,) + fin.shape[2:]).any(axis=0)
    return ME.near_tie(v).sum() / float(max(some.sum(), 1)), ME.near_tie(v)


# ----------------------------------------------------------------------------- D

@functools.lru_cache(maxsize=None)
def D():
    """(sam frames, ref frames, positions, Nw, ms)"""
    c = Case("D_stepping")
    frozen(*c.sam, *c.ref)
    return c.sam, c.ref, [tuple(int(x) for x in p) for p in c.pos], c.Nw, c.max_shift


@functools.lru_cache(maxsize=None)
def D_masks():
    rng = np.random.default_rng(15)
    return frozen(*[(rng.random(f.shape) >= 0.05).astype(np.float64) for f in D()[0]])


D_CASES = [(k, a, mk) for k, a in MODES for mk in (False, True)]
D_IDS = ["%s-%s-%s" % ("DF" if k else "NoDF", a, "mask" if mk else "plain") for k, a, mk in D_CASES]


@functools.lru_cache(maxsize=None)
def D_hp(kind, assign, masked):
    sam, ref, pos, Nw, ms = D()
    return hp_of(sam, ref, pos, Nw, ms, kind, assign, masks=D_masks() if masked else None)


def D_sets():
    sam, _, pos, Nw, ms = D()
    return frame_sets([f.shape for f in sam], pos, Nw + ms)


def D_covered(masked):
    sam, _, pos, Nw, ms = D()
    return covered_of([f.shape for f in sam], pos, Nw + ms, D_masks() if masked else None)


def D_sample():
    """(xi, xj): about 60 output pixels -- the corners of every frame-set cell (the bounding box of the set's pixels), the
    seams of the 16 x 16 pixel workgroups around the middle, and the extent's corners"""
    sets = D_sets()
    N0, N1 = sets.shape
    px = set()
    for s in np.unique(sets):
        r, c = np.nonzero(sets == s)
        px |= {(r.min(), c[r == r.min()].min()), (r.min(), c[r == r.min()].max()), (r.max(), c[r == r.max()].min()),
               (r.max(), c[r == r.max()].max())}
    px |= {(15, 15), (15, 16), (16, 15), (16, 16), (31, 47), (32, 48), (47, 63), (48, 64), (61, 71), (0, 0), (0, 71), (61, 0)}
    px = sorted((int(a), int(b)) for a, b in px)
    return np.array([p[0] for p in px]), np.array([p[1] for p in px])


# ----------------------------------------------------------------------------- E: 2 x 2 stepping, equal shapes

E_PAR = dict(H=56, W=64, K=4, Nw=2, ms=3, off=8)


@functools.lru_cache(maxsize=None)
def E(seed=0):
    """(sam frames, ref frames, positions): four frames of (H - off) x (W - off) cut from one stack at the corners of a 2 x 2
    grid of step `off`, tools/stepping_rate.py's layout.  `seed` > 0: another sample stack on the same reference (a series)."""
    from umpa_amd.synth import make_stack
    p = E_PAR
    sam, ref, _ = make_stack(p["H"], p["W"], p["K"], p["ms"], df=True, seed=80, amplitude=p["ms"] - 1.2, order=1)
    if seed:
        sam = sam + 0.002 * np.random.default_rng(seed).standard_normal(sam.shape)
    h, w = p["H"] - p["off"], p["W"] - p["off"]
    pos = [(p["off"] * ((k // 2) % 2), p["off"] * (k % 2)) for k in range(p["K"])]
    return ([np.ascontiguousarray(sam[k, :h, :w]) for k in range(p["K"])], [np.ascontiguousarray(ref[k, :h, :w]) for k in range(p["K"])], pos)


# ----------------------------------------------------------------------------- P: forced direct

P_NAME = "64x72x3"


# ----------------------------------------------------------------------------- the edge stacks

EDGE_ROWS = 21                                                       # no multiple of 16: the last workgroup row is ragged
# (Nw, max_shift, frames, columns, kind, assign, masked)
EDGE_CASES = [
    (1, 2, 3, 70, 0, "sam", False), (1, 2, 3, 64, 1, "ref", True),
    (8, 3, 2, 65, 1, "sam", False), (8, 2, 2, 70, 0, "ref", True),
    (1, 8, 3, 70, 1, "ref", False), (2, 8, 3, 65, 0, "sam", True),
    (2, 3, 1, 64, 0, "ref", False), (2, 3, 1, 65, 1, "sam", True),
    (1, 3, 26, 70, 1, "sam", False), (1, 3, 26, 64, 0, "ref", True),
]
EDGE_IDS = ["Nw%d-ms%d-Na%d-w%d-%s-%s-%s" % (c[0], c[1], c[2], c[3], "DF" if c[4] else "NoDF", c[5], "mask" if c[6] else "plain")
            for c in EDGE_CASES]


@functools.lru_cache(maxsize=None)
def edge_inputs(Nw, ms, Na, N1):
    """(sam frames, ref frames, positions, masks): `Na` frames whose extent is EDGE_ROWS x N1 pixels; from two frames on,
    odd frames are stepped by (3, 5), so that the extent's border has pixels only some frames contribute to"""
    from umpa_amd.synth import make_stack
    pad = Nw + ms
    dr, dc = (3, 5) if Na > 1 else (0, 0)
    H, W = EDGE_ROWS + 2 * pad - dr, N1 + 2 * pad - dc
    sam, ref, _ = make_stack(H, W, Na, ms, df=True, seed=900 + 10 * ms + Nw, amplitude=max(ms - 1.2, 0.5), order=1)
    pos = [(dr * (k % 2), dc * (k % 2)) for k in range(Na)]
    rng = np.random.default_rng(950 + 10 * ms + Nw)
    masks = (rng.random(sam.shape) >= 0.05).astype(np.float64)
    frozen(sam, ref, masks)
    return [sam[k] for k in range(Na)], [ref[k] for k in range(Na)], pos, [masks[k] for k in range(Na)]


@functools.lru_cache(maxsize=None)
def edge_hp(Nw, ms, Na, N1, kind, assign, masked):
    sam, ref, pos, masks = edge_inputs(Nw, ms, Na, N1)
    return hp_of(sam, ref, pos, Nw, ms, kind, assign, masks=masks if masked else None)


def within_bound(got, v, what):
    """every finite entry of hp's volume: |got - hp| <= bound; where hp is NaN (no frame, or no pair weight), got is not a
    number below +Inf.  Returns the largest ratio."""
    hp = v["cost"]
    fin = np.isfinite(hp.astype(np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.abs(got.astype(LD) - hp) / v["bound"]
        assert not (got[~fin] < np.inf).any(), "%s: a cost where the expectation has none" % what
    assert np.isfinite(got[fin]).all(), "%s: %d entries are not finite" % (what, (~np.isfinite(got[fin])).sum())
    worst = float(ratio[fin].max()) if fin.any() else 0.0
    assert worst <= 1.0, "%s: max |gpu - hp| / bound = %.4f" % (what, worst)
    return worst
