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
    out["df_bound"] = np.full((U, U) + xi.shape, np.nan, dtype=LD) if kind else None      # hp_cells' a-priori RELATIVE bound of df
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
            out["df_bound"][:, :, sel] = r["df_bound"].reshape(shape)
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


# ----------------------------------------------------------------------------- the LDS geometry (umpa_general_geom.h)

LDS_LIMIT = 64 * 1024


def lds_geometry(Nw, ms, step0, step1, masked, ref_mode, by=16, bx=16):
    """general_footprints restated: ("staged" | "fallback", LDS bytes; 0 where a box side passes 4096 and nothing is computed)"""
    boxr, boxc = (by - 1) * step0 + 1, (bx - 1) * step1 + 1
    wide = Nw + (ms - 1 if ms > 1 else 0)
    if boxr + 2 * wide > 4096 or boxc + 2 * wide > 4096:
        return "fallback", 0
    hq, hr = (wide, Nw) if ref_mode else (Nw, wide)
    even = lambda n: (n + 1) & ~1
    offR = even((boxr + 2 * hq) * (boxc + 2 * hq))
    offM = even(offR + (boxr + 2 * hr) * (boxc + 2 * hr))
    offW = even(offM + ((boxr + 2 * wide) * (boxc + 2 * wide) if masked else 0))
    nbytes = 8 * (offW + (2 * Nw + 1) ** 2 + 2)
    return ("staged" if nbytes <= LDS_LIMIT else "fallback"), nbytes


# (Nw, ms, step0, step1, masked, ref_mode) -> what tests/general_addr_check.cpp printed for it (the program is the authority; the
# CPU test holds the restatement above and this table to its output).  The first three are the issue's worked cases.
LDS_CASES = [
    ((1, 2, 4, 4, 0, 0), ("fallback", 65656)), ((1, 2, 4, 3, 0, 0), ("staged", 50280)), ((1, 2, 3, 4, 0, 0), ("staged", 50280)),
    ((1, 1, 4, 4, 0, 0), ("staged", 63608)), ((1, 1, 4, 5, 0, 0), ("fallback", 78712)), ((1, 1, 5, 4, 0, 0), ("fallback", 78712)),
    ((1, 2, 3, 3, 1, 1), ("staged", 58520)), ((1, 2, 3, 4, 1, 1), ("fallback", 76280)), ((1, 2, 2, 3, 0, 0), ("staged", 26760)),
    ((1, 2, 5, 5, 0, 0), ("fallback", 99960)), ((2, 3, 1, 1, 1, 0), ("staged", 12632)), ((8, 9, 1, 1, 1, 1), ("staged", 47384)),
    ((8, 9, 2, 2, 1, 1), ("fallback", 83528)), ((8, 9, 2, 1, 1, 1), ("staged", 62744)), ((0, 1, 5, 5, 0, 0), ("fallback", 92440)),
    ((0, 1, 6, 5, 0, 0), ("fallback", 110680)), ((1, 3, 273, 1, 0, 0), ("fallback", 0)), ((1, 3, 1, 273, 1, 1), ("fallback", 0)),
]
# the GPU cases either side of the limit, taken from that list: (Nw, ms, kind, assign, masked, staged step, fallback step)
LIMIT_CASES = [
    (1, 2, 0, "sam", False, (4, 3), (4, 4)),
    (1, 2, 1, "sam", False, (3, 4), (4, 4)),
    (1, 1, 0, "sam", False, (4, 4), (4, 5)),                          # max_shift 1: U = 1, a pass is one valid set and three aliases
    (1, 1, 1, "sam", False, (4, 4), (5, 4)),
    (1, 2, 1, "ref", True, (3, 3), (3, 4)),
    (1, 2, 0, "ref", True, (3, 3), (3, 4)),
]
LIMIT_IDS = ["Nw%d-ms%d-%s-%s-%s" % (c[0], c[1], "DF" if c[2] else "NoDF", c[3], "mask" if c[4] else "plain") for c in LIMIT_CASES]
LIMIT_COLS = 66


def limit_listed(case):
    """the two steps of a LIMIT_CASES row as LDS_CASES has them: (staged entry, fallback entry)"""
    Nw, ms, _, assign, masked, st, fb = case
    table = dict(LDS_CASES)
    return tuple(table[(Nw, ms, s[0], s[1], int(masked), int(assign == "ref"))] for s in (st, fb))


# ----------------------------------------------------------------------------- input regimes

REGIME_NAMES = ("x2^16", "x2^-5", "counts200", "vis1e-2", "vis1e-3", "zero_mean")
EDGE26 = {0: (1, 3, 26, 64, 0, "ref", True), 1: (1, 3, 26, 70, 1, "sam", False)}     # the two 26-frame rows of EDGE_CASES
INSTANCES = [(0, False), (0, True), (1, False), (1, True)]           # general_table_kernel<KIND, MASK>


def _regime_cases():
    """(regime, stack, kind, assign, masked): on D every regime meets the four kernel instantiations, the coordinate mode
    alternating over them and over the regimes -- and both modes for the two regimes whose costs are the smallest beside
    their sums, as masked_grid_expect.REGIME_CASES has it; on the 26-frame edge stack the regimes alternate between its two
    rows of EDGE_CASES"""
    out = []
    for q, r in enumerate(REGIME_NAMES):
        for n, (kind, masked) in enumerate(INSTANCES):
            modes = ("sam", "ref") if r in ("vis1e-3", "zero_mean") else (("sam", "ref")[(q + n) % 2],)
            out += [(r, "D", kind, a, masked) for a in modes]
        e = EDGE26[q % 2]
        out.append((r, "edge", e[4], e[5], e[6]))
    return out


REGIME_CASES = _regime_cases()
REGIME_IDS = ["%s-%s-%s-%s-%s" % (r, s, "DF" if k else "NoDF", a, "mask" if mk else "plain") for r, s, k, a, mk in REGIME_CASES]


# REGIME_IDS entry -> finite cells whose a-priori relative bound of an fp64 df (hp_cells' df_bound) is above the parity bar
# of 1e-5, counted from extended precision alone (tests/test_general_regimes_cpu.py holds the table to it; every other
# dark-field case has none).  On those cells a numerator of df cancels and df is held to model.cost alone; at visibility 1e-3
# they are 6 % of the volume.
DF_LOOSE = {
    "x2^16-D-DF-ref-mask": 1, "x2^-5-D-DF-sam-mask": 1,
    "vis1e-2-D-DF-ref-plain": 142, "vis1e-2-D-DF-sam-mask": 104, "vis1e-2-edge-DF-sam-plain": 245,
    "vis1e-3-D-DF-sam-plain": 13500, "vis1e-3-D-DF-ref-plain": 13402, "vis1e-3-D-DF-sam-mask": 12927, "vis1e-3-D-DF-ref-mask": 12828,
}


def apply_regime(regime, sam, ref):
    """a tests/regimes.py generator on lists of frames of unequal shapes: each stack as one array (a generator reads a stack's
    values and its mean, never its shape), cut back into the frames"""
    import regimes as RG
    flat = lambda fs: np.concatenate([np.asarray(f).ravel() for f in fs])
    s, r = RG.REGIMES[regime](flat(sam), flat(ref), None)
    cut = lambda x, fs: [np.ascontiguousarray(a.reshape(f.shape)) for a, f in zip(np.split(x, np.cumsum([f.size for f in fs])[:-1]), fs)]
    s, r = cut(s, sam), cut(r, ref)
    frozen(*s, *r)
    return s, r


@functools.lru_cache(maxsize=None)
def regime_inputs(regime, stack):
    """(sam, ref, pos, Nw, ms, masks): D, or the 26-frame edge stack of the regime's row, under the regime"""
    if stack == "D":
        sam, ref, pos, Nw, ms = D()
        masks = D_masks()
    else:
        Nw, ms, Na, N1 = EDGE26[REGIME_NAMES.index(regime) % 2][:4]
        sam, ref, pos, masks = edge_inputs(Nw, ms, Na, N1)
    s, r = apply_regime(regime, sam, ref)
    return s, r, pos, Nw, ms, masks


@functools.lru_cache(maxsize=4)
def regime_hp(regime, stack, kind, assign, masked):
    sam, ref, pos, Nw, ms, masks = regime_inputs(regime, stack)
    return hp_of(sam, ref, pos, Nw, ms, kind, assign, masks=masks if masked else None)


def pixel_sample(shapes, pos, pad):
    """D_sample's rule on any stack: the corners of every frame-set cell, the extent's corners and the workgroup seam"""
    sets = frame_sets(shapes, pos, pad)
    N0, N1 = sets.shape
    px = {(0, 0), (0, N1 - 1), (N0 - 1, 0), (N0 - 1, N1 - 1), (min(15, N0 - 1), 15), (min(16, N0 - 1), 16)}
    for s in np.unique(sets):
        r, c = np.nonzero(sets == s)
        px |= {(r.min(), c[r == r.min()].min()), (r.min(), c[r == r.min()].max()), (r.max(), c[r == r.max()].min()),
               (r.max(), c[r == r.max()].max())}
    px = sorted((int(a), int(b)) for a, b in px)
    return np.array([p[0] for p in px]), np.array([p[1] for p in px])


# ----------------------------------------------------------------------------- bad pixels on D

# name -> (frame, row, col in the frame).  D's frame 1 is 64 x 72 at (0, 12), frame 0 64 x 72 at (0, 0).  seam: image pixel
# (22, 34) = output pixel (16, 28) -- row 16 is a workgroup seam; column 32, the other seam, lies inside its window's reach.
# The last column is frame 0's: the extent ends before a pixel whose window reaches frame 1's.
BAD_POSITIONS = {"interior": (1, 30, 25), "seam": (1, 22, 22), "row0": (1, 0, 30), "col0": (1, 30, 0), "last_row": (1, 63, 30),
                 "last_col": (0, 30, 71)}


def bad_hit(where, assign, k, r, c):
    """[U, U, N0, N1] bool: the entries of D's volume whose window over the `where` stack, in frame k, holds the frame's
    pixel (r, c) while frame k contributes to the pixel.  The window that moves with the shift is the reference's in 'sam'
    mode (centre i + s) and the sample's in 'ref' mode (centre i - s); the other stays on the pixel."""
    sam, _, pos, Nw, ms = D()
    pad, U = Nw + ms, 2 * ms - 1
    contrib = contributes([f.shape for f in sam], pos, pad)[k]
    N0, N1 = contrib.shape
    xi, xj = np.meshgrid(np.arange(N0), np.arange(N1), indexing="ij")
    hit = np.zeros((U, U, N0, N1), dtype=bool)
    moves = (where == "ref") if assign == "sam" else (where == "sam")
    sign = 1 if assign == "sam" else -1
    for a in range(U):
        for b in range(U):
            si, sj = (sign * (a - ms + 1), sign * (b - ms + 1)) if moves else (0, 0)
            ci, cj = xi + pad + si - pos[k][0], xj + pad + sj - pos[k][1]
            hit[a, b] = contrib & (np.abs(ci - r) <= Nw) & (np.abs(cj - c) <= Nw)
    return hit


def bad_frames(value, where, name):
    """D with `value` written at BAD_POSITIONS[name] of frame k of the `where` stack: (sam, ref)"""
    import regimes as RG
    sam, ref = D()[:2]
    out = {"sam": [f.copy() for f in sam], "ref": [f.copy() for f in ref]}
    k, r, c = BAD_POSITIONS[name]
    out[where][k][r, c] = RG.BAD_VALUES[value]
    return out["sam"], out["ref"]


def bad_masks(weight, name):
    """D_masks() with `weight` at the bad pixel"""
    masks = [m.copy() for m in D_masks()]
    k, r, c = BAD_POSITIONS[name]
    masks[k][r, c] = weight
    return masks


# ----------------------------------------------------------------------------- what the masked path refuses (both switches on)

# which -> (Nw, ms, frames, columns): one frame with Nw 1 (exact fit: 1 x 9 <= 9), and a window half-width the masked table
# kernel has no configuration for (umpa_tiled.h: 1 to 8)
REFUSED = {"exact fit": (1, 2, 1, 40), "no configuration": (9, 2, 2, 40)}
REFUSED_MASK_SEED = 43            # (a seed under which no cell of either volume is rank-deficient: test_general_regimes_cpu.py)


@functools.lru_cache(maxsize=None)
def refused_inputs(which):
    """(sam, ref, masks, Nw, ms): EDGE_ROWS x 40 output pixels, all frames at (0, 0), 5 % of the mask pixels zero"""
    from umpa_amd.synth import make_stack
    Nw, ms, Na, N1 = REFUSED[which]
    pad = Nw + ms
    sam, ref, _ = make_stack(EDGE_ROWS + 2 * pad, N1 + 2 * pad, Na, ms, df=True, seed=40 + Nw, amplitude=0.8, order=1)
    mask = (np.random.default_rng(REFUSED_MASK_SEED).random(sam.shape) >= 0.05).astype(np.float64)
    frozen(sam, ref, mask)
    return sam, ref, mask, Nw, ms


@functools.lru_cache(maxsize=None)
def refused_hp(which, kind):
    sam, ref, mask, Nw, ms = refused_inputs(which)
    return hp_of(list(sam), list(ref), [(0, 0)] * len(sam), Nw, ms, kind, "sam", masks=list(mask))


# ----------------------------------------------------------------------------- D under weighted masks

@functools.lru_cache(maxsize=None)
def D_weights():
    """real-valued masks on D: uniform in (0, 1), 5 % of the pixels zero.  The pair weight ma mb / (ma + mb + 1e-8) then takes
    a different value at every window element -- under D_masks() it only ever takes 0 and 1 / (2 + 1e-8), which is blind to
    how the reciprocal is formed (pair_weight against pair_weight_fast, umpa_cost.h)"""
    rng = np.random.default_rng(16)
    return frozen(*[rng.uniform(0.0, 1.0, size=f.shape) * (rng.random(f.shape) >= 0.05) for f in D()[0]])


@functools.lru_cache(maxsize=None)
def D_hp_weighted(kind, assign):
    sam, ref, pos, Nw, ms = D()
    return hp_of(sam, ref, pos, Nw, ms, kind, assign, masks=D_weights())
