"""
Input regimes for tests/test_regimes_cpu.py and tests/test_hip_regimes.py (imported by both; not a conftest).

Every synthetic input of the rest of the suite is `umpa_amd.synth.make_stack`'s: finite values of 1 +- 0.3.  The
transforms below turn such a stack into the inputs real measurements bring: other scales (detector counts, data
normalised far below 1 -- where the walk's ABSOLUTE tie tolerance of 1e-8 starts to decide), low speckle contrast on a
large mean (where the expanded cost sums cancel), negative values, and NaN / Inf / 0 pixels.

CONFIGS names the matching paths of the library, one model configuration each; `run` builds and matches one of them on
either namespace (umpa_amd.model or the CPU oracle's), so that the CPU module judges exactly the cases the GPU module runs.

tests/consumer_expect.py takes the generators, BAD_VALUES and bad_positions from here for the consumers of the shift table
besides the walk (grid search, cost volume, aggregation, uncertainty, kernel search).
"""
import numpy as np

from umpa_amd import _lib
from umpa_amd.synth import make_stack


# ----------------------------------------------------------------------------- 1. regime generators

def scaled(sam, ref, e_sam, e_ref):
    """Multiply the stacks by exact powers of two."""
    return np.ascontiguousarray(np.ldexp(sam, e_sam)), np.ascontiguousarray(np.ldexp(ref, e_ref))


def tie_scaled(sam, ref, e, m):
    """Both stacks times m 2^e.  The band of scales between "the tie rule decides nothing" and "no walk converges" is about
    one octave wide (costs go with the square of the scale), so the second factor of a configuration is 0.75 2^e where the
    neighbouring power of two already lies outside the band."""
    return np.ascontiguousarray(np.ldexp(sam * m, e)), np.ascontiguousarray(np.ldexp(ref * m, e))


def counts(sam, ref, level, visibility):
    """Detector counts: the modulation about each stack's mean shrunk from make_stack's 0.3 to `visibility`, times
    `level`, rounded to integers (below 65536: the same arrays can be staged as uint16)."""
    out = []
    for x in (sam, ref):
        mean = x.mean()
        c = np.clip(np.rint(level * (mean + visibility / 0.3 * (x - mean))), 0, 65535)   # (a 4-sigma speckle dips below 0)
        out.append(np.ascontiguousarray(c, dtype=np.float64))
    return tuple(out)


def zero_mean(sam, ref):
    """Dark-subtracted background: values around zero, half of them negative."""
    return np.ascontiguousarray(sam - 1.0), np.ascontiguousarray(ref - 1.0)


# The call cap of 500 is tested in one place, the head of the walk's loop (Optim.cpp:267): the iteration that begins at 499 calls
# still makes its two probes and its gather (at most 16 calls), and a restart out of that gather (`goto start`, which skips the
# test) makes two more probes before the loop head ends the walk.  So 500 is not the largest Ncalls; 520 is a bound on it
# (the oracle reaches 507 on tiled_DF with NaN in the reference stack and 502 on staged_NoDF).
NCALLS_MAX = 520

BAD_VALUES = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "zero": 0.0}


def bad_positions(cfg):
    """(frame, row, col): one in the interior, one on a seam of the table kernels (output row 32 = a tile seam of
    corr_volume / corr_masked, UMPA_TILE; output column 48 = a strip seam of corr_march for 13- and 15-pixel windows,
    MarchCfg::WO, else column 32), one inside the padding border, one in the last frame."""
    pad, H, W, K = padding(cfg), cfg["H"], cfg["W"], cfg["K"]
    seam_col = pad + (48 if cfg["Nw"] >= 6 else 32)
    pos = [(0, H // 2 + 3, W // 2 - 5), (min(1, K - 1), pad + 32, seam_col), (0, 1, W // 3), (K - 1, H - pad - 2, W - pad - 7)]
    return pos[:cfg.get("n_bad", 4)]


def bad_pixels(sam, ref, kind, where, positions):
    """Write NaN, +Inf, -Inf or 0 at `positions` of the `where` ('sam' / 'ref') stack; returns new stacks."""
    sam, ref = sam.copy(), ref.copy()
    tgt = sam if where == "sam" else ref
    for (k, r, c) in positions:
        tgt[k, r, c] = BAD_VALUES[kind]
    return sam, ref


def checkers_agree(a, b):
    """Pixels on which two CPU results agree in the sense of the parity bar (i), (ii): err and Ncalls equal, T and df within
    1e-5 or NaN in both.  Around a non-finite pixel the checkers' answers are what their compiler (-ffast-math) made of NaN,
    not a specification; where the plain-C oracle and the in-place build of the reference still agree, the kernels are held
    to them."""
    ok = (a["err"] == b["err"]) & (a["debug_Ncalls"] == b["debug_Ncalls"])
    for k in ("T", "df"):
        if k in a:
            with np.errstate(invalid="ignore"):
                ok &= (np.abs(a[k] - b[k]) <= 1e-5 * np.abs(b[k])) | (np.isnan(a[k]) & np.isnan(b[k])) | (a[k] == b[k])
    return ok


def bad_key(name, kind, where):
    return "%s %s %s" % (name, kind, where)


def far_from(cfg, positions, shape, mk=None):
    """Output pixels further than Nw + max_shift (Chebyshev, input coordinates) from every bad pixel: what a bad pixel
    cannot reach -- a window has half-width Nw, the shift stays below max_shift (and the kernel dark-field's blur adds
    its 8 pixels, which the padding counts as well)."""
    step = (mk or cfg.get("mk", {})).get("step", 1)
    pad, reach = padding(cfg), padding(cfg)
    ii = pad + step * np.arange(shape[0])[:, None]
    jj = pad + step * np.arange(shape[1])[None, :]
    far = np.ones(shape, dtype=bool)
    for (k, r, c) in positions:
        p0, p1 = cfg["pos"][k] if cfg.get("pos") else (0, 0)          # frame-local position -> image coordinates
        far &= np.maximum(np.abs(ii - (r + p0)), np.abs(jj - (c + p1))) > reach
    return far


REGIMES = {
    "x2^16": lambda s, r, cfg: scaled(s, r, 16, 16),
    "x2^-5": lambda s, r, cfg: scaled(s, r, -5, -5),
    "tie_a": lambda s, r, cfg: tie_scaled(s, r, *cfg["tie"][0]),
    "tie_b": lambda s, r, cfg: tie_scaled(s, r, *cfg["tie"][1]),
    "counts200": lambda s, r, cfg: counts(s, r, 200, 0.3),
    "vis1e-2": lambda s, r, cfg: counts(s, r, 40000, 1e-2),
    "vis1e-3": lambda s, r, cfg: counts(s, r, 40000, 1e-3),
    "vis1e-4": lambda s, r, cfg: counts(s, r, 40000, 1e-4),
    "zero_mean": lambda s, r, cfg: zero_mean(s, r),
}
SWEEP_REGIMES = ["x2^16", "x2^-5", "tie_a", "tie_b", "counts200", "vis1e-2", "vis1e-3", "zero_mean"]


# ----------------------------------------------------------------------------- 2. the paths and their configurations

T, D, P = _lib.F_FORCE_TILED, _lib.F_FORCE_DIRECT, _lib.F_FORCE_PLAIN_DIRECT
_REF2 = dict(step=2, dxdy=(1, -1))

# name -> configuration.  path: what umpa_hip_last_path must say; tie: the two scale factors (e, m) -> m 2^e of the tie-rule regime
# (test_regimes_cpu.py asserts that they are in the regime); launch: a kernel the match must launch; table: a table-based path (cost from expanded sums).
CONFIGS = {
    "tiled_DF":      dict(df=True,  Nw=2, K=6,  ms=3, H=110, W=140, assign="sam", force=T, path=2, tie=((-9, 1.0), (-9, 0.75)), table=True, launch="corr_volume"),
    "tiled_DF10":    dict(df=True,  Nw=4, K=10, ms=4, H=116, W=150, assign="ref", force=T, path=2, tie=((-9, 1.0), (-9, 0.75)), table=True, launch="corr_volume"),
    "tiled_NoDF":    dict(df=False, Nw=3, K=5,  ms=4, H=124, W=150, assign="ref", force=T, path=2, tie=((-10, 1.0), (-9, 0.75)), table=True, mk=_REF2, launch="corr_volume"),
    "march_DF":      dict(df=True,  Nw=6, K=5,  ms=3, H=150, W=190, assign="sam", force=T, path=2, tie=((-9, 1.0), (-9, 0.75)), table=True, launch="corr_march"),
    "march_NoDF":    dict(df=False, Nw=7, K=3,  ms=3, H=150, W=190, assign="ref", force=T, path=2, tie=((-10, 1.0), (-10, 0.75)), table=True, launch="corr_march"),
    "masked_bin_DF":    dict(df=True,  Nw=3, K=5, ms=3, H=110, W=140, assign="sam", force=T, path=2, tie=((-9, 1.0), (-9, 0.75)), mask="binary", table=True, launch="corr_masked"),
    "masked_bin_NoDF":  dict(df=False, Nw=3, K=5, ms=3, H=110, W=140, assign="ref", force=T, path=2, tie=((-10, 1.0), (-10, 0.75)), mask="binary", table=True, launch="corr_masked"),
    "masked_w_DF":      dict(df=True,  Nw=3, K=5, ms=3, H=110, W=140, assign="ref", force=T, path=2, tie=((-9, 1.0), (-9, 0.75)), mask="weights", table=True, launch="corr_masked"),
    "masked_w_NoDF":    dict(df=False, Nw=3, K=5, ms=3, H=110, W=140, assign="sam", force=T, path=2, tie=((-10, 1.0), (-10, 0.75)), mask="weights", table=True, launch="corr_masked"),
    "masked_tiny_DF":   dict(df=True,  Nw=3, K=5, ms=3, H=110, W=140, assign="sam", force=T, path=2, tie=((-9, 1.0), (-9, 0.75)), mask="tiny", table=True, launch="corr_masked"),
    "masked_tiny_NoDF": dict(df=False, Nw=3, K=5, ms=3, H=110, W=140, assign="sam", force=T, path=2, tie=((-10, 1.0), (-10, 0.75)), mask="tiny", table=True, launch="corr_masked"),
    "staged_DF":     dict(df=True,  Nw=3, K=5, ms=3, H=100, W=120, assign="sam", force=D, path=3, tie=((-9, 1.0), (-9, 0.75)), launch="match_staged"),
    "staged_NoDF":   dict(df=False, Nw=3, K=5, ms=4, H=100, W=120, assign="ref", force=D, path=3, tie=((-10, 1.0), (-9, 0.75)), launch="match_staged"),
    "plain_DF":      dict(df=True,  Nw=3, K=5, ms=3, H=100, W=120, assign="ref", force=D | P, path=1, tie=((-9, 1.0), (-9, 0.75)), launch="match_direct"),
    "plain_NoDF":    dict(df=False, Nw=3, K=5, ms=4, H=100, W=120, assign="sam", force=D | P, path=1, tie=((-10, 1.0), (-9, 0.75)), mk=_REF2, launch="match_direct"),
    "stepping_DF":   dict(df=True,  Nw=3, K=4, ms=3, H=120, W=140, assign="sam", force=0, path=4, tie=((-9, 1.0), (-9, 0.75)),
                          pos=[(0, 0), (0, 9), (7, 0), (7, 9)]),
    "dfkernel":      dict(df=True,  Nw=2, K=3, ms=3, H=106, W=126, assign="sam", force=0, path=1, tie=((-9, 1.0), (-9, 0.75)), kernel=True, n_bad=1, launch="match_direct"),
}


# Further sample-stepping configurations for tests/test_hip_borrowed.py: the branch with the most host logic that only
# borrowed device frames reach (pair_slack, umpa_hip.hip).  They stand beside CONFIGS, not in it: every entry of CONFIGS is
# swept over all regimes by test_regimes_cpu.py / test_hip_regimes.py against recorded files (tests/golden/regime_observed.json,
# bad_pixel_agreement.npz), and the stacks' seeds go with the sorted names of CONFIGS.  `config(name)` finds both.
#   stepping_mask_DF, stepping_NoDF: the geometry of stepping_DF -- the centre rectangle (every frame, 102 x 119 pixels) is the
#     one tiled rectangle, every strip around it is below UMPA_STEP_CELL_MIN = 1024 pixels;
#   stepping_s2: a stepped ROI whose strips are tiled rectangles too, with descriptor lists of frame subsets: rows 17..68 x
#     columns 0..19 (frames 0, 2: 1040 pixels), rows 0..16 and 69..85 x columns 20..89 (frames 0, 1 and 2, 3: 1190 each) beside the
#     centre of 3640; the ROI starts on an even column so that image column pj + W - padding = 185 (region column 90), the last
#     one frames 0 and 2 contribute to, is in it.  Its whole region at step 1 has nine rectangles of 1365 to 14805 pixels.
STEPPING_EXTRA = {
    "stepping_mask_DF": dict(CONFIGS["stepping_DF"], mask="binary", seed=9931),
    "stepping_NoDF":    dict(CONFIGS["stepping_DF"], df=False, assign="ref", tie=((-10, 1.0), (-10, 0.75)), seed=9932),
    "stepping_s2":      dict(df=True, Nw=2, K=4, ms=3, H=150, W=190, assign="ref", force=0, path=4, pos=[(0, 0), (0, 40), (36, 0), (36, 40)],
                             mk=dict(ROI=((3, 174, 2), (0, 217, 2))), seed=9933),
}


def config(name):
    return CONFIGS[name] if name in CONFIGS else STEPPING_EXTRA[name]


def padding(cfg):
    return cfg["Nw"] + cfg["ms"] + (8 if cfg.get("kernel") else 0)


def model_name(cfg):
    return "UMPAModelDFKernel" if cfg.get("kernel") else "UMPAModelDF" if cfg["df"] else "UMPAModelNoDF"


def illposed_share(cfg):
    """tests/test_hip_fuzz.py::_illposed_share for this configuration (the function itself, so that the two cannot drift)."""
    from test_hip_fuzz import _illposed_share
    return _illposed_share(dict(df=cfg["df"], K=cfg["K"], Nw=cfg["Nw"]))


_STACKS = {}


def base_stack(name):
    """The scale-1 stack of a configuration, [K, H, W] (sample-stepping frames share a shape, so they stack too)."""
    if name not in _STACKS:
        cfg = config(name)
        seed = cfg["seed"] if "seed" in cfg else 9000 + 37 * sorted(CONFIGS).index(name)
        amp = cfg["ms"] - 2.4                                  # the 4 x 4 gather needs room inside the search box
        if cfg.get("pos"):
            fr = [make_stack(cfg["H"], cfg["W"], 1, cfg["ms"], df=cfg["df"], seed=seed + 17 * k, amplitude=amp, order=1) for k in range(cfg["K"])]
            sam, ref = np.stack([f[0][0] for f in fr]), np.stack([f[1][0] for f in fr])
        else:
            sam, ref, _ = make_stack(cfg["H"], cfg["W"], cfg["K"], cfg["ms"], df=cfg["df"], seed=seed, amplitude=amp, order=1)
        _STACKS[name] = (np.ascontiguousarray(sam), np.ascontiguousarray(ref))
    return _STACKS[name]


def mask_of(name):
    cfg = config(name)
    kind = cfg.get("mask")
    if kind is None:
        return None
    rng = np.random.default_rng(4106 if kind == "binary" else 4107)           # "tiny" is the "weights" mask itself, times 2^-24
    shape = (cfg["K"], cfg["H"], cfg["W"])
    if kind == "binary":
        return (rng.random(shape) < 0.93).astype(np.float64)
    w = rng.uniform(0.2, 1.0, size=shape) * (rng.random(shape) < 0.95)        # non-binary, of order 1, 5 % zeros
    return np.ldexp(w, -24) if kind == "tiny" else w                           # ... times 2^-24: the pair weight's 1e-8 carries weight


def regime_stack(name, regime):
    sam, ref = base_stack(name)
    if regime in (None, "x1"):
        return sam, ref
    return REGIMES[regime](sam, ref, CONFIGS[name])


def frame_order(K):
    return np.roll(np.arange(K), 1)[::-1].copy()


def build(ns, name, sam, ref, mask="cfg", subpx=-1, debug=True, permute=False):
    """The model of configuration `name` on the stacks, with the model classes of `ns`.  The stacks may also be lists of
    frames (device tensors: the model then borrows them)."""
    cfg = config(name)
    if isinstance(mask, str):
        mask = mask_of(name)
    pos = cfg.get("pos")
    if permute:                                                   # a fixed frame permutation: the summation order changes, nothing else
        order = frame_order(cfg["K"])
        sam, ref = np.ascontiguousarray(sam[order]), np.ascontiguousarray(ref[order])
        mask = None if mask is None else np.ascontiguousarray(mask[order])
        pos = None if pos is None else [pos[k] for k in order]
    kw = dict(window_size=cfg["Nw"], max_shift=cfg["ms"])
    if mask is not None:
        kw["mask_list"] = mask
    if pos:
        kw["pos_list"] = [np.array(p) for p in pos]
        if isinstance(sam, np.ndarray):
            sam, ref = [np.ascontiguousarray(f) for f in sam], [np.ascontiguousarray(f) for f in ref]
        if isinstance(mask, np.ndarray):
            kw["mask_list"] = [np.ascontiguousarray(f) for f in mask]
    m = getattr(ns, model_name(cfg))(sam, ref, **kw)
    m.debug = debug
    m.assign_coordinates = cfg["assign"]
    m.sub_pixel_mode = subpx
    if m._lib.is_hip:
        m._force = cfg["force"]
    return m


def kernel_abc(sh):
    """The (a, b, c) maps of the kernel dark-field configuration for a region of shape `sh`"""
    abc = np.zeros(tuple(sh) + (3,))
    abc[..., 0], abc[..., 1], abc[..., 2] = 0.6, 0.1, 0.5
    abc[..., 0] += np.linspace(0, 0.2, sh[1])[None, :]
    return abc


def match(m, name, mk=None, timing=False, path="cfg"):
    """One match of a model of build() with the configuration's arguments (or `mk`); `path`: what last_path must say
    (default: the configuration's, None: not checked)."""
    cfg = config(name)
    mk = dict(cfg.get("mk", {}) if mk is None else mk, quiet=True)
    if cfg.get("kernel"):
        s0, s1 = m._convert_ROI_slice(None, mk.get("step"))
        mk["abc"] = kernel_abc(m._counts(s0, s1))
    if timing:
        m._lib.timing_enable(m._handle, 1)
    out = m.match(**mk)
    out["window"] = m.window
    if timing:                                                    # which kernels the match launched, and how often
        import ctypes
        m._lib.timing_enable(m._handle, 0)
        m.launch_counts = {}
        for q in range(m._lib.timing_collect(m._handle)):
            nm, tot, cnt = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_int()
            m._lib.timing_read(m._handle, q, ctypes.byref(nm), ctypes.byref(tot), ctypes.byref(cnt))
            m.launch_counts[nm.value.decode()] = cnt.value
        m.launched = set(m.launch_counts)
    if m._lib.is_hip and path is not None:
        want = cfg["path"] if path == "cfg" else path
        assert m._lib.last_path(m._handle) == want, "%s ran on path %d, not %d" % (name, m._lib.last_path(m._handle), want)
    return out


def run(ns, name, sam, ref, mask="cfg", subpx=-1, debug=True, mk=None, permute=False, timing=False):
    """Match configuration `name` on the stacks with the model classes of `ns`; returns (result, model).  The forced
    path and last_path only exist on the HIP side."""
    m = build(ns, name, sam, ref, mask=mask, subpx=subpx, debug=debug, permute=permute)
    return match(m, name, mk=mk, timing=timing), m


def label(name, regime):
    return "regime %s %s" % (name, regime)


# Cases the reference cannot be held to its own bar on (test_regimes_cpu.py pins each as a failure of the oracle
# against itself under a frame permutation): they are not in the GPU parity sweep.  Filled from the CPU module's findings.
INADMISSIBLE = {
    ("tiled_DF", "vis1e-3"),            # 5x5 windows, dark-field: df moves by 1.6e-5 under the permutation
}
# ... and visibility 1e-4, which is in no sweep: beyond fp64 for the dark-field configurations listed (march_DF, with its 13x13
# windows, and every configuration without dark-field still agree with themselves there)
BEYOND_FP64 = [(n, "vis1e-4") for n in ("tiled_DF", "tiled_DF10", "masked_bin_DF", "masked_w_DF", "masked_tiny_DF",
                                       "staged_DF", "plain_DF", "stepping_DF", "dfkernel")]


def sweep_cases():
    return [(n, r) for n in CONFIGS for r in SWEEP_REGIMES if (n, r) not in INADMISSIBLE]


# ----------------------------------------------------------------------------- 3. costs against extended precision

HP_REGIMES = ["x1", "x2^16", "vis1e-2", "vis1e-3"]
HP_MAX_CELLS = 10000


def against_hp(name, results, sam, ref, mask="cfg", cost_fn=None):
    """A SAMPLE of the known cells of a sub_pixel_mode-0 result's 5x5 memo against oracle/hp_cost.py, in units of the a-priori fp64
    bound, and the final T / df maps against the extended-precision fits (every cell of every pixel of a lattice, see below).  `results`: tag -> result; the cells are those of the
    FIRST result, the others are read where they know the same cell.  `cost_fn(i, j, si, sj) -> cost` (the oracle's single
    evaluation) is judged on exactly those cells as well, under the tag "ref".  Where the image has more than HP_MAX_CELLS
    known cells the pixels of a lattice are taken (stride 3, 5 or 7: coprime to the tile size, so every column of a tile and
    both sides of every seam are met)."""
    from oracle import hp_cost
    cfg = CONFIGS[name]
    assert not cfg.get("pos") and not cfg.get("kernel")
    if isinstance(mask, str):
        mask = mask_of(name)
    step = cfg.get("mk", {}).get("step", 1)
    first = next(iter(results.values()))
    (xi, xj, q), (pi, pj), (si, sj) = hp_cost.memo_cells(first, padding(cfg), step=step)
    lattice = next((s for s in (1, 3, 5, 7) if q.size / (s * s) <= HP_MAX_CELLS), 7)
    sel = (xi % lattice == 0) & (xj % lattice == 0)
    xi, xj, q, pi, pj, si, sj = (v[sel] for v in (xi, xj, q, pi, pj, si, sj))
    hp = hp_cost.hp_cells(1 if cfg["df"] else 0, sam, ref, np.asarray(first["window"]), pi, pj, si, sj, cfg["assign"], mask)
    out = {}
    px = xi * first["err"].shape[1] + xj
    for tag, res in results.items():
        d = res["debug_d"][xi, xj, q].astype(np.longdouble)
        same = (d >= 0) & (res["err"][xi, xj] == 1) & (np.rint(res["dy"][xi, xj]) == np.rint(first["dy"][xi, xj])) & \
               (np.rint(res["dx"][xi, xj]) == np.rint(first["dx"][xi, xj]))
        err = np.abs(d - hp["cost"])[same]
        st = dict(lattice=lattice, cells=int(same.sum()), ratio=float((err / hp["bound"][same]).max()),
                  rel=float((err / np.abs(hp["cost"][same])).max()))
        # (at visibility 1e-2 and below the fits of neighbouring shifts differ by less than 1e-5, so there the choice of cell
        #  decides nothing: the figure then measures the fit's accuracy, not which cell it came from)
        # the maps carry the fit the walk KEPT: the minimum's, except where the reference keeps a stale one on purpose (a tie on
        # both sides, a restart of the gather: Optim.cpp:373,386) -- always the fit of a cell of this memo.  So: the nearest cell's.
        for k in ("T", "df") if cfg["df"] else ("T",):
            e = np.where(same, np.abs(res[k][xi, xj] - hp[k]) / np.abs(hp[k]), np.inf)
            best = np.full(first["err"].size, np.inf)
            np.minimum.at(best, px, e.astype(np.float64))
            best = best[np.unique(px[same])]
            st[k + "_rel"] = float(best.max())
        out[tag] = st
    if cost_fn is not None:
        c = np.array([cost_fn(int(a), int(b), int(u), int(v)) for a, b, u, v in zip(pi, pj, si, sj)]).astype(np.longdouble)
        out["ref"] = dict(cells=int(q.size), ratio=float((np.abs(c - hp["cost"]) / hp["bound"]).max()))
    out["_cells"] = (pi, pj, si, sj, hp)
    return out
