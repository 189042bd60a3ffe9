"""
Every matching path of the HIP library on the input regimes of tests/regimes.py (GPU box only): other scales -- up to
detector counts, down to where the walk's absolute tie tolerance decides --, low speckle contrast on a large mean,
negative values, and NaN / Inf / 0 pixels.  tests/test_regimes_cpu.py shows that each sweep case is one the oracle can
be held to (it meets the bar against itself under a frame permutation) and that the tie-rule factors are in the regime.

 a. parity with the oracle to the full bar (conftest.assert_parity) on every admissible (path, regime) pair;
 b. exact covariance: 2^16 (sam, ref) and 2^7 sam give the scale-1 maps bit for bit, f and the memo times the power of two;
 c. on-demand table passes change nothing at other scales either;
 d. a bad pixel changes nothing further than Nw + max_shift away, bit for bit, and every walk in reach still ends;
 e. the costs of a SAMPLE of the 5x5 memos (every known cell of the pixels of a lattice of stride 3 to 7, coprime to the tile
    and strip sizes, 4 to 11 % of the cells: R.HP_MAX_CELLS keeps the longdouble work on the host short) against an
    extended-precision evaluation (oracle/hp_cost.py) in units of the a-priori fp64 bound: at most M_FACTOR times what the
    oracle itself is away from it on the same cells, and never past the bound.

In reach of a bad pixel (d): a 0 is finite data and the whole image is held to the oracle at the full bar; around NaN / Inf the
kernels are held to the oracle on the pixels where the in-place build of the reference was recorded to agree with it
(tests/golden/bad_pixel_agreement.npz: the 51 cases with the bad pixel in the stack whose window stays at the pixel -- there
every cost of a touched pixel is NaN and the walk ends at once; in the other 51, the bad pixel in the stack whose window moves
with the shift, the reference never returns and there is nothing to hold the kernels to but the properties).

M_FACTOR is twice the largest r_gpu / r_ref observed on an MI355X (tests/golden/regime_observed.json, written by a run with
UMPA_RECORD_REGIMES=<output directory>; the factor 2 because the maximum of a rounding-error sample moves with the seed), per
family of paths: the general kernels sum in or close to the oracle's order (0.93 .. 1.04, M_FACTOR 2.07); the table paths'
filtered sums are MORE accurate than the reference's running sums (0.13 .. 0.41, M_FACTOR 0.83).  The constants stand in this
module and test_m_factor_is_twice_the_recorded_ratio ties them to the recorded file.  r_ref itself is 0.012 .. 0.03 with
dark-field and 0.05 .. 0.09 without, at every scale and visibility.  Largest relative error of T / df against the
extended-precision fit: 3e-9 / 1e-8 (visibility 1e-3), the oracle's own 1e-9 / 2e-8.

The module takes about 25 s on an MI355X host against 1 s for tests/test_hip_fuzz.py on images of the same size: half of it is
the start of torch in the flat-correction case, most of the rest the oracle runs and the longdouble sums on the CPU; the
kernels themselves take well under a second.
"""
import ctypes
import json
import os

import numpy as np
import pytest

import regimes as R
from conftest import GOLDEN, assert_parity

pytestmark = pytest.mark.gpu

MAPS = ("err", "debug_Ncalls", "f", "T", "dx", "dy", "df", "debug_d", "debug_a")
_OBSERVED_PATH = os.path.join(GOLDEN, "regime_observed.json")
RECORD = bool(os.environ.get("UMPA_RECORD_REGIMES"))
_seen = {}


@pytest.fixture(scope="module")
def ns():
    from umpa_amd import _lib, model
    from oracle import cpu_model
    if _lib.hip().device_count() < 1:
        pytest.fail("no HIP device: the GPU tests cannot run (there is no CPU fallback)")
    yield model, cpu_model.port
    if RECORD and _seen:
        out = os.environ["UMPA_RECORD_REGIMES"]                       # the directory to write into
        os.makedirs(out, exist_ok=True)
        worst = max(v["r_gpu"] / v["r_ref"] for v in _seen.values())
        json.dump(dict(max_r_gpu_over_r_ref=worst, cases=_seen), open(os.path.join(out, "regime_observed.json"), "w"), indent=1, sort_keys=True)


def _same(a, b, sel=None, what=""):
    for k in MAPS:
        if k in a:
            x, y = (a[k], b[k]) if sel is None else (a[k][sel], b[k][sel])
            assert np.array_equal(x, y, equal_nan=True), "%s: %s differs on %d entries" % (what, k, int((~((x == y) | (np.isnan(x) & np.isnan(y)))).sum()))


_BASE = {}


def _base(ns, name):
    """The scale-1 match of a configuration on the GPU and on the oracle (once per module run)."""
    if name not in _BASE:
        sam, ref = R.base_stack(name)
        got, g = R.run(ns[0], name, sam, ref, timing=True)
        want, _ = R.run(ns[1], name, sam, ref)
        _BASE[name] = (got, want, g.launched)
    return _BASE[name]


# ----------------------------------------------------------------------------- a. parity sweep

SWEEP = R.sweep_cases()


@pytest.mark.parametrize("name,regime", SWEEP, ids=["%s-%s" % c for c in SWEEP])
def test_regime_parity(ns, name, regime):
    cfg = R.CONFIGS[name]
    sam, ref = R.regime_stack(name, regime)
    got, _ = R.run(ns[0], name, sam, ref)
    want, _ = R.run(ns[1], name, sam, ref)
    st = assert_parity(got, want, cfg["ms"], R.label(name, regime))
    assert st["ok"] > 500
    if regime.startswith("tie"):                                    # the case demonstrably exercises the rule
        base = _base(ns, name)[0]
        changed = (got["debug_Ncalls"] != base["debug_Ncalls"]).mean()
        print("%s: %.1f %% of the walks differ from scale 1" % (R.label(name, regime), 100 * changed))
        assert changed >= 0.05


# ----------------------------------------------------------------------------- b. exact covariance

def _scaled_maps(base, e2):
    """What a result must be bit for bit when every cost is 2^e2 times the base's."""
    want = dict(base)
    want["f"] = np.ldexp(base["f"], e2)
    want["debug_d"] = np.where(base["debug_d"] >= 0, np.ldexp(base["debug_d"], e2), base["debug_d"])    # unknown cells stay -1
    want["debug_a"] = np.ldexp(base["debug_a"], e2)
    return want


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_power_of_two_scales_change_no_bit(ns, name):
    """Every operation on the result paths is a multiply, an add, an fma, a division or fast_rcp (hardware seed and Newton
    steps), and all of them commute with powers of two: an absolute constant anywhere on such a path shows here.  Also the
    scale-1 parity of the configuration, and that the match launched the kernel the configuration is named after."""
    cfg = R.CONFIGS[name]
    base, want, launched = _base(ns, name)
    assert cfg.get("launch") is None or cfg["launch"] in launched, launched
    st = assert_parity(base, want, cfg["ms"], R.label(name, "x1"))
    assert st["ok"] > 500
    sam, ref = R.base_stack(name)
    got, _ = R.run(ns[0], name, *R.scaled(sam, ref, 16, 16))
    _same(got, _scaled_maps(base, 32), what="2^16 (sam, ref)")
    got, _ = R.run(ns[0], name, *R.scaled(sam, ref, 7, 0))
    exp = _scaled_maps(base, 14)
    exp["T"] = base["T"] * 128.0
    _same(got, exp, what="2^7 sam")


# ----------------------------------------------------------------------------- c. on-demand passes

# (the shapes of test_on_demand_table_passes_change_nothing, where units are left out and walks are parked at scale 1)
# ("masked": with that test's mask -- the scheme is on by default for models with masks)
OD_CFG = {"volume": dict(H=420, W=520, K=4, Nw=3, ms=6, amp=4.5), "masked": dict(H=330, W=400, K=4, Nw=4, ms=5, amp=3.5, mask=True)}
OD_REGIMES = {"x2^16": lambda s, r: R.scaled(s, r, 16, 16), "tie": lambda s, r: R.tie_scaled(s, r, -9, 1.0),
              "vis1e-2": lambda s, r: R.counts(s, r, 40000, 1e-2)}


@pytest.mark.parametrize("regime", list(OD_REGIMES))
@pytest.mark.parametrize("kernel", list(OD_CFG))
def test_on_demand_passes_change_nothing_at_other_scales(ns, monkeypatch, kernel, regime):
    """test_on_demand_table_passes_change_nothing on other inputs: the walks, and with them the seed tiles' predictions and the
    parked pixels, change with the scale; the maps must still be the exhaustive table's bit for bit."""
    from umpa_amd import _lib
    from umpa_amd.synth import make_stack
    c = OD_CFG[kernel]
    sam, ref, _ = make_stack(c["H"], c["W"], c["K"], c["ms"], df=True, seed=31, amplitude=c["amp"], order=1)
    sam, ref = OD_REGIMES[regime](sam, ref)
    mask = (np.random.default_rng(2).random(sam.shape) < 0.93).astype(np.float64) if c.get("mask") else None
    out, stats = {}, {}
    for od in ("0", "1"):
        monkeypatch.setenv("UMPA_HIP_ONDEMAND", od)
        m = ns[0].UMPAModelDF(sam, ref, mask_list=mask, window_size=c["Nw"], max_shift=c["ms"])
        m._force = _lib.F_FORCE_TILED
        out[od] = m.match(quiet=True)
        assert m._lib.last_path(m._handle) == 2
        st = (ctypes.c_double * 4)()
        m._lib.check(m._lib.last_stats(m._handle, st), "last_stats")
        stats[od] = list(st)
    _same(out["0"], out["1"], what="on-demand %s %s" % (kernel, regime))
    assert (out["0"]["err"] == 1).mean() > 0.05
    assert stats["0"][0] == stats["0"][1] and stats["0"][2] == 0          # exhaustive: every unit, nothing parked
    assert 0 < stats["1"][0] <= stats["1"][1] and stats["1"][2] > 0, stats  # on demand: walks were parked and run again


# ----------------------------------------------------------------------------- d. bad pixels

BAD = [(n, k, w) for n in R.CONFIGS for k in R.BAD_VALUES for w in ("sam", "ref")]
AGREEMENT = np.load(os.path.join(GOLDEN, "bad_pixel_agreement.npz"))


def _contained(cfg, clean, dirty, pos, what):
    far = R.far_from(cfg, pos, clean["err"].shape)
    assert (~far).sum() < 0.1 * far.size, "the bad pixels reach %d of %d output pixels" % ((~far).sum(), far.size)
    _same(clean, dirty, far, what)
    assert set(np.unique(dirty["err"])) <= {0, 1} and dirty["debug_Ncalls"].max() <= R.NCALLS_MAX and dirty["debug_Ncalls"].min() >= 0
    return far


@pytest.mark.parametrize("name,kind,where", BAD, ids=["%s-%s-%s" % c for c in BAD])
def test_bad_pixels_stay_local(ns, name, kind, where):
    """NaN / +Inf / -Inf / 0 in the interior, on a tile or strip seam, inside the padding border and in the last frame: every
    output pixel out of reach is bit-identical to the clean run in every map (so one 0 * NaN in a filter stage, a halo, a
    lead-in row or a padded lane would show), and with that at the clean run's parity with the oracle.  In reach: a 0 is
    finite data, so the whole image is held to the oracle on the damaged stack at the full bar; around a non-finite pixel the
    kernels are held to the oracle where the two CPU checkers were recorded to agree (tests/golden/bad_pixel_agreement.npz --
    the in-place reference build does not return from every such stack, and what it answers is its compiler's treatment of
    NaN), and everywhere to what is specified: err is 0 or 1, the walk ends."""
    cfg = R.CONFIGS[name]
    sam, ref = R.base_stack(name)
    pos = R.bad_positions(cfg)
    clean = _base(ns, name)[0]
    bad = R.bad_pixels(sam, ref, kind, where, pos)
    dirty, _ = R.run(ns[0], name, *bad)
    far = _contained(cfg, clean, dirty, pos, "%s %s in %s" % (name, kind, where))
    want, _ = R.run(ns[1], name, *bad)
    if kind == "zero":
        st = assert_parity(dirty, want, cfg["ms"], R.label(name, "zero_" + where))
        assert st["ok"] > 500
        return
    assert not np.array_equal(clean["T"][~far], dirty["T"][~far], equal_nan=True)          # ... and in reach it does show
    key = R.bad_key(name, kind, where)
    if key in AGREEMENT.files:
        agree = np.unpackbits(AGREEMENT[key])[:far.size].reshape(far.shape).astype(bool)
        sel = agree & ~far
        for k in ("err", "debug_Ncalls"):
            assert np.array_equal(dirty[k][sel], want[k][sel]), "%s: %s differs from the oracle where both CPU checkers agree" % (key, k)
        for k in ("T", "df"):
            if k in want:
                a, b = dirty[k][sel], want[k][sel]
                with np.errstate(invalid="ignore"):
                    same = (np.abs(a - b) <= 1e-5 * np.abs(b)) | (np.isnan(a) & np.isnan(b)) | (a == b)
                assert same.all(), "%s: %s differs from the oracle on %d pixels where both CPU checkers agree" % (key, k, (~same).sum())
        print("%s: held to the oracle on %d of %d pixels in reach" % (key, sel.sum(), (~far).sum()))
    else:
        assert key in AGREEMENT["hangs"], key + " is missing from tests/golden/bad_pixel_agreement.npz"


@pytest.mark.parametrize("what", ["nan_under_zero_mask", "zero_mask"])
@pytest.mark.parametrize("name", [n for n in R.CONFIGS if R.CONFIGS[n].get("mask")])
def test_bad_pixels_and_masks(ns, name, what):
    """The same positions with a mask value of 0: an ordinary bad-pixel mask on clean data, and a NaN under it (which the
    mask does not hide: 0 * NaN, reference behaviour pinned in test_regimes_cpu.py) -- far pixels untouched either way."""
    cfg = R.CONFIGS[name]
    sam, ref = R.base_stack(name)
    pos = R.bad_positions(cfg)
    mask = R.mask_of(name).copy()
    for (k, r, c) in pos:
        mask[k, r, c] = 0.0
    masked, _ = R.run(ns[0], name, sam, ref, mask=mask)
    if what == "zero_mask":
        _contained(cfg, _base(ns, name)[0], masked, pos, name + " zero mask")
        want, _ = R.run(ns[1], name, sam, ref, mask=mask)
        assert_parity(masked, want, cfg["ms"], R.label(name, "zero_mask"))
    else:
        dirty, _ = R.run(ns[0], name, *R.bad_pixels(sam, ref, "nan", "sam", pos), mask=mask)
        _contained(cfg, masked, dirty, pos, name + " NaN under a zero mask")


def test_flat_correction_of_dead_pixels(ns):
    """uint16 raw frames through flat_correct_kernel with dead pixels: flat == 0 where raw == dark (0 / 0 = NaN) and flat == 0
    alone (x / 0 = Inf).  The match on the staged stack is bit for bit the match on numpy's (raw - dark) / flat, NaN and
    Inf positions included, and obeys the containment property against the same stack without dead pixels."""
    import torch
    name = "tiled_DF10"
    cfg = R.CONFIGS[name]
    sam, ref = R.base_stack(name)
    rng = np.random.default_rng(251)
    dark = np.rint(100.0 + rng.uniform(0, 2, size=sam.shape))
    flat = 20000.0 * (1.0 + 0.05 * rng.standard_normal(sam.shape))
    raw = np.ascontiguousarray(np.rint(sam * flat + dark).astype(np.uint16))
    pos = R.bad_positions(cfg)
    flat_bad = flat.copy()
    for n, (k, r, c) in enumerate(pos):
        flat_bad[k, r, c] = 0.0
        if n % 2 == 0:
            raw[k, r, c] = dark[k, r, c]                                # 0 / 0
    with np.errstate(divide="ignore", invalid="ignore"):
        x_bad = (raw.astype(np.float64) - dark) / flat_bad
    x_clean = (raw.astype(np.float64) - dark) / flat
    assert np.isnan(x_bad).sum() == (len(pos) + 1) // 2 and np.isinf(x_bad).sum() == len(pos) // 2
    dev = lambda a: [torch.from_numpy(np.ascontiguousarray(f)).to("cuda:0") for f in a]
    from umpa_amd import _lib
    m = ns[0].UMPAModelDF(ref.copy(), ref, window_size=cfg["Nw"], max_shift=cfg["ms"])
    m.assign_coordinates = cfg["assign"]
    m._force = _lib.F_FORCE_TILED
    m.stage_sample(list(raw), dark=dev(dark), flat=dev(flat_bad))
    got = m.match(quiet=True)
    assert m._lib.last_path(m._handle) == 2
    want, _ = R.run(ns[0], name, np.ascontiguousarray(x_bad), ref)
    _same(got, want, what="staged dead pixels")
    clean, _ = R.run(ns[0], name, np.ascontiguousarray(x_clean), ref)
    _contained(cfg, clean, got, pos, "staged dead pixels")


# ----------------------------------------------------------------------------- e. costs against extended precision

HP_CASES = [(n, r) for n in R.CONFIGS if R.CONFIGS[n].get("table") or n.startswith(("staged", "plain")) for r in R.HP_REGIMES]
OBSERVED = json.load(open(_OBSERVED_PATH))
# twice the largest r_gpu / r_ref of the recorded run, per family: the table paths (cost from expanded, filtered sums: corr_volume,
# corr_march, corr_masked + the lookup) and the general kernels (window sums in or close to the oracle's order)
M_FACTOR = {"table": 0.83, "general": 2.07}


@pytest.mark.parametrize("name,regime", HP_CASES, ids=["%s-%s" % c for c in HP_CASES])
def test_costs_against_extended_precision(ns, name, regime):
    """|gpu - hp| <= min(1, M_FACTOR r_ref) bound on every known cell of the memo (sub_pixel_mode 0), r_ref being the oracle's
    own max |oracle - hp| / bound on the very same cells.  T and df of the maps and of single cost() calls within 1e-5 of
    the extended-precision fit.  Not restricted to admissible cases: this asks for accuracy, not for agreement."""
    cfg = R.CONFIGS[name]
    sam, ref = R.regime_stack(name, regime)
    got, g = R.run(ns[0], name, sam, ref, subpx=0)
    o = getattr(ns[1], R.model_name(cfg))(sam, ref, mask_list=R.mask_of(name), window_size=cfg["Nw"], max_shift=cfg["ms"])
    o.assign_coordinates = cfg["assign"]
    st = R.against_hp(name, {"gpu": got}, sam, ref, cost_fn=lambda i, j, a, b: o.cost(i, j, a, b)[0])
    r_gpu, r_ref = st["gpu"]["ratio"], st["ref"]["ratio"]
    print("%s: %d cells (lattice %d)  r_gpu %.4f  r_ref %.4f  ratio %.2f  relative %.1e  T %.1e  df %.1e" % (
        R.label(name, regime), st["gpu"]["cells"], st["gpu"]["lattice"], r_gpu, r_ref, r_gpu / r_ref, st["gpu"]["rel"],
        st["gpu"]["T_rel"], st["gpu"].get("df_rel", 0.0)))
    _seen["%s %s" % (name, regime)] = dict(r_gpu=r_gpu, r_ref=r_ref, rel=st["gpu"]["rel"], T_rel=st["gpu"]["T_rel"], df_rel=st["gpu"].get("df_rel", 0.0))
    assert st["gpu"]["cells"] > 3000 and r_ref < 1.0
    assert r_gpu <= 1.0
    assert st["gpu"]["T_rel"] < 1e-5 and st["gpu"].get("df_rel", 0.0) < 1e-5
    # single evaluations through the C ABI (cost_one_kernel, the general kernel's arithmetic) at 40 of the cells
    pi, pj, si, sj, hp = st["_cells"]
    for q in np.random.default_rng(5).choice(pi.size, 40, replace=False):
        v = g.cost(int(pi[q]), int(pj[q]), float(si[q]), float(sj[q]))
        assert abs(v[0] - hp["cost"][q]) <= hp["bound"][q]
        assert abs(v[1] - hp["T"][q]) <= 1e-5 * abs(hp["T"][q])
        if cfg["df"]:
            assert abs(v[2] - hp["df"][q]) <= 1e-5 * abs(hp["df"][q])
    if not RECORD:
        m_factor = M_FACTOR["table" if cfg.get("table") else "general"]
        assert r_gpu <= min(1.0, m_factor * r_ref), "r_gpu / r_ref = %.2f, above M_FACTOR = %.2f" % (r_gpu / r_ref, m_factor)


def test_m_factor_is_twice_the_recorded_ratio():
    """M_FACTOR is a constant of this module, so that a change of the threshold shows in a diff; it must be what the recorded
    run (tests/golden/regime_observed.json) gives, per family of paths."""
    worst = {"table": 0.0, "general": 0.0}
    for case, v in OBSERVED["cases"].items():
        fam = "table" if R.CONFIGS[case.split()[0]].get("table") else "general"
        worst[fam] = max(worst[fam], v["r_gpu"] / v["r_ref"])
    for fam in worst:
        assert worst[fam] <= 8.0 and abs(M_FACTOR[fam] - 2.0 * worst[fam]) <= 0.006, (fam, worst[fam])
