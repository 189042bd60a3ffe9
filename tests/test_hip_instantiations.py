"""
Every compiled kernel instantiation of libumpa_hip.so, launched and held to the CPU oracle.

The library's kernels are templates: the frame count, the window half-width, the search range, the model kind, the mask
and the on-demand state pick one of several hundred instantiations (tools/kernel_coverage.py lists them).  A bug that
lives in one of them -- an unroll count, the odd / even frame-pair layout, a register budget, an LDS layout -- shows
nowhere else.  Each case here is small, is compared with the `port` oracle to the full bar (conftest.assert_parity),
asserts the route it takes with what the library reports (`last_path`, the kernel families of `timing_read`,
`last_stats`), and declares in `reaches` the kernels it is there for, by their full demangled `name<args>`.
tests/test_kernel_coverage.py checks on the CPU that every symbol of the built library is claimed by one of them, by a
named test elsewhere, or by a listed exclusion.
"""
import ctypes
import functools

import numpy as np
import pytest

from conftest import assert_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip_ns():
    from umpa_amd import _lib, model
    if _lib.hip().device_count() < 1:
        pytest.fail("no HIP device: the GPU tests cannot run (there is no CPU fallback)")
    return model


# ----------------------------------------------------------------------------- helpers

@functools.lru_cache(maxsize=None)
def _stack(H, W, K, ms, df, seed, amp):
    from umpa_amd.synth import make_stack
    sam, ref, _ = make_stack(H, W, K, ms, df=df, seed=seed, amplitude=amp, order=1)
    return sam, ref


@functools.lru_cache(maxsize=None)
def _mask(shape, seed, keep=0.93):
    return (np.random.default_rng(seed).random(shape) < keep).astype(np.float64)


def _kind(df):
    return "UMPAModelDF" if df else "UMPAModelNoDF"


def _families(m):
    lib, h = m._lib, m._handle
    out = {}
    for q in range(lib.timing_collect(h)):
        nm, tot, cnt = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_int()
        lib.timing_read(h, q, ctypes.byref(nm), ctypes.byref(tot), ctypes.byref(cnt))
        out[nm.value.decode()] = out.get(nm.value.decode(), 0) + cnt.value
    return out


def _stats(m):
    st = (ctypes.c_double * 4)()
    m._lib.check(m._lib.last_stats(m._handle, st), "last_stats")
    return list(st)


def _hip_match(ns, name, sam, ref, Nw, ms, assign="sam", mask=None, force=0, mk=None, env=None, monkeypatch=None):
    """One match on the GPU: (maps, last_path, {kernel family: launches}, last_stats)."""
    for k, v in (env or {}).items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    m = getattr(ns, name)(sam, ref, mask_list=mask, window_size=Nw, max_shift=ms)
    m.assign_coordinates = assign
    m.debug = True
    m._force = force
    m._lib.timing_enable(m._handle, 1)
    got = m.match(quiet=True, **(mk or {}))
    fam = _families(m)
    m._lib.timing_enable(m._handle, 0)
    return got, m._lib.last_path(m._handle), fam, _stats(m)


def _oracle(port_ns, name, sam, ref, Nw, ms, assign="sam", mask=None, mk=None):
    o = getattr(port_ns, name)(sam, ref, mask_list=mask, window_size=Nw, max_shift=ms)
    o.assign_coordinates = assign
    o.debug = True
    return o.match(quiet=True, **(mk or {}))


def _same(a, b, label):
    assert sorted(a) == sorted(b), label
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), "%s: %s differs" % (label, k)


def _nwc(Nw):
    return Nw if 1 <= Nw <= 8 else 0


def _assert_on_demand(family, fam_od, fam_all, st, label):
    """The on-demand run took the on-demand route: more launches of the table kernel than the exhaustive run's one per
    chunk (seed tiles, then the queue twin over the work list) -- else the bit-for-bit comparison with the exhaustive run
    would compare two static runs.  (Whether passes are left out depends on the field: on these small images with
    +-2 .. 7 shifts the walks' 4 x 4 gathers often read every pass, and the queue twin then computes all of them.)"""
    assert fam_od.get(family, 0) > fam_all.get(family, 0), (label, fam_od, fam_all)
    assert 0 < st[0] <= st[1], (label, st)


# ----------------------------------------------------------------------------- 1. DF tiled path, K = 1 .. 26

def _replay_id(K):
    return {11: "K11-last-speculative", 12: "K12-first-plain"}.get(K, "K%d" % K)


REPLAY_CASES = [pytest.param(True, K, id=_replay_id(K)) for K in range(1, 27)] + \
               [pytest.param(False, K, id="nodf-K%d" % K) for K in (3, 9)]


def _replay_reaches(df, K):
    if not df:
        return ["replay_walk_kernel<0, 0, false>", "replay_walk_kernel<0, 0, true>", "prep_maps_kernel<0, 2>"]
    na = K if K <= 24 else 0
    return ["replay_walk_kernel<1, %d, false>" % na, "replay_walk_kernel<1, %d, true>" % na, "prep_maps_kernel<1, 2>"]


@pytest.mark.parametrize("df,K", REPLAY_CASES)
def test_replay_walk_per_frame_count(hip_ns, port_ns, monkeypatch, df, K):
    """replay_walk is instantiated per frame count up to 24 (frame-pair maps, unrolled loops; NA 11 is the last one with the
    speculative second lookup), generic beyond.  Both coordinate modes ('ref' reads the MR planes as fixed maps), the
    exhaustive table against the oracle, on-demand passes against the exhaustive run bit for bit."""
    Nw, ms = 2, 3
    sam, ref = _stack(80, 110, K, ms, df, 61, 1.5)                 # 70 x 100 outputs: 3 x 4 table tiles, many replay blocks
    name = _kind(df)
    for assign in ("sam", "ref"):
        label = "replay %s K%d %s" % (name, K, assign)
        got, path, fam, st = _hip_match(hip_ns, name, sam, ref, Nw, ms, assign, env={"UMPA_HIP_ONDEMAND": "0"}, monkeypatch=monkeypatch)
        assert path == 2 and fam.get("replay_walk", 0) >= 1 and fam.get("corr_volume", 0) >= 1, (path, fam)
        assert st[0] == st[1] and st[2] == 0, st
        assert_parity(got, _oracle(port_ns, name, sam, ref, Nw, ms, assign), ms, label)
        od, path, fam_od, st = _hip_match(hip_ns, name, sam, ref, Nw, ms, assign, env={"UMPA_HIP_ONDEMAND": "1"}, monkeypatch=monkeypatch)
        assert path == 2
        _assert_on_demand("corr_volume", fam_od, fam, st, label)
        _same(od, got, label + " on-demand")


# ----------------------------------------------------------------------------- 2. corr_volume: every shape per (Nw, UB)

# launch_corr_shape's workgroup shapes (umpa_tiled.h, UMPA_CORR_SHAPES): id -> (TC, NTG, UI, WPC, NF, RO).  A forced id that
# is not compiled for (Nw, UB) runs the fallback, shape 4.  tests/test_kernel_coverage.py checks this table, the fallback and
# CORR_UB_CANDIDATES against the source, so a new shape id fails there until a case here launches it.
CORR_SHAPES = {1: (32, 256, 1, 2, 2, 1), 2: (24, 256, 1, 2, 2, 1), 3: (16, 256, 1, 2, 1, 1), 4: (32, 512, 1, 1, 2, 1),
               5: (32, 512, 1, 1, 9, 3), 6: (24, 512, 1, 1, 9, 3)}
CORR_FALLBACK = 4
CORR_UB_CANDIDATES = (9, 8, 7, 5)            # pick_ub's cand[]
CORR_MS = (3, 4, 8, 5)                       # 2 ms - 1 = 5, 7, 15, 9: UB 5 / 7 / 8 / 9 (pick_ub; clamped to what fits)
CORR_CASES = [pytest.param(Nw, ms, id="Nw%d-ms%d" % (Nw, ms)) for Nw in range(1, 9) for ms in CORR_MS]


def _ub(Nw, ms):
    """pick_ub (umpa_tiled.h): fewest column batches, then least padding, over CORR_UB_CANDIDATES in that order."""
    UJ = 2 * ms - 1
    best, key = 5, None
    for ub in CORR_UB_CANDIDATES:
        k = ((UJ + ub - 1) // ub, (UJ + ub - 1) // ub * ub - UJ)
        if key is None or k < key:
            best, key = ub, k
    return best


def corr_tail(Nw, ub, shape):
    """corr_volume's template arguments for a shape id (the three-row shapes take NF = UB: one flush round per column offset)."""
    TC, NTG, UI, WPC, NF, RO = CORR_SHAPES[shape]
    return "<%d, %d, %d, %d, %d, %d, %d, %d>" % (Nw, ub, TC, NTG, UI, WPC, ub if RO > 1 else NF, RO)


def _corr_reaches(Nw, ms):
    return ["prep_maps_kernel<%d, %d>" % (1 if ms in (3, 8) else 0, Nw)]


def _corr_reaches_where_compiled(Nw, ms):
    # the kernel each forced shape id launches, both twins, where that shape is compiled for (Nw, UB); UB as picked --
    # launch_corr_nw lowers it where it does not fit, and then the fallback's name, which always exists, would be missing
    ub = _ub(Nw, ms)
    return ["corr_volume%s_kernel%s" % (q, corr_tail(Nw, ub, shape)) for shape in CORR_SHAPES for q in ("", "_queue")]


@pytest.mark.parametrize("Nw,ms", CORR_CASES)
def test_corr_volume_every_shape(hip_ns, port_ns, monkeypatch, Nw, ms):
    """Each workgroup shape the code object holds for this (Nw, UB), forced through UMPA_HIP_CORR_SHAPE, with on-demand
    passes (the queue twin) and without; everything against one oracle result."""
    df = ms in (3, 8)                                                # both kinds over the table: prep_maps<KIND, NW>
    K = 10 if Nw <= 2 else 4                                         # narrow windows: enough frames for a well-posed fit
    pad = Nw + ms
    sam, ref = _stack(66 + 2 * pad, 70 + 2 * pad, K, ms, df, 70 + Nw, min(1.5, ms - 1.5))
    name = _kind(df)
    want = _oracle(port_ns, name, sam, ref, Nw, ms)
    env = {"UMPA_HIP_MARCH": "0"}
    for shape in CORR_SHAPES:
        env["UMPA_HIP_CORR_SHAPE"] = str(shape)
        runs, fams = {}, {}
        for od in ("0", "1"):
            env["UMPA_HIP_ONDEMAND"] = od
            got, path, fams[od], st = _hip_match(hip_ns, name, sam, ref, Nw, ms, env=env, monkeypatch=monkeypatch)
            assert path == 2 and fams[od].get("corr_volume", 0) >= 1 and "corr_march" not in fams[od], (path, fams[od])
            if od == "0":
                assert st[0] == st[1] and st[2] == 0, st
            else:
                _assert_on_demand("corr_volume", fams["1"], fams["0"], st, "Nw%d ms%d shape %d" % (Nw, ms, shape))
            runs[od] = got
        assert_parity(runs["0"], want, ms, "corr_volume Nw%d ms%d shape %d" % (Nw, ms, shape))
        _same(runs["1"], runs["0"], "corr_volume Nw%d ms%d shape %d on-demand" % (Nw, ms, shape))


AUTO_CASES = [pytest.param(Nw, ms, K, id="Nw%d-ms%d-K%d" % (Nw, ms, K)) for Nw in (2, 7) for ms in (3, 4, 5) for K in (5, 8)]


@pytest.mark.parametrize("Nw,ms,K", AUTO_CASES)
def test_corr_volume_automatic_shape(hip_ns, port_ns, monkeypatch, Nw, ms, K):
    """The automatic choice: one row offset per pass below 7 frames, three from 7 on; (2 ms - 1) mod 3 = 2, 1, 0 for ms 3, 4, 5
    leaves a third of the three-row shape's last pass idle, or not."""
    pad = Nw + ms
    sam, ref = _stack(50 + 2 * pad, 75 + 2 * pad, K, ms, True, 90 + K, min(1.5, ms - 1.5))
    got, path, fam, _ = _hip_match(hip_ns, "UMPAModelDF", sam, ref, Nw, ms,
                                   env={"UMPA_HIP_MARCH": "0", "UMPA_HIP_CORR_SHAPE": None, "UMPA_HIP_ONDEMAND": None},
                                   monkeypatch=monkeypatch)
    assert path == 2 and fam.get("corr_volume", 0) >= 1, (path, fam)
    assert_parity(got, _oracle(port_ns, "UMPAModelDF", sam, ref, Nw, ms), ms, "corr auto Nw%d ms%d K%d" % (Nw, ms, K))


# ----------------------------------------------------------------------------- 3. corr_march: NXB 8, the largest plan, the frame limit

MARCH_CASES = [
    pytest.param(6, 10, 4, True, id="Nw6-ms10-nxb8"),
    pytest.param(7, 10, 4, True, id="Nw7-ms10-nxb8"),
    pytest.param(7, 17, 3, True, id="Nw7-ms17-largest"),
    pytest.param(6, 17, 3, False, id="Nw6-ms17-largest-nodf"),
    pytest.param(6, 9, 42, True, id="Nw6-ms9-K42-last"),
    pytest.param(6, 9, 43, True, id="Nw6-ms9-K43-volume"),
    pytest.param(7, 10, 38, True, id="Nw7-ms10-K38-last"),
    pytest.param(7, 10, 39, True, id="Nw7-ms10-K39-volume"),
]
MARCH_REACHES = ["corr_march_kernel<6, 8, 4, 2, 768, 3, 1>", "corr_march_kernel<7, 8, 4, 2, 768, 3, 1>",
                 "corr_march_kernel<6, 4, 4, 2, 768, 3, 1>", "prep_maps_kernel<0, 6>"]


@pytest.mark.parametrize("Nw,ms,K,df", MARCH_CASES)
def test_corr_march_plans(hip_ns, port_ns, monkeypatch, Nw, ms, K, df):
    """corr_march (windows 13 / 15) with 8 column blocks (max_shift >= 10), the largest search range the tiled path takes, and
    the staging limit (42 frames at 4 column blocks, 38 at 8): one frame more and corr_volume takes the table.  Against the
    oracle and against corr_volume (UMPA_HIP_MARCH=0): the same walks, the maps to rounding."""
    march = (K <= 42) if ms <= 9 else (K <= 38)
    pad = Nw + ms
    H, W = (40, 48) if K > 8 else (60, 80)
    sam, ref = _stack(H + 2 * pad, W + 2 * pad, K, ms, df, 110 + K, min(3.0, ms - 1.5))
    name = _kind(df)
    env = {"UMPA_HIP_CORR_SHAPE": None, "UMPA_HIP_ONDEMAND": None, "UMPA_HIP_MARCH": None}
    got, path, fam, _ = _hip_match(hip_ns, name, sam, ref, Nw, ms, env=env, monkeypatch=monkeypatch)
    assert path == 2 and ("corr_march" in fam) == march and ("corr_volume" in fam) == (not march), fam
    st = assert_parity(got, _oracle(port_ns, name, sam, ref, Nw, ms), ms, "march Nw%d ms%d K%d" % (Nw, ms, K))
    assert st["ok"] > 200
    if march:
        env["UMPA_HIP_MARCH"] = "0"
        vol, path, fam, _ = _hip_match(hip_ns, name, sam, ref, Nw, ms, env=env, monkeypatch=monkeypatch)
        assert "corr_volume" in fam and "corr_march" not in fam, fam
        for k in ("err", "debug_Ncalls"):
            np.testing.assert_array_equal(got[k], vol[k], err_msg=k)
        ok = vol["err"] == 1
        np.testing.assert_allclose(got["T"][ok], vol["T"][ok], rtol=1e-9)


def test_corr_march_ignores_the_on_demand_switch(hip_ns, monkeypatch):
    """corr_march always computes its whole table: UMPA_HIP_ONDEMAND unset, 0 and 1 give the same maps bit for bit, launch the
    same kernels the same number of times, and last_stats reports the exhaustive table, nothing parked, no tile missed."""
    Nw, ms, K = 6, 5, 4
    pad = Nw + ms
    sam, ref = _stack(60 + 2 * pad, 80 + 2 * pad, K, ms, True, 117, 3.0)
    runs = {}
    for od in (None, "0", "1"):
        env = {"UMPA_HIP_CORR_SHAPE": None, "UMPA_HIP_MARCH": None, "UMPA_HIP_ONDEMAND": od}
        got, path, fam, st = _hip_match(hip_ns, "UMPAModelDF", sam, ref, Nw, ms, env=env, monkeypatch=monkeypatch)
        assert path == 2 and fam.get("corr_march", 0) >= 1 and fam.get("replay_walk", 0) >= 1 and "corr_volume" not in fam, (od, path, fam)
        assert st[1] > 0 and st[0] == st[1] and st[2] == 0 and st[3] == 0, (od, st)
        runs[od] = (got, fam)
    for od in ("0", "1"):
        _same(runs[od][0], runs[None][0], "UMPA_HIP_ONDEMAND=%s against unset" % od)
        assert runs[od][1] == runs[None][1], (od, runs[od][1], runs[None][1])


# ----------------------------------------------------------------------------- 4. the search-range edge of the tiled path

@pytest.mark.parametrize("ms", [17, 18])
def test_search_range_edge(hip_ns, port_ns, monkeypatch, ms):
    """(2 ms - 1)^2 <= 1089 keeps max_shift 17 on the tiled path (four column batches of 9); 18 goes to the general kernels."""
    Nw, K = 3, 3
    pad = Nw + ms
    sam, ref = _stack(50 + 2 * pad, 70 + 2 * pad, K, ms, True, 130, 3.0)
    got, path, fam, _ = _hip_match(hip_ns, "UMPAModelDF", sam, ref, Nw, ms,
                                   env={"UMPA_HIP_CORR_SHAPE": None, "UMPA_HIP_ONDEMAND": None}, monkeypatch=monkeypatch)
    if ms == 17:
        assert path == 2 and "corr_volume" in fam, (path, fam)
    else:
        assert path in (1, 3) and "corr_volume" not in fam, (path, fam)
    assert_parity(got, _oracle(port_ns, "UMPAModelDF", sam, ref, Nw, ms), ms, "search edge ms%d" % ms)


# ----------------------------------------------------------------------------- 5. the masked tiled path

MASKED_CASES = [pytest.param(df, Nw, id="%s-Nw%d" % ("df" if df else "nodf", Nw)) for df in (True, False) for Nw in range(1, 9)]


def masked_ub(kind, Nw):
    """masked_ub (umpa_tiled.h): corr_masked's column offsets per pass; checked against the source by test_kernel_coverage."""
    return (3 if Nw <= 6 else 2) if kind == 1 else (5 if Nw <= 6 else 3)


def _masked_reaches(df, Nw):
    k = 1 if df else 0
    tail = "<%d, %d, %d, 32>" % (k, Nw, masked_ub(k, Nw))
    return ["corr_masked_kernel" + tail, "corr_masked_queue_kernel" + tail, "replay_cost_kernel<%d>" % k]


@pytest.mark.parametrize("df,Nw", MASKED_CASES)
def test_masked_tiled_path(hip_ns, port_ns, monkeypatch, df, Nw):
    """corr_masked + replay_cost per kind and window, with on-demand passes (the queue twin) and without."""
    ms = 3
    K = 10 if Nw <= 2 else 3                                         # K (2 Nw + 1)^2 > 9: not the exact-fit rule's general kernel
    pad = Nw + ms
    sam, ref = _stack(70 + 2 * pad, 100 + 2 * pad, K, ms, df, 150 + Nw, 1.2)
    mask = _mask(sam.shape, Nw)
    name = _kind(df)
    runs, fams = {}, {}
    for od in ("0", "1"):
        got, path, fams[od], st = _hip_match(hip_ns, name, sam, ref, Nw, ms, mask=mask,
                                             env={"UMPA_HIP_ONDEMAND": od}, monkeypatch=monkeypatch)
        assert path == 2 and fams[od].get("corr_masked", 0) >= 1 and fams[od].get("replay_cost", 0) >= 1, (path, fams[od])
        if od == "0":
            assert st[0] == st[1] and st[2] == 0, st
        else:
            _assert_on_demand("corr_masked", fams["1"], fams["0"], st, "masked %s Nw%d" % (name, Nw))
        runs[od] = got
    assert_parity(runs["0"], _oracle(port_ns, name, sam, ref, Nw, ms, mask=mask), ms, "masked tiled %s Nw%d" % (name, Nw))
    _same(runs["1"], runs["0"], "masked tiled %s Nw%d on-demand" % (name, Nw))


# ----------------------------------------------------------------------------- 6. the general kernels

# (no dark-field model at Nw 0: a one-pixel window is its own mean, the dark-field term has nothing to fit and the walks follow
# rounding noise; the generic instantiation runs for it at Nw 10)
GENERAL_NW = list(range(0, 9)) + [10]
GENERAL_CASES = [pytest.param(df, masked, Nw, id="%s-%s-Nw%d" % ("df" if df else "nodf", "mask" if masked else "plain", Nw))
                 for df in (True, False) for masked in (False, True) for Nw in GENERAL_NW if Nw or not df]


def _general_reaches(df, masked, Nw):
    k = 1 if df else 0
    out = ["match_direct_kernel<%d, %s, %d>" % (k, "true" if masked else "false", _nwc(Nw))]
    if not masked:
        out.append("match_staged_kernel<%d, false, %d>" % (k, _nwc(Nw)))
    return out


@pytest.mark.parametrize("df,masked,Nw", GENERAL_CASES)
def test_general_kernels(hip_ns, port_ns, monkeypatch, df, masked, Nw):
    """match_direct (windows through L1) and match_staged (windows out of LDS; unmasked models only) per kind, mask and
    window, the generic NWC = 0 instantiation at Nw 0 and at a window wider than 17."""
    from umpa_amd import _lib
    ms = 3
    K = 6 if Nw == 0 else 10 if Nw <= 2 else 3
    pad = Nw + ms
    sam, ref = _stack(24 + 2 * pad, 40 + 2 * pad, K, ms, df, 170 + Nw, 1.2)
    mask = _mask(sam.shape, 40 + Nw) if masked else None
    name = _kind(df)
    want = _oracle(port_ns, name, sam, ref, Nw, ms, mask=mask)
    for force, paths in ((_lib.F_FORCE_DIRECT, (1,) if masked else (3,)), (_lib.F_FORCE_DIRECT | _lib.F_FORCE_PLAIN_DIRECT, (1,))):
        got, path, fam, _ = _hip_match(hip_ns, name, sam, ref, Nw, ms, mask=mask, force=force, monkeypatch=monkeypatch)
        assert path in paths, (force, path, fam)
        assert ("match_staged" if path == 3 else "match_direct") in fam, fam
        assert_parity(got, want, ms, "general %s mask=%s Nw%d force %d" % (name, masked, Nw, force))


@pytest.mark.parametrize("df", [True, False])
def test_masked_single_pixel_cost(hip_ns, port_ns, df):
    """cost_one_kernel<KIND, true>: the single-pixel cost() of a masked model."""
    sam, ref = _stack(60, 70, 3, 4, df, 190, 1.5)
    mask = _mask(sam.shape, 191, keep=0.8)
    name = _kind(df)
    g = getattr(hip_ns, name)(sam, ref, mask_list=mask, window_size=2, max_shift=4)
    o = getattr(port_ns, name)(sam, ref, mask_list=mask, window_size=2, max_shift=4)
    for assign in ("sam", "ref"):
        g.assign_coordinates = o.assign_coordinates = assign
        for (i, j) in [(6, 6), (20, 33), (40, 50), (31, 8)]:
            for (sx, sy) in [(0, 0), (1, -2), (-3, 3), (2.4, -0.6)]:
                np.testing.assert_allclose(g.cost(i, j, sx, sy), o.cost(i, j, sx, sy), rtol=1e-10)


# ----------------------------------------------------------------------------- 7. the kernel-dark-field model

DFK_NW = list(range(0, 9)) + [10]
DFK_CASES = [pytest.param(Nw, masked, id="Nw%d-%s" % (Nw, "mask" if masked else "plain")) for Nw in DFK_NW for masked in (False, True)]


def _dfk(ns, sam, ref, Nw, ms, mask, assign):
    m = ns.UMPAModelDFKernel(sam, ref, mask_list=mask, window_size=Nw, max_shift=ms)
    m.assign_coordinates = assign
    m.debug = True
    return m


def _dfk_match(ns, sam, ref, Nw, ms, mask, assign, mk, abc_vals=(0.15, 0.0, 0.1), ramp=False):
    m = _dfk(ns, sam, ref, Nw, ms, mask, assign)
    s0, s1 = m._convert_ROI_slice(mk.get("ROI"), mk.get("step"))
    sh = (1 + (s0[1] - s0[0] - 1) // s0[2], 1 + (s1[1] - s1[0] - 1) // s1[2])
    abc = np.zeros(sh + (3,))
    abc[..., 0], abc[..., 1], abc[..., 2] = abc_vals
    if ramp:
        abc[..., 0] += np.linspace(0, 0.2, sh[1])[None, :]
        abc[..., 2] += np.linspace(0, 0.05, sh[0])[:, None]
    fam = None
    if hasattr(m._lib, "timing_enable") and m._lib.is_hip:
        m._lib.timing_enable(m._handle, 1)
        got = m.match(abc=abc, quiet=True, **mk)
        fam = _families(m)
        m._lib.timing_enable(m._handle, 0)
        assert m._lib.last_path(m._handle) == 1
    else:
        got = m.match(abc=abc, quiet=True, **mk)
    return got, fam


@pytest.mark.parametrize("Nw,masked", DFK_CASES)
def test_dfkernel_windows(hip_ns, port_ns, Nw, masked):
    """match_direct_kernel<2, MASK, NWC> per window in both coordinate modes ('ref': the blur halo is Nw, not
    Nw + max_shift - 1); a few dozen pixels at wide windows (the oracle blurs 289 taps per footprint pixel)."""
    ms = 3
    K = 5 if Nw == 0 else 3
    pad = Nw + ms + 8
    sam, ref = _stack(12 + 2 * pad, 16 + 2 * pad, K, ms, True, 210 + Nw, 1.2)
    mask = _mask(sam.shape, 60 + Nw) if masked else None
    mk = dict(ROI=((2, 10, 1), (1, 15, 2)))                          # 8 x 7 pixels
    for assign in ("sam", "ref"):
        got, fam = _dfk_match(hip_ns, sam, ref, Nw, ms, mask, assign, mk)
        want, _ = _dfk_match(port_ns, sam, ref, Nw, ms, mask, assign, mk)
        assert "match_direct" in fam, fam
        assert_parity(got, want, ms, "dfkernel Nw%d mask=%s %s" % (Nw, masked, assign))


DFK_BLUR_CASES = [
    pytest.param(True, "sam", dict(), ("blur_tiles_kernel<true>",), id="mask-step1-blur_tiles"),
    pytest.param(True, "ref", dict(step=2, dxdy=(1, -1)), ("blur_tiles_kernel<true>",), id="mask-ref-step2-dxdy"),
    pytest.param(False, "sam", dict(), ("blur_tiles_kernel<false>",), id="plain-step1-blur_tiles"),
    pytest.param(False, "sam", dict(step=4), (), id="plain-step4-per-lane-fill"),
    pytest.param(False, "ref", dict(ROI=((3, 30, 1), (4, 40, 3))), ("blur_tiles_kernel<false>",), id="plain-ref-roi"),
]


@pytest.mark.parametrize("masked,assign,mk,reaches", DFK_BLUR_CASES)
def test_dfkernel_blur_staging(hip_ns, port_ns, masked, assign, mk, reaches):
    """Where a box's reference patch fits half the LDS budget blur_tiles stages it (step 1, with and without mask); an
    unmasked step-4 region does not fit and every lane fills its own footprint.  A per-pixel varying abc throughout."""
    Nw, ms, K = 2, 4, 3
    pad = Nw + ms + 8
    sam, ref = _stack(36 + 2 * pad, 48 + 2 * pad, K, ms, True, 230, 1.5)
    mask = _mask(sam.shape, 231) if masked else None
    got, fam = _dfk_match(hip_ns, sam, ref, Nw, ms, mask, assign, mk, ramp=True)
    want, _ = _dfk_match(port_ns, sam, ref, Nw, ms, mask, assign, mk, ramp=True)
    assert ("blur_tiles" in fam) == bool(reaches), fam
    assert_parity(got, want, ms, "dfkernel blur mask=%s %s %s" % (masked, assign, mk))


# ----------------------------------------------------------------------------- 8. stage_sample: raw dtypes and flat correction

STAGE_CASES = [pytest.param(dt, corr, id="%s-%s" % (dt, "darkflat" if corr else "raw"))
               for dt in ("float64", "float32", "uint16") for corr in (True, False)]


@pytest.mark.parametrize("dtype,corrected", STAGE_CASES)
def test_stage_sample_dtypes(hip_ns, dtype, corrected):
    """stage_sample uploads a raw stack (float64 / float32 / uint16), flat_correct_kernel forms (raw - dark) / flat on the
    device, the next match adopts it (F_USE_STAGED): bit for bit a match of a model built from numpy's (raw - dark) / flat."""
    import torch
    Nw, ms, K = 3, 4, 4
    sam, ref = _stack(80, 96, K, ms, True, 250, 1.5)
    rng = np.random.default_rng(251)
    if corrected:
        dark = 100.0 + rng.uniform(0, 2, size=sam.shape)
        flat = 20000.0 * (1.0 + 0.05 * rng.standard_normal(sam.shape))
        raw = sam * flat + dark
    else:
        dark = flat = None
        raw = sam * (1000.0 if dtype == "uint16" else 1.0)
    raw = np.rint(raw).astype(np.uint16) if dtype == "uint16" else raw.astype(dtype)
    raw = np.ascontiguousarray(raw)
    x = raw.astype(np.float64)
    if corrected:
        x = (x - dark) / flat
    m = hip_ns.UMPAModelDF(ref.copy(), ref, window_size=Nw, max_shift=ms)
    m.debug = True
    dev = lambda a: [torch.from_numpy(np.ascontiguousarray(f)).to("cuda:0") for f in a]
    m.stage_sample(list(raw), dark=dev(dark) if corrected else None, flat=dev(flat) if corrected else None)
    got = m.match(quiet=True)
    w = hip_ns.UMPAModelDF(np.ascontiguousarray(x), ref, window_size=Nw, max_shift=ms)
    w.debug = True
    want = w.match(quiet=True)
    _same(got, want, "stage_sample %s corrected=%s" % (dtype, corrected))
    assert (want["err"] == 1).sum() > 1000


# ----------------------------------------------------------------------------- what the cases are there for

def _all_reaches():
    r = {}
    for p in REPLAY_CASES:
        r["test_replay_walk_per_frame_count[%s]" % p.id] = _replay_reaches(*p.values)
    for p in CORR_CASES:
        r["test_corr_volume_every_shape[%s]" % p.id] = _corr_reaches(*p.values)
    r["test_corr_march_plans"] = MARCH_REACHES
    for p in MASKED_CASES:
        r["test_masked_tiled_path[%s]" % p.id] = _masked_reaches(*p.values)
    for p in GENERAL_CASES:
        r["test_general_kernels[%s]" % p.id] = _general_reaches(*p.values)
    r["test_masked_single_pixel_cost"] = ["cost_one_kernel<0, true>", "cost_one_kernel<1, true>"]
    for p in DFK_CASES:
        Nw, masked = p.values
        r["test_dfkernel_windows[%s]" % p.id] = ["match_direct_kernel<2, %s, %d>" % ("true" if masked else "false", _nwc(Nw))]
    for p in DFK_BLUR_CASES:
        if p.values[3]:
            r["test_dfkernel_blur_staging[%s]" % p.id] = list(p.values[3])
    r["test_stage_sample_dtypes"] = ["flat_correct_kernel<double>", "flat_correct_kernel<float>",
                                     "flat_correct_kernel<unsigned short>"]
    return r


REACHES = _all_reaches()
# names that a case launches only where the instantiation is compiled (forcing a shape id that is not falls back to shape 4)
REACHES_WHERE_COMPILED = {"test_corr_volume_every_shape[%s]" % p.id: _corr_reaches_where_compiled(*p.values) for p in CORR_CASES}
