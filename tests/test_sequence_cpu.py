"""
Sequence search (umpa_grid_sequence, model.sequence, umpa_amd.sequence), what can be checked without a GPU: the restatement
the GPU tests use (tests/sequence_expect.py) against a brute-force loop and against umpa_amd.sequence.restate, the
consequences the header states, the library's build, the refusals that come before any device work, and the host logic of
Sequence.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import REPO

import grid_expect as GE
import sequence_expect as SE
from nativelibs import assert_claimed, build_all as _build, declared, exported, kernel_keys, tool

GRID_LIB = os.path.join(REPO, "umpa_amd", "libumpa_grid.so")
KTEMPL = 24
NAN, INF = float("nan"), float("inf")


# ----------------------------------------------------------------------------- 1. the restatement against the loop

def _random_case(U, N0, N1, seed, special=True):
    """(cost, T, df, prev): random volumes; with `special`, NaN, +Inf and -Inf entries in both, an all-NaN prev pixel, a prev
    pixel that is all +Inf and one whose only finite entry stands alone"""
    rng = np.random.default_rng(seed)
    cost, prev = rng.random((U, U, N0, N1)), 3.0 * rng.random((U, U, N0, N1))
    T, df = 0.5 + rng.random(cost.shape), rng.random(cost.shape)
    if special:
        for a in (cost, prev):
            w = rng.random(a.shape)
            a[w < 0.06] = NAN
            a[(w >= 0.06) & (w < 0.10)] = INF
            a[(w >= 0.10) & (w < 0.11)] = -INF
        prev[:, :, 0, 0] = NAN
        prev[:, :, 0, 1] = INF
        prev[:, :, 1, 0] = NAN
        prev[U // 2, U - 1, 1, 0] = 0.25
        cost[:, :, 1, 1] = NAN                                          # a pixel without any cost
        for a, px in ((cost, (0, 2)), (prev, (1, 2))):                  # one of each kind for certain, in pixels of their own
            a[0, 1][px], a[1, 0][px], a[U - 1, U - 1][px] = -INF, INF, NAN
        assert all(np.isnan(a).any() and (a == INF).any() and (a == -INF).any() for a in (cost, prev))
    return cost, T, df, prev


@pytest.mark.parametrize("U", [3, 5, 9, 15])
def test_restatement_against_the_brute_force_loop_and_the_package(U):
    from umpa_amd.sequence import restate
    N0, N1 = (3, 4) if U < 15 else (2, 3)
    seen = {}
    for special in (False, True):
        cost, T, df, prev = _random_case(U, N0, N1, 40 + U, special)
        for lam in (0.0, 0.013, 0.4):
            for trunc in (0.0, 0.21, INF, None):
                for with_df in (False, True):
                    for subpx in ((-1, 0, 1) if (lam, trunc, special) == (0.013, 0.21, True) else (0,)):
                        d = df if with_df else None
                        a = SE.restate(cost, T, d, prev, lam, trunc, subpx)
                        b = SE.brute(cost, T, d, prev, lam, trunc, subpx)
                        SE.assert_equal(a, b, "U %d lam %g trunc %s special %s subpx %d" % (U, lam, trunc, special, subpx))
                        assert sorted(a) == sorted(["dx", "dy", "f", "T", "cost", "total", "cost0", "shift", "err", "moved", "state"] + (["df"] if with_df else []))
                # the package's restatement: the same state and choice
                r = restate(cost, prev, lam, trunc)
                for n in ("state", "shift", "cost", "total", "cost0", "moved"):
                    np.testing.assert_array_equal(r[n], a[n], err_msg="%s U %d lam %g trunc %s" % (n, U, lam, trunc))
                np.testing.assert_array_equal(r["M"], SE.transition(prev, lam, trunc, cost.shape))
                seen[(special, lam, trunc)] = a
        start = SE.restate(cost, T, df, None, 0.4, 0.21, 0)
        SE.assert_equal(start, SE.brute(cost, T, df, None, 0.4, 0.21, 0), "prev None")
        np.testing.assert_array_equal(restate(cost, None, 0.4, 0.21)["state"], start["state"])
        # the consequences: lam = 0 (a prev without -Inf) and prev = None choose what the data term alone chooses, A = C + 0.0
        if not special:
            with np.errstate(invalid="ignore"):
                for d in (start, seen[(False, 0.0, 0.21)], seen[(False, 0.0, None)], seen[(False, 0.4, 0.0)]):
                    np.testing.assert_array_equal(d["state"], cost + 0.0)
                    np.testing.assert_array_equal(d["cost"], d["cost0"])
                    np.testing.assert_array_equal(d["total"], d["cost"])
                    assert (d["moved"] == 0).all()
            # a weight that matters: somewhere the series overrules the data term, and total is cost plus a transition >= 0
            mid = seen[(False, 0.013, INF)]
            assert (mid["moved"] == 1).any() and (mid["moved"] == 0).any()
            assert (mid["total"] >= mid["cost"]).all() and (mid["cost"] >= mid["cost0"]).all()
            assert ((mid["cost"] > mid["cost0"]) == (mid["moved"] == 1)).all()
    # special pixels: an all-NaN and an all-Inf prev pixel have M = 0; a pixel without costs has zeros and a NaN state
    sp = seen[(True, 0.013, 0.21)]
    cost, T, df, prev = _random_case(U, N0, N1, 40 + U, True)
    with np.errstate(invalid="ignore"):
        for px in ((0, 0), (0, 1)):
            np.testing.assert_array_equal(sp["state"][(slice(None), slice(None)) + px], cost[(slice(None), slice(None)) + px] + 0.0)
    assert np.isnan(sp["state"][:, :, 1, 1]).all() and sp["err"][1, 1] == 0 and sp["moved"][1, 1] == 0
    assert all(sp[n][1, 1] == 0 for n in ("dx", "dy", "f", "T", "cost", "total", "cost0")) and (sp["shift"][:, 1, 1] == 0).all()
    # trunc = 0: M = 0 wherever prev has a finite minimum
    z = seen[(True, 0.4, 0.0)]
    m0 = np.where(prev < INF, prev, INF).reshape(U * U, N0, N1).min(axis=0)
    fin = np.isfinite(m0)
    assert fin.any()
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(z["state"][:, :, fin], (cost + 0.0)[:, :, fin])


def test_on_an_oracle_volume_lam_0_and_no_state_are_the_grid_search():
    """The extended-precision volumes of the grid tests, rounded: with lam = 0 or without a state the maps are those of the grid
    search's restatement (tests/grid_expect.py states them for the global minimum; tests/basins_expect.py's rank 0 is it)."""
    import basins_expect as BE
    sam, ref, c = GE.stack("64x72x3")
    v = GE.hp_volumes(1, sam, ref, GE.window(c["Nw"]), c["ms"], c["ms"] + c["Nw"], "sam")
    r = {k: np.ascontiguousarray(np.asarray(v[k], dtype=np.float64)[:, :, ::3, ::4]) for k in ("cost", "T", "df")}
    rng = np.random.default_rng(8)
    prev = rng.random(r["cost"].shape)
    for subpx in (0, -1):
        b = BE.restate(r["cost"], r["T"], r["df"], 1, subpx)
        for what, args in (("lam 0", (prev, 0.0, 0.3)), ("no state", (None, 0.2, None))):
            s = SE.restate(r["cost"], r["T"], r["df"], *args, subpx)
            for n in ("dx", "dy", "f", "T", "df", "cost"):
                np.testing.assert_array_equal(s[n], b[n][0], err_msg="%s %s" % (what, n))
            np.testing.assert_array_equal(s["shift"], b["shift"][0])
            np.testing.assert_array_equal(s["err"], np.maximum(b["err"][0], 0))
            assert (s["moved"] == 0).all() and (s["cost"] == s["cost0"]).all()
    # and a weight on the scale of the volume moves some pixels away from the data term's choice
    scale = float(np.median(r["cost"]))
    s = SE.restate(r["cost"], r["T"], r["df"], 5.0 * scale * prev, 0.2 * scale, None, 0)
    assert (s["moved"] == 1).any() and (s["moved"] == 0).any()


# ----------------------------------------------------------------------------- 2. the library

def test_grid_library_exports_sequence_and_its_kernels_are_claimed():
    g = _build()
    from umpa_amd import _lib
    assert len(g.LIBRARIES) == 8                                      # a sixth consumer in libumpa_grid.so, not a ninth library
    assert "umpa_grid_sequence" in declared("umpa_grid.h", "umpa_grid_") and "sequence" in _lib.GRID_SYMBOLS
    assert declared("umpa_grid.h", "umpa_grid_") == sorted("umpa_grid_" + s for s in _lib.GRID_SYMBOLS)
    assert "umpa_grid_sequence" in exported(GRID_LIB)
    assert sorted(n for n in exported(GRID_LIB) if n.startswith("umpa")) == declared("umpa_grid.h", "umpa_grid_")
    assert hasattr(_lib.grid(), "sequence")
    hdr = open(os.path.join(REPO, "include", "umpa_grid.h")).read()
    assert "#define UMPA_GRID_SEQUENCE_MAX_SHIFT 8" in hdr and (_lib.GRID_SEQUENCE_MIN_MS, _lib.GRID_SEQUENCE_MAX_MS) == (2, 8)
    keys = kernel_keys(GRID_LIB)
    syms = [k for k in keys if k.split("<", 1)[0] == "grid_sequence_kernel" or k.startswith("sequence_")]
    want = ["grid_sequence_kernel<1, %d>" % n for n in range(KTEMPL + 1)] + ["grid_sequence_kernel<0, 0>"]
    assert sorted(syms) == sorted(want) and len(syms) == 26, sorted(set(syms) ^ set(want))
    assert_claimed(syms, "sequence")
    assert sum("grid_sequence_kernel<" in s for s in tool("kernel_coverage").kernel_symbols(GRID_LIB)) == 26
    # the sibling families keep their counts
    family = lambda f: [k for k in keys if k.split("<", 1)[0] == f]
    assert len(family("grid_track_kernel")) == 26 and len(family("grid_basins_kernel")) == 26
    assert len(family("grid_min_kernel")) == 26 and len(family("cost_volume_kernel")) == 26
    assert sum(k.startswith("widen_") for k in keys) == 33
    import levels_expect as LE
    assert sorted(k for k in keys if k.startswith("levels_")) == sorted(LE.KERNELS)
    # the main library: no new public symbol, none of the new kernels
    public = sorted(n for n in exported(g.HIP_LIB) if n.startswith("umpa_hip_"))
    assert public == sorted("umpa_hip_" + s for s in _lib.HIP_SYMBOLS)
    assert not [k for k in kernel_keys(g.HIP_LIB) if "sequence" in k]


def test_the_ctypes_row_is_the_header_s_signature():
    from umpa_amd import _lib
    restype, args = _lib._GRID_ABI["sequence"]
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    # model | start0 step0 N0 start1 step1 N1 | prev lam trunc next | f T dx dy cost df | si sj err | total cost0 moved | flags stream
    assert restype is i and args == [vp] + [i] * 6 + [vp, d, d, vp] + [vp] * 6 + [vp] * 3 + [vp] * 3 + [i, vp]
    hdr = open(os.path.join(REPO, "include", "umpa_grid.h")).read()
    proto = hdr[hdr.index("int umpa_grid_sequence("):]
    proto = proto[:proto.index(";")]
    params = [p.strip() for p in proto[proto.index("(") + 1:proto.rindex(")")].split(",")]
    kinds = [vp if "*" in p else d if p.startswith("double") else i for p in params]
    assert kinds == args and len(params) == 25
    assert [p.split()[-1].lstrip("*") for p in params[7:11]] == ["prev", "lam", "trunc", "next"]
    assert [p.split()[-1].lstrip("*") for p in params[11:23]] == ["f", "T", "dx", "dy", "cost", "df", "si", "sj", "err", "total", "cost0", "moved"]


E_ARG = -1
MODEL_TEXT = "grid: sequence: null model"
PLANE_TEXT = "grid: sequence: null output plane (only df and next may be NULL)"
LAM_TEXT = "grid: sequence: lam must be finite and not negative, not %s"
TRUNC_TEXT = "grid: sequence: trunc must be >= 0 or +Inf, not %s"
FLAGS_TEXT = "grid: sequence takes UMPA_HIP_F_DEVICE_IO, UMPA_HIP_F_USE_STAGED and no other flag, not 0x%x"


def test_c_abi_refusals_come_before_any_device_work():
    """No device, no model: a pointer that is never followed stands for one.  Every refusal has its code and its full text,
    which names the value; of two faults the first in the header's order (model, output planes, lam, trunc, flags) is the
    one reported."""
    _build()
    from umpa_amd import _lib
    g = _lib.grid()
    fake = ctypes.create_string_buffer(64)
    # the output planes in the order of the arguments: f T dx dy cost df | si sj err | total cost0 | moved
    bufs = [np.zeros(8) for _ in range(6)] + [np.zeros(8, np.int32) for _ in range(3)] + [np.zeros(8), np.zeros(8), np.zeros(8, np.int32)]
    state = np.zeros(9 * 8)

    def call(model=ctypes.addressof(fake), prev=None, lam=0.0, trunc=INF, nxt=None, flags=0, drop=None):
        ptrs = [None if q == drop else a.ctypes.data for q, a in enumerate(bufs)]
        return g.sequence(model, 0, 1, 1, 0, 1, 1, prev, lam, trunc, nxt, *ptrs, flags, None), g.error()

    fmt = lambda v: "%g" % v                                           # (as printf's %g writes these values)
    assert call(model=None) == (E_ARG, MODEL_TEXT)
    for q in range(12):
        if q != 5:                                                    # every plane but df is needed
            assert call(drop=q) == (E_ARG, PLANE_TEXT), q
    for lam in (-1.0, -1e-300, INF, -INF):
        assert call(lam=lam) == (E_ARG, LAM_TEXT % fmt(lam)), lam
    rc, text = call(lam=NAN)
    assert rc == E_ARG and text in (LAM_TEXT % "nan", LAM_TEXT % "-nan")
    for trunc in (-1.0, -1e-300, -INF):
        assert call(trunc=trunc) == (E_ARG, TRUNC_TEXT % fmt(trunc)), trunc
    rc, text = call(trunc=NAN)
    assert rc == E_ARG and text in (TRUNC_TEXT % "nan", TRUNC_TEXT % "-nan")
    for flags in (_lib.F_FORCE_DIRECT, _lib.F_FORCE_TILED, _lib.F_PLANAR, _lib.F_REUSE_REF_MAPS, _lib.F_ASYNC, _lib.F_FORCE_PLAIN_DIRECT,
                  _lib.F_DEVICE_IO | _lib.F_PLANAR, _lib.F_USE_STAGED | _lib.F_ASYNC, 256):
        assert call(flags=flags) == (E_ARG, FLAGS_TEXT % flags), flags
        assert call(prev=state.ctypes.data, nxt=state.ctypes.data, trunc=0.0, flags=flags) == (E_ARG, FLAGS_TEXT % flags), flags
    # double refusals: the header's order
    assert call(model=None, drop=0, lam=-1.0) == (E_ARG, MODEL_TEXT)
    assert call(drop=11, lam=-1.0, flags=_lib.F_PLANAR) == (E_ARG, PLANE_TEXT)
    assert call(lam=-2.0, trunc=-1.0) == (E_ARG, LAM_TEXT % "-2")
    assert call(trunc=-1.0, flags=_lib.F_PLANAR) == (E_ARG, TRUNC_TEXT % "-1")
    assert all((a == 0).all() for a in bufs) and (state == 0).all()


# ----------------------------------------------------------------------------- 3. the Python layer

class _HipLib:
    is_hip = True


class _CpuLib:
    is_hip = False


def _stub(cls, **kw):
    """a model object that has what the checks in front of the native call read, and no device: 28 x 36 pixels, max_shift 3"""
    from umpa_amd import model
    m = object.__new__(getattr(model, cls))
    m._lib, m._mask, m._force, m._device = _HipLib(), None, 0, 0
    m._pos_list, m._shape_list, m._padding, m._max_shift = [(0, 0)] * 3, [(40, 48)] * 3, 6, 3
    m._ROI = ((0, 28, 1), (0, 36, 1))
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def test_python_refusals():
    import torch
    from umpa_amd import _lib, model
    tail = " (grid search / cost volume): "
    for cls in ("UMPAModelDF", "UMPAModelNoDF"):
        cases = [(dict(_mask=np.ones((3, 40, 48))), "masked models are not supported (their table holds finished costs)"),
                 (dict(_pos_list=[(0, 0), (2, 1), (1, 3)]), "frames at different positions (pos_list) or of different shapes are not supported"),
                 (dict(_shape_list=[(40, 48), (40, 48), (40, 50)]), "frames at different positions (pos_list) or of different shapes are not supported"),
                 (dict(_force=_lib.F_FORCE_DIRECT), "the model is forced onto the direct kernel"),
                 (dict(_lib=_CpuLib()), "it runs on the HIP library only")]
        for kw, why in cases:
            for args in (dict(lam=0.1), dict(lam=-1.0), dict(lam=0.1, state=np.zeros((2, 2))), dict(lam=0.1, step=2)):   # the model's refusal comes first
                with pytest.raises(RuntimeError) as e:
                    _stub(cls, **kw).sequence(**args)
                assert str(e.value) == "sequence" + tail + why
        for ms in (1, 9, 17):
            for args in (dict(lam=0.1), dict(lam=-1.0)):                # the search range comes before the weights
                with pytest.raises(RuntimeError) as e:
                    _stub(cls, _max_shift=ms).sequence(**args)
                assert str(e.value) == "sequence: max_shift must be 2 to 8, not %d" % ms
        for lam in (None, -1.0, -1e-300, INF, NAN, "1", True, [1.0], 1j):
            with pytest.raises(ValueError) as e:
                _stub(cls).sequence(lam=lam)
            assert str(e.value) == "sequence: lam must be a finite number >= 0, not %r" % (lam,)
        for trunc in (-1.0, NAN, "2", False, (1.0,)):
            with pytest.raises(ValueError) as e:
                _stub(cls).sequence(lam=0.1, trunc=trunc)
            assert str(e.value) == "sequence: trunc must be None (no truncation) or a number >= 0, not %r" % (trunc,)
            with pytest.raises(ValueError, match="sequence: lam must be a finite number"):   # lam's refusal comes first
                _stub(cls).sequence(lam=-2.0, trunc=trunc)
        # state and out shapes, against the region asked for (U = 5)
        for shape, region in (((5, 5, 28, 35), {}), ((5, 28, 36), {}), ((3, 3, 28, 36), {}), ((5, 5, 28, 36), dict(step=2)),
                              ((5, 5, 14, 18), dict(ROI=((0, 28, 2), (0, 30, 2))))):
            want = (5, 5, 14, 15) if "ROI" in region else (5, 5, 14, 18) if region else (5, 5, 28, 36)
            with pytest.raises(ValueError) as e:
                _stub(cls).sequence(state=np.zeros(shape), lam=0.1, **region)
            assert str(e.value) == "sequence: state must be of shape %s, not %s" % (want, shape)
            with pytest.raises(ValueError) as e:
                _stub(cls).sequence(state=np.zeros(want), lam=0.1, out=np.zeros(shape), **region)
            assert str(e.value) == "sequence: out must be of shape %s, not %s" % (want, shape)
        with pytest.raises(ValueError) as e:
            _stub(cls).sequence(state=np.zeros((5, 5, 28, 36), dtype=complex), lam=0.1)
        assert str(e.value) == "sequence: state must be of a real number type, not complex128"
        with pytest.raises(ValueError) as e:
            _stub(cls).sequence(lam=0.1, out=np.zeros((5, 5, 28, 36), dtype=np.float32))
        assert str(e.value) == "sequence: a host out must be a C-contiguous float64 numpy array"
        a = np.zeros((5, 5, 28, 36))
        with pytest.raises(ValueError) as e:
            _stub(cls).sequence(state=a, lam=0.1, out=a)
        assert str(e.value) == "sequence: out must not be the state itself (the call reads the one while it writes the other)"
        # sides: a tensor beside a numpy array; a tensor that is not a float64 HIP tensor on the model's device
        t = torch.zeros((5, 5, 28, 36), dtype=torch.float64)
        for args in (dict(state=t, out=np.zeros((5, 5, 28, 36))), dict(state=np.zeros((5, 5, 28, 36)), out=t)):
            with pytest.raises(ValueError) as e:
                _stub(cls).sequence(lam=0.1, **args)
            assert str(e.value) == "sequence: state and out must be both numpy arrays or both HIP tensors"
        for args in (dict(state=t), dict(state=t.float())):
            with pytest.raises(ValueError) as e:
                _stub(cls).sequence(lam=0.1, **args)
            assert str(e.value) == "sequence: a device state must be a contiguous float64 HIP tensor on the model's device"
    assert not hasattr(model.UMPAModelDFKernel, "sequence")
    with pytest.raises(RuntimeError) as e:
        _stub("UMPAModelDFKernel")._grid_check("sequence")
    assert str(e.value) == "sequence" + tail + "the kernel dark-field model has no shift table"


class _FakeModel:
    """what Sequence touches of a model; its 'device' is the host, its states are the tensors it is handed"""
    _device = "cpu"
    sh = (2, 3)
    max_shift = 2

    def __init__(self):
        self.calls, self.staged = [], []

    def stage_sample(self, raw_frames, dark=None, flat=None):
        self.staged.append((raw_frames, dark, flat))

    def sequence(self, state=None, lam=None, trunc=None, out=None):
        assert len(self.staged) == len(self.calls) + 1               # the stack was staged first
        self.calls.append((state, lam, trunc, out))
        out.fill_(float(len(self.calls)))
        return {"state": out, "dx": len(self.calls)}


def test_sequence_on_a_fake_model():
    import torch
    import umpa_amd
    from umpa_amd import sequence as S
    assert umpa_amd.sequence is S and S.__all__ == ["Sequence", "restate"]
    assert umpa_amd.Sequence is S.Sequence and umpa_amd.restate is S.restate
    assert all(n in umpa_amd.__all__ for n in ("sequence", "Sequence", "restate"))
    m = _FakeModel()
    q = S.Sequence(m, 0.25, trunc=3.0)
    assert q.state is None
    frames = [object() for _ in range(5)]
    outs = []
    for n in range(4):
        r = q.step(frames[n], dark="d%d" % n, flat="f%d" % n)
        assert r["dx"] == n + 1 and m.staged[n] == (frames[n], "d%d" % n, "f%d" % n)
        state, lam, trunc, out = m.calls[n]
        assert (lam, trunc) == (0.25, 3.0)
        assert isinstance(out, torch.Tensor) and out.dtype == torch.float64 and tuple(out.shape) == (3, 3, 2, 3)
        if n == 0:
            assert state is None                                      # the first step starts a series
        else:
            assert state is outs[n - 1] and out is not state and (state == float(n)).all()
        assert q.state is out
        outs.append(out)
    assert outs[2] is outs[0] and outs[3] is outs[1] and outs[0] is not outs[1]   # two tensors take turns, none is allocated per step
    q.reset()
    assert q.state is None
    q.step(frames[4])
    assert m.calls[4][0] is None and m.staged[4] == (frames[4], None, None) and (m.calls[4][3] is outs[0] or m.calls[4][3] is outs[1])
    with pytest.raises(RuntimeError, match=r"Sequence needs a model with sequence\(\)"):
        S.Sequence(object(), 0.1)
