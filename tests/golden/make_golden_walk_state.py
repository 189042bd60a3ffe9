"""
tests/golden/walk_state_parent.npz: what the kernels that inline walk_feed answered BEFORE the walk machine's state was
rewritten (the commit before "walk_feed: one way out"), for the cases of tests/test_hip_walk_state.py.

    python tests/golden/make_golden_walk_state.py            # on a GPU, with libumpa_hip.so built from that parent commit

The rewrite changes how the machine is expressed, not what it does: the test demands every byte of these maps.  Per case
the file holds err, Ncalls and the float maps in full, and of the two debug arrays (25 + 16 doubles per pixel, which would
not fit a committed file) their SHA-256.  The cases and how one is run are defined here, once; the test imports them.
"""
import contextlib
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "walk_state_parent.npz")

H, W, NW = 45, 61, 2        # with max_shift 3 a region of 35 x 51: no multiple of replay_walk's 4 rows or 16 columns
FULL = ("err", "debug_Ncalls", "T", "dx", "dy", "f", "df")
HASHED = ("debug_d", "debug_a")

# id -> frames, dark-field, max_shift, call cap (None: the default), zeroed patch, route ("tiled", "direct", "staged"), mask
CASES = {
    "df-K10-two-lookups": (10, True, 3, None, False, "tiled", False),
    "df-K12-one-lookup": (12, True, 3, None, False, "tiled", False),
    "nodf-K3": (3, False, 3, None, False, "tiled", False),
    "df-K10-ms2-bound": (10, True, 2, None, False, "tiled", False),
    "df-K10-cap7": (10, True, 3, 7, False, "tiled", False),
    "df-K10-zero-patch": (10, True, 3, None, True, "tiled", False),
    "df-K10-direct": (10, True, 3, None, False, "direct", False),
    "df-K10-staged": (10, True, 3, None, False, "staged", False),
    "df-K10-mask95-replay-cost": (10, True, 3, None, False, "tiled", True),
}


def stack(case):
    """(sam, ref, mask or None) of a case: a smooth displacement field of +-1.2 px, 0.5 % noise"""
    from umpa_amd.synth import make_stack
    K, df, ms, cap, zero, route, masked = CASES[case]
    sam, ref, _ = make_stack(H, W, K, ms, df=df, seed=410, amplitude=min(1.2, ms - 1.2), order=1)
    if zero:
        # A dead patch of the reference, wider than a window: where the reference window lies inside it every sum with a
        # reference factor is exactly 0 and the cost is 0 / 0 = NaN in the kernels and in the checker alike; the walks
        # around it step over NaN neighbours.  (Zeros in the sample stack as well would make costs of exactly 0 over
        # whole neighbourhoods, where `val < c0` of the gather decides by the last bit of two sums in different orders:
        # that compares the cost arithmetic, not the walk.)
        ref[:, 17:27, 24:37] = 0.0
    mask = (np.random.default_rng(411).random(sam.shape) < 0.95).astype(np.float64) if masked else None
    return sam, ref, mask


@contextlib.contextmanager
def environment(cap):
    """the plain (not on-demand) table kernels, and the case's call cap: both libraries read it when a model is created"""
    want = {"UMPA_HIP_ONDEMAND": "0", "UMPA_CALL_CAP": None if cap is None else str(cap)}
    old = {k: os.environ.get(k) for k in want}
    try:
        for k, v in want.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run(ns, case, hip=True):
    """One match of a case by the model classes of `ns` (umpa_amd.model, or the CPU checker's namespace):
    (maps, last_path or None)."""
    from umpa_amd import _lib
    K, df, ms, cap, zero, route, masked = CASES[case]
    sam, ref, mask = stack(case)
    with environment(cap):
        m = getattr(ns, "UMPAModelDF" if df else "UMPAModelNoDF")(sam, ref, mask_list=mask, window_size=NW, max_shift=ms)
        m.debug = True
        if hip:
            m._force = {"tiled": _lib.F_FORCE_TILED, "staged": _lib.F_FORCE_DIRECT,
                        "direct": _lib.F_FORCE_DIRECT | _lib.F_FORCE_PLAIN_DIRECT}[route]
        got = m.match(quiet=True)
    return got, (m._lib.last_path(m._handle) if hip else None)


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def record(got):
    """what the golden file keeps of one case's maps"""
    out = {k: np.ascontiguousarray(got[k]) for k in FULL if k in got}
    for k in HASHED:
        out[k + ".sha256"] = digest(got[k])
    return out


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from umpa_amd import model
    out = {}
    for case in CASES:
        got, path = run(model, case)
        for k, v in record(got).items():
            out[case + "/" + k] = v
        print("%-28s path %d, %d of %d pixels ok, Ncalls %d .. %d" % (
            case, path, int((got["err"] == 1).sum()), got["err"].size, got["debug_Ncalls"].min(), got["debug_Ncalls"].max()))
    np.savez_compressed(GOLDEN, **out)
    print("wrote %s (%d bytes)" % (GOLDEN, os.path.getsize(GOLDEN)))


if __name__ == "__main__":
    main()
