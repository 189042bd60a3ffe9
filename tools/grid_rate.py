#!/usr/bin/env python3
"""what the exhaustive table's other consumers cost beside the walk.

    python tools/grid_rate.py [--out FILE] [--repeats N] [--configs C2,C3] [--walk-lib OTHER_LIBUMPA_HIP_SO]

Per config (BASELINE C2: 2048^2 x 10 frames, Nw 5, max_shift 5; C3: 4096^2 x 20 frames, Nw 7, max_shift 8; dark-field,
synthetic stacks) in ONE process, alternating, N times after a warm-up of each:
    search='walk', search='grid', cost_volume(with_fit) of a 256-row ROI
the per-kernel HIP-event times of the library's own timers (umpa_hip_timing_*: `table_consumer` brackets grid_min_kernel
or cost_volume_kernel, launched where `replay_walk` would be), device-resident outputs (F_DEVICE_IO, no downloads), and
the host wall time of the whole call around a stream synchronise.  Median and range over the repeats.

--walk-lib: the walk of ANOTHER build of libumpa_hip.so (the parent commit's) timed in a child process per repeat,
alternating with this build's, on the same stack: the hook's host path must not show (+-3 %).
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"C2": dict(n=2048, K=10, Nw=5, ms=5, seed=0), "C3": dict(n=4096, K=20, Nw=7, ms=8, seed=11)}
ROI_ROWS = 256


def kernel_times(m):
    lib, h = m._lib, m._handle
    out = {}
    for q in range(lib.timing_collect(h)):
        nm, tot, cnt = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_int()
        lib.timing_read(h, q, ctypes.byref(nm), ctypes.byref(tot), ctypes.byref(cnt))
        out[nm.value.decode()] = tot.value
    return out


def device_calls(m, with_volume=True):
    """walk / grid / volume on device-resident outputs: closures that enqueue on the current torch stream"""
    import torch
    from umpa_amd import _lib
    N0, N1 = m.extent
    U, ms = 2 * m.max_shift - 1, m.max_shift
    dev = torch.device("cuda", m._device)
    values = torch.zeros((m.Nparam, N0, N1), dtype=torch.float64, device=dev)
    err = torch.zeros((N0, N1), dtype=torch.int32, device=dev)
    rows = min(ROI_ROWS, N0)
    vol = [torch.zeros((U, U, rows, N1) if with_volume else (1,), dtype=torch.float64, device=dev) for _ in range(3)]
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    flags = _lib.F_DEVICE_IO | _lib.F_PLANAR
    region = (m._handle, 0, 1, N0, 0, 1, N1, values.data_ptr(), m.Nparam, None, err.data_ptr(), None, 0.0, None, None, None)
    r0 = (N0 - rows) // 2

    def walk():
        m._lib.check(m._lib.match_region(*region, flags | _lib.F_FORCE_TILED, sp), "match_region")

    def grid():
        g = _lib.grid()
        g.check(g.match_region(*region, flags, sp), "grid match_region")

    def volume():
        g = _lib.grid()
        g.check(g.cost_volume(m._handle, r0, 1, rows, 0, 1, N1, vol[0].data_ptr(), vol[1].data_ptr(), vol[2].data_ptr(),
                              _lib.F_DEVICE_IO, sp), "grid cost_volume")

    return dict(walk=walk, grid=grid, volume=volume), (values, err, vol)


def timed(m, fn):
    import time
    import torch
    torch.cuda.synchronize()
    m._lib.timing_enable(m._handle, 1)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    m._lib.timing_enable(m._handle, 0)
    k = kernel_times(m)
    k["wall"] = wall
    return k


def run_config(name, repeats, only=None):
    from umpa_amd import model
    from umpa_amd.synth import make_stack
    c = CONFIGS[name]
    sam, ref, _ = make_stack(c["n"], c["n"], c["K"], c["ms"], df=True, seed=c["seed"], order=1)
    m = model.UMPAModelDF(sam, ref, window_size=c["Nw"], max_shift=c["ms"])
    calls, keep = device_calls(m, with_volume=not only or "volume" in only)
    if only:
        calls = {k: calls[k] for k in only}
    for fn in calls.values():                                        # warm-up: code objects, scratch, the table
        timed(m, fn)
    series = {k: [] for k in calls}
    for _ in range(repeats):
        for k, fn in calls.items():                                  # alternating
            series[k].append(timed(m, fn))
    out = {}
    for k, runs in series.items():
        out[k] = {}
        for kern in sorted(set().union(*runs)):
            v = [r.get(kern, 0.0) for r in runs]
            out[k][kern] = dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))
    return out


def fmt(name, res, c):
    lines = ["%s: %d^2 x %d frames, Nw %d, max_shift %d, dark-field; ms per call, median [min .. max]" % (name, c["n"], c["K"], c["Nw"], c["ms"])]
    for call, kernels in res.items():
        lines.append("  %s" % {"walk": "search='walk'", "grid": "search='grid'", "volume": "cost_volume, %d rows, with T and df" % ROI_ROWS}.get(call, call))
        for kern, v in kernels.items():
            lines.append("    %-16s %9.3f  [%9.3f .. %9.3f]" % (kern, v["median"], v["min"], v["max"]))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--walk-lib")
    ap.add_argument("--child-walk", help=argparse.SUPPRESS)          # internal: one config's walk, JSON on stdout
    a = ap.parse_args()
    if a.child_walk:
        print(json.dumps(run_config(a.child_walk, a.repeats, only=("walk",))))
        return
    lines = []
    for name in a.configs.split(","):
        res = run_config(name, a.repeats)
        first = len(lines)
        lines += fmt(name, res, CONFIGS[name])
        print("\n".join(lines[first:]), flush=True)                  # before the children: a time limit must not lose these
        first = len(lines)
        if a.walk_lib:
            # fresh processes, alternating: this build's walk and the other build's, same stack, same call
            rows = {"this build": [], "other build": []}
            for rep in range(3):
                for tag, lib in (("this build", None), ("other build", a.walk_lib)):
                    env = dict(os.environ)
                    if lib:
                        env["UMPA_GRID_RATE_HIP_LIB"] = os.path.abspath(lib)
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-walk", name, "--repeats", str(a.repeats)],
                                       env=env, stdout=subprocess.PIPE, check=True, text=True, timeout=600)
                    rows[tag].append(json.loads(p.stdout.strip().splitlines()[-1])["walk"])
            lines.append("  search='walk', this build against %s (3 processes each, alternating; medians of %d calls)" % (a.walk_lib, a.repeats))
            for tag, rs in rows.items():
                for kern in ("wall", "prep_maps", "corr_volume", "corr_march", "replay_walk"):
                    if kern in rs[0]:
                        lines.append("    %-12s %-12s %s" % (tag, kern, "  ".join("%9.3f" % r[kern]["median"] for r in rs)))
        print("\n".join(lines[first:]), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if os.environ.get("UMPA_GRID_RATE_HIP_LIB"):                     # the child of --walk-lib: bind the other build
        from umpa_amd import _lib
        _lib.HIP_LIB_PATH = os.environ["UMPA_GRID_RATE_HIP_LIB"]
    main()
