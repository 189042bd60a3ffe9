#!/usr/bin/env python3
"""what the grid consumers cost on the general table, beside the walk on the same model and beside the
fp64 floor of the brute-force sum.

    python tools/general_grid_rate.py [--out FILE] [--repeats N] [--size 2048]

Two models, C2's parameters (10 frames, Nw 5, max_shift 5, dark-field), device-resident arrays (F_DEVICE_IO, no transfers):
    the 2 x 2 sample-stepping stack of tools/stepping_rate.py (four positions 64 pixels apart), whole extent;
    C2's stack at one position, forced onto the direct kernel, a band of 256 rows.
Per model, N times after a warm-up: match() (the walk, as the model runs it) and search='grid' with general_grid on, each with
the library's own HIP-event timers.  `table_consumer` brackets general_table_kernel AND the consumer's kernel (masked_min) of
every row chunk in one pair of events (the library has no call that runs a consumer on a table that is already there): the
bracket is reported as it is, and the consumer's share is gauged by a device copy of the table's cost planes (what
masked_min must read), timed with HIP events.  The floor: 3 Na (2 Nw + 1)^2 (2 ms - 1)^2 FMAs per pixel at the vector fp64
rate of the MI355X (78.6 TFLOP/s = 39.3 T FMA/s).  No pass mark: the rows are the measurement.
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, NW, MS = 10, 5, 5
FP64_FMA_PER_S = 78.6e12 / 2


def timers(m, fn):
    """fn() with the library's timers on: {kernel family: (ms, launches)}"""
    lib, h = m._lib, m._handle
    lib.timing_enable(h, 1)
    try:
        fn()
        import torch
        torch.cuda.synchronize()
    finally:
        seen = {}
        for q in range(lib.timing_collect(h)):
            nm, tot, cnt = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_int()
            lib.timing_read(h, q, ctypes.byref(nm), ctypes.byref(tot), ctypes.byref(cnt))
            seen[nm.value.decode()] = (tot.value, cnt.value)
        lib.timing_enable(h, 0)
    return seen


def calls_of(m, rows):
    import torch
    from umpa_amd import _lib
    N0, N1 = m.extent
    N0 = min(N0, rows) if rows else N0
    dev = torch.device("cuda", m._device)
    values = torch.zeros((m.Nparam, N0, N1), dtype=torch.float64, device=dev)
    err = torch.zeros((N0, N1), dtype=torch.int32, device=dev)
    cm = m.coverage(ROI=((0, N0, 1), (0, N1, 1)))
    cover = torch.from_numpy(cm).to(dev)
    thr = float(.1 * cm.max() / K)
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    flags = _lib.F_DEVICE_IO | _lib.F_PLANAR | m._force
    region = (m._handle, 0, 1, N0, 0, 1, N1, values.data_ptr(), m.Nparam, None, err.data_ptr(), cover.data_ptr(), thr, None, None, None)

    def walk():
        m._lib.check(m._lib.match_region(*region, flags, sp), "match_region")

    def grid():
        g = _lib.grid()
        g.check(g.match_region(*region, flags, sp), "grid match_region")
    return dict(walk=walk, grid=grid), (N0, N1), (values, err, cover)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--size", type=int, default=2048)
    a = ap.parse_args()
    import numpy as np
    import torch
    from umpa_amd import _lib, model
    from umpa_amd.synth import make_stack
    H = W = a.size
    sam, ref, _ = make_stack(H, W, K, MS, df=True, seed=0, order=1)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    for title, rows in (("2 x 2 sample stepping, whole extent", 0), ("one position, forced direct, 256 rows", 256)):
        if rows:
            m = model.UMPAModelDF(sam, ref, window_size=NW, max_shift=MS)
            m._force = _lib.F_FORCE_DIRECT
        else:
            m = model.UMPAModelDF([np.ascontiguousarray(sam[k, :H - 64, :W - 64]) for k in range(K)],
                                  [np.ascontiguousarray(ref[k, :H - 64, :W - 64]) for k in range(K)], window_size=NW, max_shift=MS,
                                  pos_list=[np.array([64 * ((k // 2) % 2), 64 * (k % 2)]) for k in range(K)])
        m.general_grid = True
        calls, (N0, N1), keep = calls_of(m, rows)
        U = 2 * MS - 1
        floor_ms = 3.0 * K * (2 * NW + 1) ** 2 * U * U * N0 * N1 / FP64_FMA_PER_S * 1e3
        say("%s: %d x %d pixels, %d frames, Nw %d, max_shift %d, dark-field" % (title, N0, N1, K, NW, MS))
        for name in ("walk", "grid"):
            calls[name]()
            torch.cuda.synchronize()
            got = [timers(m, calls[name]) for _ in range(a.repeats)]
            path = m._lib.last_path(m._handle)
            for fam in sorted(got[0]):
                ms = [g[fam][0] for g in got]
                say("  %-5s path %d  %-16s %9.2f ms (%.2f .. %.2f), %d launches" % (name, path, fam, statistics.median(ms), min(ms), max(ms), got[0][fam][1]))
        say("  fp64 floor of the brute-force sum (3 Na (2Nw+1)^2 (2ms-1)^2 FMAs per pixel at 39.3 T FMA/s): %.2f ms" % floor_ms)
        src = torch.empty((U * U, N0, N1), dtype=torch.float64, device=keep[0].device)
        dst = torch.empty_like(src)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        dst.copy_(src)
        t0.record()
        dst.copy_(src)
        t1.record()
        torch.cuda.synchronize()
        say("  device copy of the cost planes (%d x %d x %d doubles; masked_min reads as much): %.2f ms" % (U * U, N0, N1, t0.elapsed_time(t1)))
        del m, keep, src, dst
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
