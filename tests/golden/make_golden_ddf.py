#!/usr/bin/env python3
"""
Golden fixture of the directional dark-field search (umpa_amd/ddf.py): the REFERENCE's `UMPAModelDFKernel.match` with the
same (a, b, c) at every pixel, for the three variants of tests/ddf_expect.GOLDEN_VARIANTS on the 64 x 72 x 3 stack of the
identity check (Nw = 2, max_shift = 4).  Run in the BUILD container only, after `__graft_entry__.build()` has made
oracle/_ref/libumpa_ref.so from the unmodified reference core.

Only data is written (tests/golden/K_ddf.npz): the input stacks and the reference's output maps f, T, dx, dy, err and
debug_Ncalls (the 4 x 4 and 5 x 5 debug arrays are left out: 41 doubles per pixel).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    from oracle import cpu_model
    import ddf_expect as DE
    if not cpu_model.have_ref():
        raise SystemExit("oracle/_ref/libumpa_ref.so is not built")
    sam, ref = DE.identity_stack()
    p = DE.IDENTITY
    out = {"sam": np.array(sam), "ref": np.array(ref)}
    meta = {"Nw": p["Nw"], "max_shift": p["max_shift"], "variants": []}
    for n, (abc, assign, subpx, roi) in enumerate(DE.GOLDEN_VARIANTS):
        res = DE.dfkernel_uniform(cpu_model.ref, sam, ref, abc, p["Nw"], p["max_shift"], roi, assign, subpx)
        for k in ("f", "T", "dx", "dy", "err", "debug_Ncalls"):
            out["v%d_%s" % (n, k)] = np.array(res[k])
        meta["variants"].append({"abc": list(abc), "assign": assign, "subpx": subpx, "ROI": roi})
        ok = res["err"] == 1
        print("variant %d %r %s subpx %d ROI %r: %d px, %d ok, median dx %.3f dy %.3f" % (
            n, abc, assign, subpx, roi, ok.size, ok.sum(), np.median(res["dx"][ok]), np.median(res["dy"][ok])))
        if ok.sum() < 0.5 * ok.size:
            raise SystemExit("variant %d: fewer than half of the pixels matched" % n)
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "K_ddf.npz")
    np.savez_compressed(path, **out)
    print("wrote K_ddf.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
