"""
Writes tests/golden/integrate_dense.npz (the dense least-squares solutions of the cases of tests/integrate_expect.py,
component-demeaned) and tests/golden/integrate_observed.json (per case the worst deviation of the restated solve from
them and its iteration count).  numpy and scipy only; about two minutes.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import integrate_expect as E  # noqa: E402

dense, observed = {}, {}
for shape in E.SHAPES:
    for kind in ("ones", "holes"):
        name = E.case_name(shape, kind)
        gx, gy, w, _ = E.case(name)
        dense[name] = E.dense_live(name)
        phi, it, resid, status = E.pcg(gx, gy, w if kind == "holes" else None)
        assert status == E.CONVERGED
        observed[name] = {"deviation": E.deviation(phi, name, ref=dense[name]), "iterations": it, "residual": resid}
        print(name, observed[name], flush=True)
np.savez_compressed(os.path.join(HERE, "integrate_dense.npz"), **dense)
json.dump(observed, open(os.path.join(HERE, "integrate_observed.json"), "w"), indent=1, sort_keys=True)
