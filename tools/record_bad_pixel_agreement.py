#!/usr/bin/env python3
"""Record tests/golden/bad_pixel_agreement.npz: for every non-finite bad-pixel case of tests/regimes.py, whether the in-place
build of the reference (oracle/_ref) returns at all -- it has no UMPA_MOVE_CAP and walks over NaN costs for ever on some
stacks -- and, where it does, on which output pixels it agrees with the plain-C oracle (regimes.checkers_agree, packed bits).
Each case runs in a child process under a time limit; a case that does not return is listed under "hangs".
tests/test_regimes_cpu.py re-checks the table where oracle/_ref is built, tests/test_hip_regimes.py holds the kernels to the
oracle on the agreed pixels."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [root, os.path.join(root, "tests")]
LIMIT = 30


def one(name, kind, where, out):
    import numpy as np
    import regimes as R
    from oracle import cpu_model
    sam, ref = R.bad_pixels(*R.base_stack(name), kind, where, R.bad_positions(R.CONFIGS[name]))
    a, _ = R.run(cpu_model.port, name, sam, ref)
    b, _ = R.run(cpu_model.ref, name, sam, ref)
    np.save(out, np.packbits(R.checkers_agree(a, b)))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--one"]:
        one(*sys.argv[2:6])
        sys.exit(0)
    import tempfile
    import numpy as np
    import regimes as R
    cases = [(n, k, w) for n in R.CONFIGS for k in R.BAD_VALUES if k != "zero" for w in ("sam", "ref")]
    tmp = tempfile.mkdtemp()

    def job(c):
        out = os.path.join(tmp, "%s_%s_%s.npy" % c)
        try:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--one", *c, out], timeout=LIMIT, check=True,
                           env=dict(os.environ, OMP_NUM_THREADS="1"), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            return c, np.load(out)
        except subprocess.TimeoutExpired:
            return c, None

    with ThreadPoolExecutor(int(sys.argv[1]) if len(sys.argv) > 1 else 4) as ex:
        res = list(ex.map(job, cases))
    table = {R.bad_key(*c): v for c, v in res if v is not None}
    table["hangs"] = np.array(sorted(R.bad_key(*c) for c, v in res if v is None))
    np.savez_compressed(os.path.join(root, "tests", "golden", "bad_pixel_agreement.npz"), **table)
    print("%d cases returned, %d did not within %d s:" % (len(table) - 1, len(table["hangs"]), LIMIT), ", ".join(table["hangs"]))
