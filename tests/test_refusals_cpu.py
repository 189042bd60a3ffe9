"""
The refusals of the satellite libraries' C ABI, pinned in full: every call of tests/refusal_calls.py gives the return code
and the complete error text recorded in tests/golden/refusals_observed.json (tests/golden/make_golden_refusals.py).
"""
import json
import os

from conftest import GOLDEN

import nativelibs
import refusal_calls


def test_every_refusal_gives_the_recorded_code_and_text():
    nativelibs.build_all()
    from umpa_amd import _lib
    observed = json.load(open(os.path.join(GOLDEN, "refusals_observed.json")))
    rows = refusal_calls.rows()
    assert sorted(r[0] for r in rows) == sorted(observed) and len(rows) == len(observed) > 150
    for lib, fn in {(r[1], r[2]) for r in rows}:                      # every entry point: a single and a double refusal
        mine = [r[0] for r in rows if (r[1], r[2]) == (lib, fn) and not r[4]]
        assert mine and any("+" in n for n in mine) or fn == "attach", (lib, fn)
    no_device = _lib.hip().device_count() == 0
    wrong, ran = [], 0
    for row in rows:
        want = observed[row[0]]
        assert want["no_device"] == row[4], row[0]
        if row[4] and not no_device:                                  # answered by the device count: only without a device
            continue
        code, text = refusal_calls.call(row)
        ran += 1
        assert code <= 0, row[0]                                      # refused, every one
        if (code, text) != (want["code"], want["text"]):
            wrong.append((row[0], (code, text), (want["code"], want["text"])))
    assert not wrong, "\n".join("%s: %r, recorded %r" % w for w in wrong)
    assert ran == len(rows) - (0 if no_device else sum(1 for r in rows if r[4]))
