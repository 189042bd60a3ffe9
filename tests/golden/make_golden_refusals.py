"""
Writes tests/golden/refusals_observed.json: return code and complete error text of every call of tests/refusal_calls.py,
as the built libraries answer them on a machine WITHOUT a HIP device (the rows that the device count answers are recorded
with the others).  Recorded before the libraries' host scaffolds were folded into umpa_amd/csrc/umpa_host.h; the file pins
what they said then.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import refusal_calls  # noqa: E402
from umpa_amd import _lib  # noqa: E402

assert _lib.hip().device_count() == 0, "record on a machine without a HIP device"
observed = {}
for row in refusal_calls.rows():
    assert row[0] not in observed, row[0]
    code, text = refusal_calls.call(row)
    observed[row[0]] = {"code": code, "text": text, "no_device": row[4]}
    print("%-60s %3d  %s" % (row[0], code, text), flush=True)
json.dump(observed, open(os.path.join(HERE, "refusals_observed.json"), "w"), indent=1, sort_keys=True)
