"""
Writes tests/golden/binding_refusals_observed.json: exception type and complete text of every call of
tests/binding_refusal_calls.py, as the package answered them before the bindings' host / device twins, region checks and
cost_volume calls were written once; the file pins what they said then.

``python tests/golden/make_golden_binding_refusals.py host`` records the host rows, on a machine WITHOUT a HIP device (the
rows that the device count answers are recorded with the others); ``... device [FILE]`` records the device rows on a
machine with one.  Either merges its rows into FILE (default: the golden file).
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import binding_refusal_calls as calls  # noqa: E402
from umpa_amd import _lib  # noqa: E402

needs = sys.argv[1]
path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "binding_refusals_observed.json")
assert needs in ("host", "device") and (_lib.hip().device_count() == 0) == (needs == "host"), "host rows without a HIP device, device rows with one"
observed = json.load(open(path)) if os.path.exists(path) else {}
context = calls.Context() if needs == "device" else None
for row in calls.rows():
    if row[1] != needs:
        continue
    kind, text = calls.observe(row, context)
    observed[row[0]] = {"type": kind, "text": text, "needs": needs, "no_device": row[3]}
    print("%-70s %-14s %s" % (row[0], kind, text), flush=True)
json.dump(observed, open(path, "w"), indent=1, sort_keys=True)
