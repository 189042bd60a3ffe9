"""
The refusals of the Python bindings, pinned in full: every call of tests/binding_refusal_calls.py raises the exception type
and the complete text recorded in tests/golden/binding_refusals_observed.json (tests/golden/make_golden_binding_refusals.py):
the host rows without a GPU, the rows on HIP tensors and on models with one.
"""
import json
import os

import pytest

from conftest import GOLDEN

import binding_refusal_calls as calls
import nativelibs


def _replay(needs, context=None):
    nativelibs.build_all()
    from umpa_amd import _lib
    observed = json.load(open(os.path.join(GOLDEN, "binding_refusals_observed.json")))
    rows = calls.rows()
    assert sorted(r[0] for r in rows) == sorted(observed) and len(rows) == len(observed) > 300
    for prefix in {r[0].split(":")[0] for r in rows}:                 # every function: a double refusal
        assert any("+" in r[0] for r in rows if r[0].startswith(prefix + ":")) or prefix in ("register.shift_data", "model.UMPAModelDFKernel.uncertainty"), prefix
    no_device = _lib.hip().device_count() == 0
    wrong, ran = [], 0
    for row in rows:
        want = observed[row[0]]
        assert (want["needs"], want["no_device"]) == (row[1], row[3]), row[0]
        assert want["type"], row[0]                                   # refused, every one
        if row[1] != needs or (row[3] and not no_device):             # answered by the device count: only without a device
            continue
        got = calls.observe(row, context)
        ran += 1
        if got != [want["type"], want["text"]]:
            wrong.append((row[0], got, [want["type"], want["text"]]))
    assert not wrong, "\n".join("%s: %r, recorded %r" % w for w in wrong)
    return ran, sum(1 for r in rows if r[1] == needs and not r[3])


def test_every_host_refusal_gives_the_recorded_type_and_text():
    ran, always = _replay("host")
    assert ran >= always > 100


@pytest.mark.gpu
def test_every_device_refusal_gives_the_recorded_type_and_text():
    ran, always = _replay("device", calls.Context())
    assert ran == always > 150
