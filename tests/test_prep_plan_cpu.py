"""
Which sides of the maps a match computes (umpa_amd/csrc/umpa_prep_plan.h), checked without a GPU: tests/prep_plan_check.cpp
drives the header through random lives of a model -- matches on random tile rectangles, reference and sample updates, new
windows, kinds, frame counts and plane sizes, subset matches, reallocations, frames the library owns and frames it borrows,
with UMPA_HIP_F_REUSE_REF_MAPS and without -- against a model that knows, per tile, what the tile's reference-side planes were
computed from.  A host program of its own, built with the host compiler, and once more under AddressSanitizer and UBSan.
"""
import os
import re
import shutil
import subprocess

import pytest

from conftest import REPO

STEPS = 200000


def _build(tmp_path, tag, flags):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / ("prep_plan_check_" + tag))
    subprocess.run([cxx, "-std=c++17"] + flags + ["-I", os.path.join(REPO, "umpa_amd", "csrc"),
                    os.path.join(REPO, "tests", "prep_plan_check.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("tag,flags", [
    pytest.param("plain", ["-O1"], id="host-compiler"),
    pytest.param("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], id="asan-ubsan"),
])
def test_no_match_reads_stale_reference_maps_and_whole_roi_whole_reuses(tmp_path, tag, flags):
    """Every step: no tile a match reads is taken from reference-side maps of another reference stack, window, layout or
    allocation.  Every so often: [whole region, ROI, whole region] with nothing changed computes the reference side once.
    (With the rectangle also overwritten by a sample-only pass the second fails at step 53 of the default seed; with frames
    the library borrows trusted like its own the first fails at step 47.)"""
    out = subprocess.run([_build(tmp_path, tag, flags), str(STEPS)], check=True, capture_output=True, text=True).stdout
    m = re.search(r"(\d+) steps, (\d+) matches \((\d+) computed the reference side, (\d+) reused it\), (\d+) whole/ROI/whole triples: OK", out)
    assert m, out
    steps, matches, computed, reused, triples = (int(x) for x in m.groups())
    assert steps == STEPS >= 100000 and computed + reused == matches
    assert reused > 10000 and computed > 10000 and triples > 1000, out      # the sequence went both ways often enough to mean something


def test_the_library_decides_through_the_header():
    """run_tiled, tiled_maps and tiled_prep call the header's functions, and nothing else in the native sources writes the
    record's flag or rectangle."""
    src = {f: open(os.path.join(REPO, "umpa_amd", "csrc", f)).read() for f in os.listdir(os.path.join(REPO, "umpa_amd", "csrc"))
           if f.endswith((".h", ".hip"))}
    for f, text in src.items():
        if f != "umpa_prep_plan.h":
            assert not re.search(r"ref_(maps_ok|rect\[\d\]|kind|K|plane)\s*=[^=]", text), f
    assert "prep_reuse(sub != nullptr, m->owns_frames, (flags & UMPA_HIP_F_REUSE_REF_MAPS) != 0)" in src["umpa_hip.hip"]
    tiled = src["umpa_tiled.h"]
    for call in ("prep_plan_layout(st,", "prep_plan_sides(st, PR, reuse, reuse_sides)", "prep_plan_done(st, PR, sides,"):
        assert call in tiled, call
    plan = src["umpa_prep_plan.h"]
    assert "hip" not in re.sub(r"//.*", "", plan).lower()                  # no device code, no HIP type: the host compiler builds it
