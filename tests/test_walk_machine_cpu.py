"""
The walk machine of umpa_amd/csrc/umpa_walk.h, compiled for the host and held to oracle/umpa_oracle.c (no GPU).

tests/walk_machine_check.cpp is a program of its own: it includes the header with UMPA_WALK_HOST (the few shims a host
compiler needs; the device sees none of them), links the oracle's C file, and runs every walk twice -- umpaor_min, and
walk_begin / walk_feed / walk_finish fed by umpaor_cost, every second walk with replay_walk's second delivery
(walk_speculate).  Status, Ncalls, f, T, df, uv, the memo and the 4x4 neighbourhood must agree bit for bit over more than
200 000 walks: 1-4 frames, windows 3-7, max_shift 2-5, both models, both shift conventions, three noise levels, a
constant image (exact ties), zeroed patches and all-zero stacks (NaN costs, the move cap), call caps 3 .. 40.
Built twice: optimised, and with AddressSanitizer + UBSan (host code with its own main; nothing is preloaded).
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp, tag, flags):
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cc and cxx, "no host C / C++ compiler"
    obj, exe = str(tmp / ("oracle_%s.o" % tag)), str(tmp / ("walk_machine_check_" + tag))
    # -ffp-contract=off and no -ffast-math: both sides evaluate costs with the same function, whatever gets inlined where
    subprocess.run([cc, "-std=c11", "-ffp-contract=off", "-fopenmp"] + flags + ["-c", os.path.join(REPO, "oracle", "umpa_oracle.c"), "-o", obj],
                   check=True)
    subprocess.run([cxx, "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-DUMPA_WALK_HOST"] + flags +
                   ["-I" + os.path.join(REPO, "umpa_amd", "csrc"), os.path.join(REPO, "tests", "walk_machine_check.cpp"), obj,
                    "-o", exe, "-lm", "-fopenmp"], check=True)
    return exe


def _run(exe, args=()):
    p = subprocess.run([exe] + list(args), capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    return {k: int(v) for k, v in re.findall(r"(\w+) (\d+)", p.stdout)}


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("walk_machine")


def test_machine_walks_like_the_oracle(tmp):
    c = _run(_build(tmp, "opt", ["-O2"]))
    print(c)
    assert c["mismatches"] == 0
    assert c["walks"] >= 200000
    # the run went where a rewrite of the control flow can go wrong
    assert c["ok"] > 10000 and c["bound"] > 10000 and c["call_capped"] > 1000
    assert c["restarts"] > 5000 and c["move_capped"] > 10 and c["nan_walks"] > 10000 and c["tie_walks"] > 10000
    assert c["second_deliveries"] > 50000


def test_machine_under_the_sanitizers(tmp):
    """the same program with AddressSanitizer and UBSan, a tenth of the walks on another seed"""
    c = _run(_build(tmp, "san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), ["8", "7"])
    print(c)
    assert c["mismatches"] == 0 and c["walks"] >= 20000 and c["restarts"] > 500 and c["call_capped"] > 100
