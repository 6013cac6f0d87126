"""The persistent nullifier set's per-lane bodies (zk-nullifier-sig_amd/csrc/plume_nullset.h) on the host: tests/nullset/nullset_lanes.cpp compiled with g++ under
AddressSanitizer + UBSan runs probe / commit / contains / rehash / export lanes in forward, reversed and random orders on exactly-sized tables, against a std::set and the
definition of `fresh` (sequences with live masks and descending ids, growth, clear, export round trips, a 64-slot table where every record has one home slot)."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "zk-nullifier-sig_amd" / "csrc"


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("nullset_lanes") / "nullset_lanes"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}",
                    str(ROOT / "tests" / "nullset" / "nullset_lanes.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True, timeout=600)
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3, 20261016])
def test_lane_bodies_match_the_definition(harness, seed):
    r = subprocess.run([str(harness), str(seed)], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert f"nullset_lanes {seed} ok" in r.stdout
