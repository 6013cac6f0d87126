"""plume_merkle_* on the host side (csrc/plume_merkle_capi.hip) under the sanitizers, on the CPU: the unchanged objects of the
existing host-side harness (tests/hostsim/Makefile: plume_capi.hip against the mock HIP runtime, the other kernels as host loops, the C oracle) linked with the ABI's
translation unit, the Merkle kernels as host loops (tests/hostsim/merkle_launch.cpp) and a driver (tests/hostsim/merkle_driver.cpp) that pins every output to vectors this
test writes from the restatement (tests/_merkle.py): the committed fixture's trees and one of 2 100 leaves (a stage of the sort in the workspace, per-depth launches under
the fused top).  Host forms with chunks of 1, 7 and n, the device forms chained on a caller stream (nothing runs before the caller synchronises), plume_init_multi contexts
over three and eight mock devices, argument errors, every allocation of a call failing in turn, no table built.  ASan + UBSan and TSan, lazy, random and eager schedulers:
stand-alone programs, nothing is loaded into Python.  One mutant of a launcher, which drops its stream argument, must fail the driver."""
import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import _merkle as M

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "zk-nullifier-sig_amd" / "csrc"
HOSTSIM = ROOT / "tests" / "hostsim"
FLAGS = ["-std=c++17", "-g", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off", "-DPLUME_GW=16", "-DPLUME_COMB_W=10", f"-I{HOSTSIM / 'mockhip'}", f"-I{CSRC}"]


def _san_flags(san):
    return [f"-fsanitize={san}", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if san else []


def _build(out, san, launch_defs=()):
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("no g++ / make")
    out.mkdir(parents=True, exist_ok=True)
    subprocess.run(["make", "-C", str(HOSTSIM), f"OUT={out}", f"SAN={san}", "-j2", str(out / "capi.o"), str(out / "launch.o"), str(out / "oracle.o")],
                   check=True, capture_output=True, text=True, timeout=1200)
    flags = FLAGS + _san_flags(san)
    units = [(["-x", "c++", "-O1", "-Werror"], CSRC / "plume_merkle_capi.hip", "mcapi.o"), (["-O2", "-Werror", *launch_defs], HOSTSIM / "merkle_launch.cpp", "mlaunch.o"),
             (["-O1", "-Werror"], HOSTSIM / "merkle_driver.cpp", "mdriver.o")]
    procs = [subprocess.Popen(["g++", *extra, *flags, "-c", str(src), "-o", str(out / obj)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for extra, src, obj in units]
    for p, (_, src, _) in zip(procs, units):
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, (src.name, err[-4000:])
    exe = out / "merkle_driver"
    subprocess.run(["g++", *_san_flags(san), "-o", str(exe), *[str(out / o) for o in ("capi.o", "launch.o", "oracle.o", "mcapi.o", "mlaunch.o", "mdriver.o")], "-lpthread"],
                   check=True, capture_output=True, text=True, timeout=600)
    return exe


def _record(t):
    return struct.pack("<5I", t["leaf_format"], t["addr_format"], t["sort"], t["n"], t["depth"]) + b"".join(
        bytes.fromhex(t[k]) if isinstance(t[k], str) else b"" for k in ("items", "amounts", "leaves")) + bytes(t["leaf_status"]) + bytes.fromhex(t["tree"]) + \
        np.array(t["leaf_pos"], np.uint32).tobytes() + bytes.fromhex(t["proofs"]) + bytes(t["proof_len"])


@pytest.fixture(scope="module")
def vectors(tmp_path_factory):
    trees = list(M.load_kats()["trees"])
    rng = np.random.default_rng(2100)
    n = 2100
    leaves = [rng.bytes(32) for _ in range(n)]
    leaves[700] = leaves[3]
    tree, pos = M.build(leaves, sort=True)
    depth = M.max_proof_len(n)
    proof, ln = M.proof_batch(tree, pos, depth)
    trees.append({"leaf_format": 0, "addr_format": 0, "sort": 1, "n": n, "depth": depth, "items": b"".join(leaves).hex(), "amounts": None, "leaves": b"".join(leaves).hex(),
                  "leaf_status": [1] * n, "tree": b"".join(tree).hex(), "leaf_pos": pos, "proofs": proof.tobytes().hex(), "proof_len": [int(x) for x in ln]})
    path = tmp_path_factory.mktemp("merkle_vectors") / "vectors.bin"
    path.write_bytes(struct.pack("<I", len(trees)) + b"".join(_record(t) for t in trees))
    return path


def _run(exe, vectors, seed, sched, extra_env=None):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")
    for k in ("PLUME_MOCK_SCHED", "PLUME_SUB_BATCHES", "PLUME_SERIAL", "PLUME_STAGE_TIMES", "PLUME_OVERLAP_MIN", "PLUME_MSM_PAIR_MAX", "PLUME_INGEST_SPLIT_MAX", "PLUME_MERKLE_FUSED_TOP"):
        env.pop(k, None)
    if sched:
        env["PLUME_MOCK_SCHED"] = sched
    env.update(extra_env or {})
    return subprocess.run([str(exe), str(vectors), str(seed)], capture_output=True, text=True, timeout=1500, env=env)


def _ok(r, seed):
    assert r.returncode == 0, (seed, r.stdout[-2000:], r.stderr[-4000:])
    assert f"merkle_driver seed {seed}: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "WARNING: ThreadSanitizer" not in r.stderr


@pytest.mark.parametrize("san,runs", [("address,undefined", [(1, None), (2, "random:2"), (3, "eager")]), ("thread", [(4, "random:4")])])
def test_merkle_host_side_under_sanitizers(tmp_path, vectors, san, runs):
    exe = _build(tmp_path / "b", san)
    for seed, sched in runs:
        _ok(_run(exe, vectors, seed, sched), seed)
    if san != "thread":                                                      # one launch per depth all the way up gives the same trees
        _ok(_run(exe, vectors, 5, None, {"PLUME_MERKLE_FUSED_TOP": "0"}), 5)


def test_the_driver_fails_when_a_launcher_drops_its_stream(tmp_path, vectors):
    r = _run(_build(tmp_path / "b", "", launch_defs=["-DMERKLE_MUTANT_DROPS_STREAM"]), vectors, 1, None)
    assert r.returncode != 0 and "merkle_driver:" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])
