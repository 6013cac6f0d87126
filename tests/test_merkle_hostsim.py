"""plume_merkle_* on the host side (csrc/plume_merkle_capi.hip) under the sanitizers, on the CPU (tests/_hostsim.py): the ABI's
translation unit, the Merkle kernels as host loops (tests/hostsim/merkle_launch.cpp) and a driver (tests/hostsim/merkle_driver.cpp) that pins every output to vectors this
test writes from the restatement (tests/_merkle.py): the committed fixture's trees and one of 2 100 leaves (a stage of the sort in the workspace, per-depth launches under
the fused top).  Host forms with chunks of 1, 7 and n, the device forms chained on a caller stream (nothing runs before the caller synchronises), plume_init_multi contexts
over three and eight mock devices, argument errors, every allocation of a call failing in turn, no table built.  ASan + UBSan and TSan, lazy, random and eager schedulers:
stand-alone programs, nothing is loaded into Python.  One mutant of a launcher, which drops its stream argument, must fail the driver."""
import struct

import numpy as np
import pytest

from tests import _hostsim as H
from tests import _merkle as M

UNITS = dict(driver="merkle_driver", capi=["plume_merkle_capi.hip"], launch=["merkle_launch.cpp"])


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


@pytest.mark.parametrize("san,runs", H.RUNS)
def test_merkle_host_side_under_sanitizers(tmp_path, vectors, san, runs):
    exe = H.build(tmp_path / "b", san, **UNITS)
    for seed, sched in runs:
        H.ok(H.run(exe, vectors, seed, sched=sched), "merkle_driver", seed)
    if san != "thread":                                                      # one launch per depth all the way up gives the same trees
        H.ok(H.run(exe, vectors, 5, extra_env={"PLUME_MERKLE_FUSED_TOP": "0"}), "merkle_driver", 5)


def test_the_driver_fails_when_a_launcher_drops_its_stream(tmp_path, vectors):
    r = H.run(H.build(tmp_path / "b", "", **UNITS, defs={"merkle_launch.cpp": ["-DMERKLE_MUTANT_DROPS_STREAM"]}), vectors, 1)
    assert r.returncode != 0 and "merkle_driver:" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])
