"""The lane bodies of the Merkle calls (zk-nullifier-sig_amd/csrc/plume_merkle.h) on the host: tests/merkle/merkle_lanes.cpp, a stand-alone program built by its Makefile
with g++ under AddressSanitizer + UBSan and -Werror, against the restatement of tests/_merkle.py.  The grid and the sort's stage schedule are host loops over the same
compare-exchange and node bodies the kernels run.  The whole fixture through every mode; n = 2^k - 1, 2^k, 2^k + 1 for k = 1 .. 11 with seeded leaves (the last sizes cross
the 2048-record tile: a stage in the workspace and a merge); outputs at odd offsets between guard bytes, inputs in allocations that end with their last byte."""
import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import _merkle as M

ROOT = Path(__file__).resolve().parent.parent
G = b"\xAA" * 32


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("no g++ / make")
    out = tmp_path_factory.mktemp("merkle_lanes")
    subprocess.run(["make", "-C", str(ROOT / "tests" / "merkle"), f"OUT={out}"], check=True, capture_output=True, text=True, timeout=900)
    return out / "merkle_lanes"


def _exec(harness, tmp_path, mode, head, arrays, out_sizes):
    """head: (a, b, n, m, depth, mis_in, mis_out, flags); returns the output arrays, their guards checked"""
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<8I", *head) + b"".join(bytes(a) for a in arrays))
    r = subprocess.run([str(harness), mode, str(fin), str(fout)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "merkle_lanes ok" in r.stdout, (mode, head, r.returncode, r.stdout[-500:], r.stderr[-4000:])
    got, res, pos = fout.read_bytes(), [], 0
    for sz in out_sizes:
        seg = got[pos:pos + 64 + sz]
        pos += len(seg)
        assert seg[:32] == G and seg[-32:] == G, f"{mode}: bytes outside an output array were written {head}"
        res.append(seg[32:-32])
    assert pos == len(got)
    return res


def _build(harness, tmp_path, leaves, sort, mis_in=0, mis_out=1, want_pos=True):
    n = len(leaves) // 32
    tree, pos = _exec(harness, tmp_path, "build", (0, 0, n, 0, 0, mis_in, mis_out, (1 if sort else 0) | (0 if want_pos else 2)), [leaves],
                      [32 * (2 * n - 1), 4 * n if want_pos else 0])
    return tree, list(np.frombuffer(pos, np.uint32))


def test_the_fixture_through_every_mode(harness, tmp_path):
    kats = M.load_kats()
    trees = {}
    for k, t in enumerate(kats["trees"]):
        n, mis_in, mis_out = t["n"], k % 5, 1 + 2 * (k % 7)
        arrays = [bytes.fromhex(t["items"])] + ([bytes.fromhex(t["amounts"])] if t["leaf_format"] == M.LEAF_ADDRESS_UINT256 else [])
        leaf, st = _exec(harness, tmp_path, "leaf", (t["leaf_format"], t["addr_format"], n, 0, 0, mis_in, mis_out, 0), arrays, [32 * n, n])
        assert leaf.hex() == t["leaves"] and list(st) == t["leaf_status"], t["name"]
        tree, pos = _build(harness, tmp_path, leaf, t["sort"], mis_in, mis_out, want_pos=k % 4 != 3)
        assert tree.hex() == t["tree"] and (pos == t["leaf_pos"] or k % 4 == 3), t["name"]
        proof, ln = _exec(harness, tmp_path, "proof", (0, 0, n, n, t["depth"], mis_in, mis_out, 0), [tree, np.array(t["leaf_pos"], np.uint32).tobytes()],
                          [32 * t["depth"] * n, n])
        assert proof.hex() == t["proofs"] and list(ln) == t["proof_len"], t["name"]
        trees[t["name"]] = tree
    for k, c in enumerate(kats["proof_cases"]):
        n, m = (len(trees[c["tree"]]) // 32 + 1) // 2, len(c["pos"])
        proof, ln = _exec(harness, tmp_path, "proof", (0, 0, n, m, c["depth"], k % 3, 5 + k, 0), [trees[c["tree"]], np.array(c["pos"], np.uint32).tobytes()],
                          [32 * c["depth"] * m, m])
        assert proof.hex() == c["proofs"] and list(ln) == c["proof_len"], (c["tree"], c["depth"])
    for k, c in enumerate(kats["verify_cases"]):
        m = len(c["status"])
        arrays = [bytes.fromhex(c["items"])] + ([bytes.fromhex(c["amounts"])] if c["leaf_format"] == M.LEAF_ADDRESS_UINT256 else []) + \
                 [bytes.fromhex(c["proofs"]), bytes(c["proof_len"]), bytes.fromhex(c["root"])]
        for mis_in in (0, 1 + k % 3):
            (st,) = _exec(harness, tmp_path, "verify", (c["leaf_format"], c["addr_format"], m, m, c["depth"], mis_in, 3, 0), arrays, [m])
            assert list(st) == c["status"], (c["tree"], [w for w, a, b in zip(c["what"], st, c["status"]) if a != b])


def _sizes():
    return sorted({n for k in range(1, 12) for n in (2**k - 1, 2**k, 2**k + 1)})


def test_sizes_around_every_power_of_two(harness, tmp_path):
    rng = np.random.default_rng(20261018)
    for n in _sizes():
        leaves = [rng.bytes(32) for _ in range(n)]
        if n > 4:
            leaves[n // 2] = leaves[1]                                        # a duplicate: the index breaks the tie
            leaves[-1] = leaves[0][:31] + bytes([leaves[0][31] ^ 1])          # ... and a pair that differs in its last bit only
        for sort in ((True, False) if n <= 33 or n == 2049 else (True,)):
            want_tree, want_pos = M.build(leaves, sort)
            tree, pos = _build(harness, tmp_path, b"".join(leaves), sort, mis_in=n % 4, mis_out=1 + n % 15)
            assert pos == want_pos, (n, sort)
            assert tree == b"".join(want_tree), (n, sort)
        if n in (1, 3, 64, 1025, 2049):                                        # every leaf's proof, and back through verify with one mutant each
            depth = M.max_proof_len(n)
            proof, ln = _exec(harness, tmp_path, "proof", (0, 0, n, n, depth, 1, 3, 0), [tree, np.array(pos, np.uint32).tobytes()], [32 * depth * n, n])
            wp, wl = M.proof_batch(want_tree, want_pos, depth)
            assert proof == wp.tobytes() and ln == wl.tobytes(), n
            mut = bytearray(proof)
            for j in range(n):
                if ln[j]:
                    mut[32 * depth * j + 32 * (j % ln[j]) + j % 32] ^= 1 << (j % 8)
            for prf, want in ((proof, 1), (bytes(mut), 0)):
                (st,) = _exec(harness, tmp_path, "verify", (M.LEAF_HASH32, 0, n, n, depth, 2, 1, 0), [b"".join(leaves), prf, ln, want_tree[0]], [n])
                assert list(st) == [want if ln[j] or want else 1 for j in range(n)], (n, want)
