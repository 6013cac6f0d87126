"""The restatement the Merkle tests compare against (tests/_merkle.py) on the CPU.  Its independent pin is the root published in the README of @openzeppelin/merkle-tree
for the two-row ["address", "uint256"] example, a literal here: it fixes the double hash, the ABI encoding and the sorted pair.  The array layout for n > 2 is fixed by the
definition in include/plume_hip.h only.  Every proof the restatement emits passes its own processProof, and any single flipped bit fails; the committed fixture
(tests/golden/merkle_kats.json) says what the restatement says today."""
import numpy as np
import pytest

from tests import _keccak as K
from tests import _merkle as M

OZ_ROOT = "d4dee0beab2d53f2cc83e567171bd2820e49898130a22622b10ead383e90bd77"
OZ_ITEMS = [bytes([0x11]) * 20, bytes([0x22]) * 20]
OZ_AMOUNTS = [5000000000000000000, 2500000000000000000]


def _leaves(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.bytes(32) for _ in range(n)]


def test_the_published_openzeppelin_root():
    leaves, st = M.leaf_batch(M.LEAF_ADDRESS_UINT256, M.ADDR_RAW20, OZ_ITEMS, OZ_AMOUNTS)
    assert list(st) == [M.MATCH, M.MATCH]
    enc = bytes(12) + OZ_ITEMS[0] + OZ_AMOUNTS[0].to_bytes(32, "big")
    assert len(enc) == 64 and leaves[0].tobytes() == K.keccak256(K.keccak256(enc))
    tree, leaf_pos = M.build([x.tobytes() for x in leaves], sort=True)
    assert tree[0].hex() == OZ_ROOT and sorted(leaf_pos) == [1, 2]
    assert tree[2] == min(tree[1], tree[2])                                   # the smallest leaf is the LAST node
    rec, st = M.leaf_batch(M.LEAF_ADDRESS_UINT256, M.ADDR_RECORD64, [bytes(44) + a for a in OZ_ITEMS], OZ_AMOUNTS)
    assert np.array_equal(rec, leaves) and M.load_kats()["oz_root"] == OZ_ROOT


def test_layout_and_proof_lengths():
    for n in (1, 2, 3, 4, 5, 7, 8, 9, 13, 16, 17):
        leaves = _leaves(n, n)
        tree, leaf_pos = M.build(leaves, sort=True)
        assert len(tree) == 2 * n - 1 and [tree[2 * n - 2 - i] for i in range(n)] == sorted(leaves)
        assert all(tree[leaf_pos[j]] == leaves[j] for j in range(n))
        assert all(tree[i] == M.hash_pair(tree[2 * i + 1], tree[2 * i + 2]) for i in range(n - 1))
        lens = {len(M.proof(tree, t)) for t in leaf_pos}
        assert max(lens) == M.max_proof_len(n) and len(lens) == (1 if n & (n - 1) == 0 else 2)
        unsorted, pos = M.build(leaves, sort=False)
        assert pos == [2 * n - 2 - j for j in range(n)]
    dup = [b"\x07" * 32, b"\x03" * 32, b"\x07" * 32, b"\x07" * 32]
    assert M.build(dup)[1] == [5, 6, 4, 3]                                    # equal leaves keep their input order


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 13])
def test_every_proof_verifies_and_any_flipped_bit_fails(n):
    leaves = _leaves(n, 100 + n)
    tree, leaf_pos = M.build(leaves)
    rng = np.random.default_rng(n)
    for j in range(n):
        prf = M.proof(tree, leaf_pos[j])
        assert M.process_proof(leaves[j], prf) == tree[0]
        blob = bytearray(leaves[j] + b"".join(prf))
        for bit in ([int(b) for b in rng.integers(0, 8 * len(blob), 6)] if n > 3 else range(8 * len(blob))):
            m = bytearray(blob)
            m[bit // 8] ^= 1 << (bit % 8)
            assert M.process_proof(bytes(m[:32]), [bytes(m[32 + 32 * s:64 + 32 * s]) for s in range(len(prf))]) != tree[0], (j, bit)
    for t in range(2 * n - 1):                                                # inner nodes have proofs too
        assert M.process_proof(tree[t], M.proof(tree, t)) == tree[0]


def test_the_fixture_is_what_the_restatement_says():
    kats = M.load_kats()
    by = {}
    assert len(kats["trees"]) >= 40
    for t in kats["trees"]:
        W, n = M.item_width(t["leaf_format"], t["addr_format"]), t["n"]
        raw = bytes.fromhex(t["items"])
        items = [raw[W * j:W * j + W] for j in range(n)]
        amounts = None if t["amounts"] is None else [bytes.fromhex(t["amounts"])[32 * j:32 * j + 32] for j in range(n)]
        leaves, st = M.leaf_batch(t["leaf_format"], t["addr_format"], items, amounts)
        assert leaves.tobytes().hex() == t["leaves"] and list(st) == t["leaf_status"], t["name"]
        tree, leaf_pos = M.build([x.tobytes() for x in leaves], bool(t["sort"]))
        assert b"".join(tree).hex() == t["tree"] and leaf_pos == t["leaf_pos"] and t["depth"] == M.max_proof_len(n), t["name"]
        proof, ln = M.proof_batch(tree, leaf_pos, t["depth"])
        assert proof.tobytes().hex() == t["proofs"] and list(ln) == t["proof_len"], t["name"]
        by[t["name"]] = tree
    assert {(t["n"], t["leaf_format"], t["sort"]) for t in kats["trees"]} >= {(n, f, s) for n in (1, 2, 3, 5, 8, 13) for f in (0, 1, 2) for s in (0, 1)}
    for c in kats["proof_cases"]:
        proof, ln = M.proof_batch(by[c["tree"]], c["pos"], c["depth"])
        assert proof.tobytes().hex() == c["proofs"] and list(ln) == c["proof_len"], c["tree"]
    assert any(M.BAD_LEN in c["proof_len"] for c in kats["proof_cases"])
    seen = set()
    for c in kats["verify_cases"]:
        W, m = M.item_width(c["leaf_format"], c["addr_format"]), len(c["status"])
        raw = bytes.fromhex(c["items"])
        amounts = None if c["amounts"] is None else [bytes.fromhex(c["amounts"])[32 * k:32 * k + 32] for k in range(m)]
        got = M.verify_batch(c["leaf_format"], c["addr_format"], [raw[W * k:W * k + W] for k in range(m)], amounts, c["depth"],
                             np.frombuffer(bytes.fromhex(c["proofs"]), np.uint8), c["proof_len"], bytes.fromhex(c["root"]))
        assert list(got) == c["status"], c["tree"]
        seen |= {(w.split()[0], s) for w, s in zip(c["what"], c["status"])}
    assert seen >= {("valid", 1), ("sibling", 0), ("truncated", 0), ("leaf", 1), ("proof_len", 3), ("valid", 3)}
