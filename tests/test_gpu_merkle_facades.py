"""The façades of the Merkle calls: Engine.merkle_tree and its MerkleTree object, the single-item merkle_leaf / merkle_root / merkle_proof / merkle_verify and
PlumeSignature.verify_for_root in Python (zk-nullifier-sig_amd/capi.py, plume.py), and the same names in C++ (include/plume.hpp, tests/abi_cpp/merkle_test.cpp), against the
restatement of tests/_merkle.py and the root published in the README of @openzeppelin/merkle-tree."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import _keccak as K
from tests import _merkle as M

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
OZ_ROOT = "d4dee0beab2d53f2cc83e567171bd2820e49898130a22622b10ead383e90bd77"
OZ = [(bytes([0x11]) * 20, 5000000000000000000), (bytes([0x22]) * 20, 2500000000000000000)]


def _addresses(n):
    return [K.keccak256(b"merkle facade %d" % j)[:20] for j in range(n)]


def test_python_facades():
    import zk_nullifier_sig_amd as plume
    eng = plume.Engine(0)
    try:
        t = eng.merkle_tree(np.frombuffer(b"".join(a for a, _ in OZ), np.uint8).reshape(2, 20), [v for _, v in OZ])
        assert t.root.hex() == OZ_ROOT and t.n == 2 and t.tree.shape == (3, 32) and sorted(t.leaf_pos) == [1, 2]
        for j, (a, v) in enumerate(OZ):
            assert plume.merkle_leaf(a, v, eng) == M.leaf_of(M.LEAF_ADDRESS_UINT256, M.ADDR_RAW20, a, v)
            assert plume.merkle_verify(a, t.proof(j), t.root, v, eng) and not plume.merkle_verify(a, t.proof(j), t.root, v + 1, eng)
            assert not plume.merkle_verify(a, t.proof(j), t.root, None, eng) and not plume.merkle_verify(a, t.proof(1 - j), t.root, v, eng)
        addrs = _addresses(11)
        leaves = [M.leaf_of(M.LEAF_ADDRESS, M.ADDR_RAW20, a) for a in addrs]
        want_tree, want_pos = M.build(leaves, sort=True)
        assert plume.merkle_leaf(addrs[3], None, eng) == leaves[3]
        for t in (eng.merkle_tree(addrs), eng.merkle_tree(np.frombuffer(b"".join(bytes(44) + a for a in addrs), np.uint8).reshape(11, 64), addr_format="record64"),
                  eng.merkle_tree(leaves)):
            assert t.root == want_tree[0] and list(t.leaf_pos) == want_pos and t.tree.tobytes() == b"".join(want_tree) and t.depth == 4
            proof, ln = t.proofs()
            wp, wl = M.proof_batch(want_tree, want_pos, 4)
            assert np.array_equal(proof, wp) and np.array_equal(ln, wl)
            assert t.proof(6) == M.proof(want_tree, want_pos[6]) and np.array_equal(t.proofs([6, 2])[0], wp[[6, 2]])
        assert plume.merkle_root(leaves, True, eng) == want_tree[0] and plume.merkle_root(leaves, False, eng) == M.build(leaves, sort=False)[0][0]
        assert plume.merkle_proof(leaves, 9, True, eng) == M.proof(want_tree, want_pos[9])
        assert plume.merkle_verify(leaves[9], M.proof(want_tree, want_pos[9]), want_tree[0], engine=eng) and plume.merkle_verify(addrs[9], M.proof(want_tree, want_pos[9]), want_tree[0], engine=eng)
        assert not plume.merkle_verify(leaves[8], M.proof(want_tree, want_pos[9]), want_tree[0], engine=eng)
        assert plume.merkle_verify(want_tree[0], [], want_tree[0], engine=eng) and not plume.merkle_verify(leaves[0], [bytes(32)] * 65, want_tree[0], engine=eng)
        with pytest.raises(ValueError):
            eng.merkle_tree(np.ones((2, 64), np.uint8), addr_format="record64", leaf_format="address")

        # a signer on the list: pk -> address -> leaf -> proof
        class Rng:
            def fill_bytes(self, k):
                return bytes.fromhex("93b9323b629f251b8f3fc2dd11f4672c5544e8230d493eceea98a90bda789808")
        sk = plume.SecretKey.from_bytes(bytes.fromhex("519b423d715f8b581f4fa8ee59f4771a5b44c8130b4e3eacca54a56dda72b464"))
        sig = plume.PlumeSignature.sign_v1(sk, b"An example app message string", Rng(), eng)
        me = sig.eth_address(eng)
        members = addrs[:6] + [me] + addrs[6:]
        t = eng.merkle_tree(members)
        assert sig.verify_for_root(t.root, t.proof(6), engine=eng) and not sig.verify_for_root(t.root, t.proof(5), engine=eng)
        assert not sig.verify_for_root(eng.merkle_tree(addrs).root, t.proof(6), engine=eng)
        ta = eng.merkle_tree(members, [100 + j for j in range(12)])
        assert sig.verify_for_root(ta.root, ta.proof(6), 106, eng) and not sig.verify_for_root(ta.root, ta.proof(6), 107, eng) and not sig.verify_for_root(ta.root, ta.proof(6), engine=eng)
    finally:
        eng.close()


def test_cpp_facade(tmp_path):
    import zk_nullifier_sig_amd as plume
    rows = []
    for a, v in OZ:
        rows.append(("leaf", a.hex(), v.to_bytes(32, "big").hex(), M.leaf_of(M.LEAF_ADDRESS_UINT256, M.ADDR_RAW20, a, v).hex()))
    addrs = _addresses(7)
    rows += [("leaf", a.hex(), "-", M.leaf_of(M.LEAF_ADDRESS, M.ADDR_RAW20, a).hex()) for a in addrs[:2]]
    for n, sort in ((1, True), (2, True), (5, True), (7, False), (7, True)):
        leaves = [M.leaf_of(M.LEAF_ADDRESS, M.ADDR_RAW20, a) for a in addrs[:n]]
        rows.append(("tree", str(int(sort)), M.build(leaves, sort)[0][0].hex()) + tuple(x.hex() for x in leaves))
    oz_leaves = [M.leaf_of(M.LEAF_ADDRESS_UINT256, M.ADDR_RAW20, a, v) for a, v in OZ]
    tree, pos = M.build(oz_leaves)
    assert tree[0].hex() == OZ_ROOT
    rows += [("member", OZ_ROOT, a.hex(), v.to_bytes(32, "big").hex()) + tuple(p.hex() for p in M.proof(tree, pos[j])) for j, (a, v) in enumerate(OZ)]
    leaves = [M.leaf_of(M.LEAF_ADDRESS, M.ADDR_RAW20, a) for a in addrs]
    tree, pos = M.build(leaves)
    rows.append(("member", tree[0].hex(), addrs[4].hex(), "-") + tuple(p.hex() for p in M.proof(tree, pos[4])))
    vectors = tmp_path / "vectors.txt"
    vectors.write_text("".join(" ".join(r) + "\n" for r in rows))
    exe = tmp_path / "merkle_test"
    libdir = plume.library_path().parent
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"), str(ROOT / "tests" / "abi_cpp" / "merkle_test.cpp"), "-L", str(libdir),
                    "-lplume_hip", f"-Wl,-rpath,{libdir}", "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe), str(vectors)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "merkle_test ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
