"""A restatement of the Merkle calls of include/plume_hip.h (plume_merkle_*) in plain Python over tests/_keccak.py, shared by the Merkle tests.  The tree is the one
OpenZeppelin's StandardMerkleTree builds and MerkleProof.verify checks: double-hashed ABI-encoded leaves, sorted by hash, nodes Keccak-256 of the two children in sorted
order, the whole tree one array of 2n - 1 nodes with the leaves at its end in reverse.  Nothing here is taken from the library's code."""
import json
from pathlib import Path

import numpy as np

from tests import _keccak as K

LEAF_HASH32, LEAF_ADDRESS, LEAF_ADDRESS_UINT256 = 0, 1, 2
ADDR_RAW20, ADDR_RECORD64, ADDR_EIP55 = 0, 1, 2
SORT_LEAVES = 1
MISMATCH, MATCH, INVALID = 0, 1, 3
BAD_LEN = 255
ITEM_WIDTH = {ADDR_RAW20: 20, ADDR_RECORD64: 64}
GOLDEN = Path(__file__).resolve().parent / "golden" / "merkle_kats.json"


def _nodes(hexstr):
    b = bytes.fromhex(hexstr)
    return [b[k:k + 32] for k in range(0, len(b), 32)]


def _slots(tree, idx_lists, depth):
    """proofs written as lists of tree indices -> (proof bytes in `depth` slots, lengths); None: a refused request"""
    out = np.zeros((len(idx_lists), depth, 32), np.uint8)
    for k, idx in enumerate(idx_lists):
        for s, t in enumerate(idx or []):
            out[k, s] = np.frombuffer(tree[t], np.uint8)
    return out, [BAD_LEN if idx is None else len(idx) for idx in idx_lists]


def load_kats():
    """the committed vectors as the tests use them: {"oz_root", "trees": [{name, leaf_format, addr_format, sort, n, items, amounts, leaves, leaf_status, tree, leaf_pos,
    depth, proofs, proof_len}], "proof_cases": [{tree, depth, pos, proofs, proof_len}], "verify_cases": [{tree, leaf_format, addr_format, depth, what, items, amounts,
    proofs, proof_len, root, status}]}, byte arrays as hex strings.  The file says every node once: a proof is a list of tree indices, a 64-byte record its 20 address
    bytes (and its head where that is not zero), a leaf is tree[leaf_pos], and a verify item is (item of the tree, proof_len, one flipped bit) over that item's proof
    with 0xA5 in the slots behind it: all undone here"""
    kats = json.loads(GOLDEN.read_text())
    by = {}
    for t in kats["trees"]:
        n, tree = t["n"], _nodes(t["tree"])
        if t["leaf_format"] != LEAF_HASH32 and t["addr_format"] == ADDR_RECORD64:
            heads, a = t.pop("heads", {}), bytes.fromhex(t["items"])
            t["items"] = b"".join(bytes.fromhex(heads.get(str(j), "00" * 44)) + a[20 * j:20 * j + 20] for j in range(n)).hex()
        t["leaves"] = b"".join(tree[p] for p in t["leaf_pos"]).hex()
        proof, t["proof_len"] = _slots(tree, t.pop("proof_idx"), t["depth"])
        t["proofs"] = proof.tobytes().hex()
        by[t["name"]] = t
    for c in kats["proof_cases"]:
        proof, c["proof_len"] = _slots(_nodes(by[c["tree"]]["tree"]), c.pop("proof_idx"), c["depth"])
        c["proofs"] = proof.tobytes().hex()
    for c in kats["verify_cases"]:
        if "rows" not in c:
            continue
        t = by[c["tree"]]
        W, base = item_width(t["leaf_format"], t["addr_format"]), np.frombuffer(bytes.fromhex(t["proofs"]), np.uint8).reshape(t["n"], t["depth"], 32)
        items, amounts, proofs = bytes.fromhex(t["items"]), None if t["amounts"] is None else bytes.fromhex(t["amounts"]), []
        rows = c.pop("rows")
        for what, j, ln, mut in rows:
            p = np.full((c["depth"], 32), 0xA5, np.uint8)
            p[:t["depth"]] = base[j]
            if mut:
                p[mut[0], mut[1]] ^= mut[2]
            proofs.append(p)
        c.update(leaf_format=t["leaf_format"], addr_format=t["addr_format"], what=[r[0] for r in rows], proof_len=[r[2] for r in rows], root=t["tree"][:64],
                 items=b"".join(items[W * r[1]:W * r[1] + W] for r in rows).hex(), amounts=None if amounts is None else b"".join(amounts[32 * r[1]:32 * r[1] + 32] for r in rows).hex(),
                 proofs=np.stack(proofs).tobytes().hex())
    return kats


def item_width(leaf_format, addr_format):
    return 32 if leaf_format == LEAF_HASH32 else ITEM_WIDTH[addr_format]


def leaf_of(leaf_format, addr_format, item, amount=None):
    """the 32-byte leaf of one input item, or None when the item is invalid (a RECORD64 whose first 44 bytes are not zero).  amount: an integer below 2^256 or 32 bytes"""
    item = bytes(item)
    if leaf_format == LEAF_HASH32:
        assert len(item) == 32
        return item
    assert len(item) == ITEM_WIDTH[addr_format]
    if addr_format == ADDR_RECORD64:
        if any(item[:44]):
            return None
        item = item[44:]
    enc = bytes(12) + item                                     # abi.encode(address): left-padded to 32 bytes
    if leaf_format == LEAF_ADDRESS_UINT256:
        enc += amount.to_bytes(32, "big") if isinstance(amount, int) else bytes(amount)
        assert len(enc) == 64
    return K.keccak256(K.keccak256(enc))


def leaf_batch(leaf_format, addr_format, items, amounts=None):
    """(leaf uint8[n, 32], status uint8[n]): an invalid item has status 3 and the zero leaf"""
    n = len(items)
    leaf, status = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
    for i in range(n):
        h = leaf_of(leaf_format, addr_format, items[i], None if amounts is None else amounts[i])
        status[i] = INVALID if h is None else MATCH
        if h is not None:
            leaf[i] = np.frombuffer(h, np.uint8)
    return leaf, status


def hash_pair(a, b):
    a, b = bytes(a), bytes(b)
    return K.keccak256(a + b if a <= b else b + a)            # bytes compare lexicographically: big-endian numbers


def build(leaves, sort=True):
    """(tree: list of 2n - 1 nodes, leaf_pos: list of n tree indices) for n >= 1 leaves of 32 bytes"""
    leaves = [bytes(x) for x in leaves]
    n = len(leaves)
    assert n >= 1 and all(len(x) == 32 for x in leaves)
    order = sorted(range(n), key=lambda j: (leaves[j], j)) if sort else list(range(n))
    tree = [None] * (2 * n - 1)
    leaf_pos = [0] * n
    for i, j in enumerate(order):
        tree[2 * n - 2 - i] = leaves[j]
        leaf_pos[j] = 2 * n - 2 - i
    for i in range(n - 2, -1, -1):
        tree[i] = hash_pair(tree[2 * i + 1], tree[2 * i + 2])
    return tree, leaf_pos


def proof(tree, t):
    out = []
    while t > 0:
        out.append(tree[t + 1 if t & 1 else t - 1])
        t = (t - 1) // 2
    return out


def max_proof_len(n):
    return (2 * n - 1).bit_length() - 1


def proof_batch(tree, pos, depth):
    """(proof uint8[m, depth, 32], proof_len uint8[m]): an index outside the tree or a proof longer than depth gives 255 and zero slots"""
    m = len(pos)
    out, ln = np.zeros((m, depth, 32), np.uint8), np.zeros(m, np.uint8)
    for k, t in enumerate(pos):
        t = int(t)
        if not 0 <= t < len(tree) or (t + 1).bit_length() - 1 > depth:
            ln[k] = BAD_LEN
            continue
        p = proof(tree, t)
        assert len(p) == (t + 1).bit_length() - 1
        ln[k] = len(p)
        for s, e in enumerate(p):
            out[k, s] = np.frombuffer(e, np.uint8)
    return out, ln


def process_proof(leaf, prf):
    h = bytes(leaf)
    for p in prf:
        h = hash_pair(h, p)
    return h


def verify_batch(leaf_format, addr_format, items, amounts, depth, prf, proof_len, root):
    """status uint8[m]: 1 the proof leads to root, 0 it does not, 3 an invalid item or proof_len[k] > depth"""
    m = len(items)
    prf = np.asarray(prf, np.uint8).reshape(m, depth, 32)
    st = np.zeros(m, np.uint8)
    for k in range(m):
        h = leaf_of(leaf_format, addr_format, items[k], None if amounts is None else amounts[k])
        if h is None or int(proof_len[k]) > depth:
            st[k] = INVALID
            continue
        st[k] = MATCH if process_proof(h, [prf[k, s].tobytes() for s in range(int(proof_len[k]))]) == bytes(root) else MISMATCH
    return st
