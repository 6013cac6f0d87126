#!/usr/bin/env python3
"""Writes tests/golden/merkle_kats.json: the trees, proofs and verdicts the Merkle tests pin (python tests/golden/make_merkle_kats.py).  Everything is made by the
restatement in tests/_merkle.py from fixed seeds, so the file is reproducible; while writing it this script ASSERTS the root published in the README of
@openzeppelin/merkle-tree for its two-row ["address", "uint256"] example.
"trees": n = 1, 2, 3, 5, 8, 13 in the three leaf formats, sorted (addresses as 20 raw bytes) and unsorted (as 64-byte records); 13 leaves with duplicates; leaves that share
their first 8 and their first 28 bytes (HASH32, chosen here); two and four equal leaves (equal children at both levels); records with a non-zero head.  Each holds the
items, the leaves and their status, the whole tree, leaf_pos, and the proof of every input item in `depth` slots.
"proof_cases": indices of any node, indices outside the tree, a depth that is too small for some of them.
"verify_cases": every proof of a tree, a wrong sibling at each position, a truncated proof, an empty proof with leaf == root, a proof_len above depth, an invalid record.
The file is kept small by saying every node once (compact() below; tests/_merkle.load_kats undoes it, and this script checks that it does): proofs are lists of tree
indices, a 64-byte record is its address and its head where that is not zero, a verify item is a row (item, proof_len, flipped bit) over a tree of the file."""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
from tests import _keccak as K  # noqa: E402
from tests import _merkle as M  # noqa: E402

OZ_ROOT = "d4dee0beab2d53f2cc83e567171bd2820e49898130a22622b10ead383e90bd77"


def h(tag, j):
    return K.keccak256(b"merkle kats %s %d" % (tag.encode(), j))


def hx(a):
    return np.asarray(a, np.uint8).tobytes().hex()


def make_tree(name, leaf_format, addr_format, sort, items, amounts=None):
    leaves, status = M.leaf_batch(leaf_format, addr_format, items, amounts)
    tree, leaf_pos = M.build([x.tobytes() for x in leaves], sort)
    depth = M.max_proof_len(len(items))
    proof, proof_len = M.proof_batch(tree, leaf_pos, depth)
    for j in range(len(items)):                                               # every proof leads to the root
        assert M.process_proof(leaves[j].tobytes(), [proof[j, s].tobytes() for s in range(proof_len[j])]) == tree[0], (name, j)
    return {"name": name, "leaf_format": leaf_format, "addr_format": addr_format, "sort": int(sort), "n": len(items), "items": b"".join(items).hex(),
            "amounts": None if amounts is None else b"".join(a.to_bytes(32, "big") for a in amounts).hex(), "leaves": hx(leaves), "leaf_status": [int(x) for x in status],
            "tree": b"".join(tree).hex(), "leaf_pos": leaf_pos, "depth": depth, "proofs": hx(proof), "proof_len": [int(x) for x in proof_len]}


def _walk(tree, t):
    """the tree indices of the proof of node t"""
    idx = []
    while t > 0:
        idx.append(t + 1 if t & 1 else t - 1)
        t = (t - 1) // 2
    return idx


def compact(full):
    """the form the file holds (tests/_merkle.load_kats undoes it): every node once"""
    out = {"oz_root": full["oz_root"], "trees": [], "proof_cases": [], "verify_cases": []}
    by = {}
    for t in full["trees"]:
        n = t["n"]
        c = {k: t[k] for k in ("name", "leaf_format", "addr_format", "sort", "n", "items", "amounts", "leaf_status", "tree", "leaf_pos", "depth")}
        if t["leaf_format"] != M.LEAF_HASH32 and t["addr_format"] == M.ADDR_RECORD64:
            raw = bytes.fromhex(t["items"])
            c["items"] = b"".join(raw[64 * j + 44:64 * j + 64] for j in range(n)).hex()
            heads = {str(j): raw[64 * j:64 * j + 44].hex() for j in range(n) if any(raw[64 * j:64 * j + 44])}
            if heads:
                c["heads"] = heads
        c["proof_idx"] = [_walk(None, p) for p in t["leaf_pos"]]
        out["trees"].append(c)
        by[t["name"]] = t
    for p in full["proof_cases"]:
        out["proof_cases"].append({"tree": p["tree"], "depth": p["depth"], "pos": p["pos"],
                                   "proof_idx": [None if ln == M.BAD_LEN else _walk(None, t) for t, ln in zip(p["pos"], p["proof_len"])]})
    for v in full["verify_cases"]:
        out["verify_cases"].append({"tree": v["tree"], "depth": v["depth"], "rows": v["_rows"], "status": v["status"]} if "_rows" in v else v)
    return out


def main():
    out = {"oz_root": OZ_ROOT}
    oz_items = [bytes([0x11]) * 20, bytes([0x22]) * 20]
    oz_amounts = [5000000000000000000, 2500000000000000000]
    trees = [make_tree("openzeppelin readme", M.LEAF_ADDRESS_UINT256, M.ADDR_RAW20, True, oz_items, oz_amounts)]
    assert trees[0]["tree"][:64] == OZ_ROOT, trees[0]["tree"][:64]
    for n in (1, 2, 3, 5, 8, 13):
        for lf, tag in ((M.LEAF_HASH32, "hash32"), (M.LEAF_ADDRESS, "address"), (M.LEAF_ADDRESS_UINT256, "address_uint256")):
            for sort, af in ((True, M.ADDR_RAW20), (False, M.ADDR_RECORD64)):
                addrs = [h(f"{tag} {n}", j)[:20] for j in range(n)]
                items = [h(f"{tag} {n}", j) for j in range(n)] if lf == M.LEAF_HASH32 else addrs if af == M.ADDR_RAW20 else [bytes(44) + a for a in addrs]
                amounts = [int.from_bytes(h("amount", 100 * n + j), "big") >> (8 * (j % 32)) for j in range(n)] if lf == M.LEAF_ADDRESS_UINT256 else None
                trees.append(make_tree(f"{tag} n={n} {'sorted' if sort else 'input order'}", lf, af, sort, items, amounts))
    dup = [h("dup", j % 5) for j in range(13)]
    trees.append(make_tree("13 leaves, five values", M.LEAF_HASH32, M.ADDR_RAW20, True, dup))
    trees.append(make_tree("13 leaves, five values, input order", M.LEAF_HASH32, M.ADDR_RAW20, False, dup))
    trees.append(make_tree("first 8 bytes shared", M.LEAF_HASH32, M.ADDR_RAW20, True, [h("p8", 0)[:8] + h("p8 tail", j)[:24] for j in range(11)]))
    trees.append(make_tree("first 28 bytes shared", M.LEAF_HASH32, M.ADDR_RAW20, True, [h("p28", 0)[:28] + h("p28 tail", j)[:4] for j in range(11)]))
    trees.append(make_tree("last byte decides", M.LEAF_HASH32, M.ADDR_RAW20, True, [h("p31", 0)[:31] + bytes([(7 * j + 3) % 256]) for j in range(9)]))
    trees.append(make_tree("two equal leaves", M.LEAF_HASH32, M.ADDR_RAW20, True, [h("eq", 0)] * 2))
    trees.append(make_tree("four equal leaves", M.LEAF_HASH32, M.ADDR_RAW20, True, [h("eq", 1)] * 4))
    trees.append(make_tree("all-ones and zero leaves", M.LEAF_HASH32, M.ADDR_RAW20, True, [b"\xff" * 32, bytes(32), b"\xff" * 32, h("ones", 0), b"\xff" * 31 + b"\xfe"]))
    bad = []
    for j, at in enumerate((0, 1, 15, 16, 31, 43, None, None)):                   # a record whose head is not zero has no leaf
        rec = bytearray(bytes(44) + h("badrec", j)[:20])
        if at is not None:
            rec[at] = 0x80 >> (j % 8)
        bad.append(bytes(rec))
    trees.append(make_tree("records with a non-zero head", M.LEAF_ADDRESS, M.ADDR_RECORD64, True, bad))
    trees.append(make_tree("records with a non-zero head, with amounts", M.LEAF_ADDRESS_UINT256, M.ADDR_RECORD64, False, bad, list(range(1, 9))))
    assert trees[-1]["leaf_status"] == [3] * 6 + [1, 1]
    out["trees"] = trees
    by = {t["name"]: t for t in trees}

    def nodes(t):
        b = bytes.fromhex(t["tree"])
        return [b[k:k + 32] for k in range(0, len(b), 32)]

    cases = []
    for name, depth in (("hash32 n=13 sorted", 4), ("hash32 n=13 sorted", 3), ("hash32 n=13 sorted", 0), ("hash32 n=5 sorted", 5), ("address n=5 input order", 2),
                        ("hash32 n=1 sorted", 0), ("hash32 n=1 sorted", 2)):
        t = by[name]
        total = 2 * t["n"] - 1
        pos = list(range(total)) + [total, total + 1, 2**31, 2**32 - 1, 2 * total]
        proof, ln = M.proof_batch(nodes(t), pos, depth)
        cases.append({"tree": name, "depth": depth, "pos": pos, "proofs": hx(proof), "proof_len": [int(x) for x in ln]})
    assert any(M.BAD_LEN in c["proof_len"][:2 * by[c["tree"]]["n"] - 1] for c in cases)
    out["proof_cases"] = cases

    vcases = []
    for name in ("openzeppelin readme", "address_uint256 n=5 sorted", "address n=3 input order", "hash32 n=8 sorted", "four equal leaves",
                 "records with a non-zero head"):
        t = by[name]
        n, depth, W = t["n"], t["depth"] + 1, M.item_width(t["leaf_format"], t["addr_format"])   # one slot more than needed: unused slots hold junk here
        items = bytes.fromhex(t["items"])
        items = [items[W * j:W * j + W] for j in range(n)]
        amounts = None if t["amounts"] is None else [bytes.fromhex(t["amounts"])[32 * j:32 * j + 32] for j in range(n)]
        base = np.frombuffer(bytes.fromhex(t["proofs"]), np.uint8).reshape(n, t["depth"], 32)
        rows = []                                                               # (what, item index, proof array, proof_len)
        for j in range(n):
            p = np.full((depth, 32), 0xA5, np.uint8)
            p[:t["depth"]] = base[j]
            ln = t["proof_len"][j]
            rows.append(("valid", j, p, ln, None))
            if t["leaf_status"][j] != M.MATCH and j > 0:                        # (an invalid record is invalid whatever comes with it: one set of mutants is enough)
                continue
            for s in range(ln):                                                 # a wrong sibling at each position
                q = p.copy()
                q[s, (5 * s + j) % 32] ^= 1 << (s % 8)
                rows.append((f"sibling {s} wrong", j, q, ln, [s, (5 * s + j) % 32, 1 << (s % 8)]))
            if ln:
                rows.append(("truncated", j, p, ln - 1, None))
            rows.append(("one element too many", j, p, ln + 1, None))
            rows.append(("proof_len above depth", j, p, depth + 1, None))
            rows.append(("proof_len 255", j, p, 255, None))
        v_items = [items[j] for _, j, _, _, _ in rows]
        v_amounts = None if amounts is None else [amounts[j] for _, j, _, _, _ in rows]
        v_proof = np.stack([p for _, _, p, _, _ in rows])
        v_len = [ln for _, _, _, ln, _ in rows]
        root = bytes.fromhex(t["tree"][:64])
        st = M.verify_batch(t["leaf_format"], t["addr_format"], v_items, v_amounts, depth, v_proof, v_len, root)
        for (what, j, _, ln, _), s in zip(rows, st):
            ok = t["leaf_status"][j] == M.MATCH
            want = M.INVALID if (not ok or ln > depth) else M.MATCH if what == "valid" else M.MISMATCH
            if what == "one element too many" and ok and ln <= depth:
                want = M.MISMATCH
            assert s == want, (name, what, j, s, want)
        vcases.append({"tree": name, "leaf_format": t["leaf_format"], "addr_format": t["addr_format"], "depth": depth, "what": [w for w, _, _, _, _ in rows], "_rows": [[w, j, ln, mut] for w, j, _, ln, mut in rows],
                       "items": b"".join(v_items).hex(), "amounts": None if v_amounts is None else b"".join(v_amounts).hex(), "proofs": hx(v_proof), "proof_len": v_len,
                       "root": root.hex(), "status": [int(x) for x in st]})
    # an empty proof: the leaf is the root (a tree of one leaf, and any 32 bytes against themselves); depth 0, no proof array at all
    one = by["address n=1 sorted"]
    vcases.append({"tree": one["name"], "leaf_format": one["leaf_format"], "addr_format": one["addr_format"], "depth": 0, "what": ["leaf == root", "another address"],
                   "items": one["items"] + h("other", 0)[:20].hex(), "amounts": None, "proofs": "", "proof_len": [0, 0], "root": one["tree"][:64], "status": [1, 0]})
    r = h("root", 0)
    vcases.append({"tree": None, "leaf_format": M.LEAF_HASH32, "addr_format": M.ADDR_RAW20, "depth": 2, "what": ["leaf == root", "leaf != root", "proof_len 3"],
                   "items": (r + h("root", 1) + r).hex(), "amounts": None, "proofs": bytes(3 * 2 * 32).hex(), "proof_len": [0, 0, 3], "root": r.hex(), "status": [1, 0, 3]})
    for c in vcases[-2:]:
        W = M.item_width(c["leaf_format"], c["addr_format"])
        it = bytes.fromhex(c["items"])
        got = M.verify_batch(c["leaf_format"], c["addr_format"], [it[W * k:W * k + W] for k in range(len(c["status"]))], None, c["depth"],
                             np.frombuffer(bytes.fromhex(c["proofs"]), np.uint8), c["proof_len"], bytes.fromhex(c["root"]))
        assert list(got) == c["status"], c["what"]
    out["verify_cases"] = vcases
    path = ROOT / "tests" / "golden" / "merkle_kats.json"
    path.write_text(json.dumps(compact(out), separators=(",", ":")) + "\n")
    back = M.load_kats()
    for c in out["verify_cases"]:
        c.pop("_rows", None)
    assert back == json.loads(json.dumps(out)), "the file does not expand to what was made"
    print(path, path.stat().st_size, "bytes;", len(trees), "trees,", sum(len(c["pos"]) for c in cases), "proof requests,", sum(len(c["status"]) for c in vcases), "verify items")


if __name__ == "__main__":
    main()
