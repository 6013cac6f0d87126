#!/usr/bin/env python3
"""Writes tests/golden/hd_kats.json: what the key-derivation tests pin (python tests/golden/make_hd_kats.py).  "known": BIP-32's test vector 1 (seed, the values and the
base58 strings of m, m/0', m/0'/1) and the Hardhat / Anvil default accounts (the BIP-39 seed of the mnemonic, the node m/44'/60'/0'/0, children 0 - 2 with their
addresses), as published -- while writing the file this script ASSERTS that the restatement of tests/_hd.py reproduces every one of them, that the strings' checksums hold
and that the public form agrees.  "batches": seeded batches through the restatement's batch functions (parents, paths with the index edges, hardened and not, both forms,
invalid parents planted), one row per item, so that a change of the restatement shows as a change of this file."""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
from tests import _hd as H  # noqa: E402
from tests import _keccak as K  # noqa: E402


def known():
    m = H.master(H.V1_SEED)
    assert (H.b32(m[0]).hex(), m[1].hex()) == H.V1["m"][:2]
    for depth, (path, (sk, chain, xprv)) in enumerate(H.V1.items()):
        private, d, child, c, key = H.parse_xkey(xprv)                      # (raises on a checksum that fails)
        assert private and (d, c.hex(), key.hex()) == (depth, chain, sk) and child == (0, H.H, 1)[depth]
        if depth:
            k, c2 = H.derive(m[0], m[1], path)
            assert (H.b32(k).hex(), c2.hex()) == (sk, chain)
    k0, c0 = int(H.V1["m/0'"][0], 16), bytes.fromhex(H.V1["m/0'"][1])
    Kc, cc = H.ckd_pub(H.g_mul(k0), c0, 1)
    assert Kc == H.g_mul(int(H.V1["m/0'/1"][0], 16)) and cc.hex() == H.V1["m/0'/1"][1]
    seed = H.hardhat_seed()
    assert seed.hex() == H.HARDHAT_SEED
    hm = H.master(seed)
    acct = H.derive(hm[0], hm[1], H.HARDHAT_ACCOUNT_PATH)
    assert (H.b32(acct[0]).hex(), acct[1].hex()) == H.HARDHAT_ACCOUNT
    for i, (sk, addr) in enumerate(H.HARDHAT_CHILDREN):
        k, c = H.ckd_priv(acct[0], acct[1], i)
        assert H.b32(k).hex() == sk and K.address_of(H.g_mul(k)).hex() == addr
        assert H.derive(hm[0], hm[1], f"{H.HARDHAT_ACCOUNT_PATH}/{i}") == (k, c) and H.ckd_pub(H.g_mul(acct[0]), acct[1], i) == (H.g_mul(k), c)
    return {"bip32_vector_1": {"seed": H.V1_SEED.hex(), "nodes": [{"path": p, "sk": v[0], "chain": v[1], "xprv": v[2]} for p, v in H.V1.items()]},
            "hardhat": {"mnemonic": H.HARDHAT_MNEMONIC.decode(), "seed": H.HARDHAT_SEED, "account_path": H.HARDHAT_ACCOUNT_PATH, "account_sk": H.HARDHAT_ACCOUNT[0],
                        "account_chain": H.HARDHAT_ACCOUNT[1], "children": [{"index": i, "sk": sk, "address": a} for i, (sk, a) in enumerate(H.HARDHAT_CHILDREN)]}}


def batch(n, depth, seed):
    sk, chain = H.seeded_nodes(n, seed)
    for j, v in enumerate((0, H.N, 2**256 - 1)):
        sk[2 + 5 * j] = np.frombuffer(H.b32(v), np.uint8)
    path = H.seeded_paths(n, depth, seed + 1)
    priv = H.derive_priv_batch(sk, chain, path, depth, 0, "sec1", "raw20")
    ppath = path & np.uint32(0x7FFFFFFF)
    ppath[1, depth - 1] = H.H + 7
    pk = H.pk_of(np.where((sk == 0).all(axis=1, keepdims=True) | (sk[:, :1] >= 0x80), np.uint8(1), sk), "sec1")
    pk[4] = np.frombuffer(b"\x04" + bytes(pk[4, 1:]), np.uint8)
    pub = H.derive_pub_batch(pk, chain, ppath, depth, 0, "sec1", "raw20")
    hx = lambda a: bytes(a).hex()  # noqa: E731
    return {"depth": depth, "items": [{"sk": hx(sk[i]), "chain": hx(chain[i]), "path": [int(x) for x in path[i]],
                                       "priv": {"sk": hx(priv[0][i]), "chain": hx(priv[1][i]), "pk": hx(priv[2][i]), "address": hx(priv[3][i]), "status": int(priv[4][i])},
                                       "pk": hx(pk[i]), "pub_path": [int(x) for x in ppath[i]],
                                       "pub": {"pk": hx(pub[0][i]), "chain": hx(pub[1][i]), "address": hx(pub[2][i]), "status": int(pub[3][i])}} for i in range(n)]}


def main():
    seeds = np.random.default_rng(17).integers(0, 256, (6, 64), dtype=np.uint8)
    masters = []
    for j, ln in enumerate((16, 24, 32, 33, 63, 64)):
        sk, chain, st = H.master_batch(seeds[j:j + 1, :ln], ln)
        masters.append({"seed": bytes(seeds[j, :ln]).hex(), "sk": bytes(sk[0]).hex(), "chain": bytes(chain[0]).hex(), "status": int(st[0])})
    doc = {"known": known(), "masters": masters, "batches": [batch(16, 1, 1701), batch(16, 5, 1705), batch(16, 8, 1708)]}
    (Path(__file__).resolve().parent / "hd_kats.json").write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
