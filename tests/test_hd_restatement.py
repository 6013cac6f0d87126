"""The restatement the key-derivation tests compare against (tests/_hd.py) pinned to what it did not make: BIP-32's test vector 1 -- the published values AND the published
base58 strings, whose checksums guard the digits --, the Hardhat / Anvil default accounts (mnemonic -> PBKDF2 seed -> m/44'/60'/0'/0/i -> address, the most copied keys
in Ethereum tooling), its point arithmetic held against the oracle's, and the committed fixture (tests/golden/hd_kats.json) it is regenerated from.  CPU only."""
import hashlib
import hmac

import numpy as np
import pytest

from oracle import plume_oracle as O
from tests import _hd as H
from tests import _keccak as K


def test_bip32_vector_1_values_and_strings():
    m = H.master(H.V1_SEED)
    assert (H.b32(m[0]).hex(), m[1].hex()) == H.V1["m"][:2]
    for depth, (path, (sk, chain, xprv)) in enumerate(H.V1.items()):
        private, d, child, c, key = H.parse_xkey(xprv)
        assert private and d == depth and child == (0, H.H, 1)[depth] and c.hex() == chain and key.hex() == sk
        if depth:
            k, c2 = H.derive(m[0], m[1], path)
            assert (H.b32(k).hex(), c2.hex()) == (sk, chain)
        i = len(xprv) // 2
        with pytest.raises(ValueError):                                      # a flipped character does not pass the checksum
            H.parse_xkey(xprv[:i] + ("2" if xprv[i] != "2" else "3") + xprv[i + 1:])
    Kc, cc = H.ckd_pub(H.g_mul(int(H.V1["m/0'"][0], 16)), bytes.fromhex(H.V1["m/0'"][1]), 1)        # CKDpub from (m/0') G with index 1
    assert Kc == H.g_mul(int(H.V1["m/0'/1"][0], 16)) and cc.hex() == H.V1["m/0'/1"][1]


def test_hardhat_accounts_both_ways():
    seed = H.hardhat_seed()
    assert seed.hex() == H.HARDHAT_SEED and len(seed) == 64
    m = H.master(seed)
    acct = H.derive(m[0], m[1], H.HARDHAT_ACCOUNT_PATH)
    assert (H.b32(acct[0]).hex(), acct[1].hex()) == H.HARDHAT_ACCOUNT
    path = np.array([H.parse_path(f"{H.HARDHAT_ACCOUNT_PATH}/{i}") for i in range(3)], np.uint32)
    sk, chain, pk, address, status = H.derive_priv_batch(H.b32(m[0]), m[1], path, 5, H.SHARED_PARENT)
    assert not status.any() and [bytes(r).hex() for r in sk] == [c[0] for c in H.HARDHAT_CHILDREN] and [bytes(r).hex() for r in address] == [c[1] for c in H.HARDHAT_CHILDREN]
    ppk, pchain, paddr, pst = H.derive_pub_batch(H.pk_of(np.frombuffer(H.b32(acct[0]), np.uint8)), acct[1], np.arange(3, dtype=np.uint32).reshape(3, 1), 1, H.SHARED_PARENT)
    assert not pst.any() and np.array_equal(ppk, pk) and np.array_equal(pchain, chain) and np.array_equal(paddr, address)
    assert K.eip55(address[0].tobytes()) == "0xf39Fd6e51aad88F6F4ce6aB8827279cffFb92266"


def test_point_arithmetic_against_the_oracle_and_the_statuses():
    rng = np.random.default_rng(5)
    for _ in range(6):
        k = int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "big") % (H.N - 1) + 1
        assert H.g_mul(k) == tuple(O.pt_mul(k, O.G))
    assert H.g_mul(0) is None and H.g_mul(H.N) is None
    kp = 0x1234567
    assert H.priv_tweak(H.N - 1, kp) == kp - 1 and all(H.priv_tweak(il, kp) is None for il in (H.N, H.N + 1, 2**256 - 1, H.N - kp))
    Kp = H.g_mul(kp)
    assert H.pub_tweak(H.N - kp, Kp) is None and H.pub_tweak(H.N, Kp) is None and H.pub_tweak(kp, Kp) == H.g_mul(2 * kp) and H.pub_tweak(H.N - 1, Kp) == H.g_mul(kp - 1)
    # the batch forms: statuses and zeroing
    sk, chain = H.seeded_nodes(4, 9)
    sk[1] = 0
    sk[2] = 0xFF
    path = np.array([[0], [1], [2], [H.H]], np.uint32)
    out = H.derive_priv_batch(sk, chain, path, 1)
    assert list(out[4]) == [0, H.BAD_SCALAR, H.BAD_SCALAR, 0] and all(not o[1].any() and not o[2].any() for o in out[:4])
    pk = H.pk_of(np.where(out[4][:, None] != 0, np.uint8(3), sk))
    pub = H.derive_pub_batch(pk, chain, path, 1)
    assert list(pub[3]) == [0, 0, 0, H.HARDENED_PUB] and not pub[0][3].any() and not pub[1][3].any() and not pub[2][3].any() and np.array_equal(pub[0][0], out[2][0])
    i_l, i_r = H._I(b"k" * 32, b"d" * 37)
    d = hmac.new(b"k" * 32, b"d" * 37, hashlib.sha512).digest()
    assert H.b32(i_l) + i_r == d


def test_the_committed_fixture_is_what_the_restatement_says():
    doc = H.load_kats()
    v1, hh = doc["known"]["bip32_vector_1"], doc["known"]["hardhat"]
    assert v1["seed"] == H.V1_SEED.hex() and [(n["path"], n["sk"], n["chain"], n["xprv"]) for n in v1["nodes"]] == [(p, *v) for p, v in H.V1.items()]
    assert hh["seed"] == H.HARDHAT_SEED and [(c["sk"], c["address"]) for c in hh["children"]] == list(H.HARDHAT_CHILDREN)
    for e in doc["masters"]:
        seed = bytes.fromhex(e["seed"])
        sk, chain, st = H.master_batch(seed, len(seed))
        assert (bytes(sk[0]).hex(), bytes(chain[0]).hex(), int(st[0])) == (e["sk"], e["chain"], e["status"])
    seen = set()
    for b in doc["batches"]:
        items, depth = b["items"], b["depth"]
        rows = lambda key: np.frombuffer(b"".join(bytes.fromhex(e[key]) for e in items), np.uint8)  # noqa: E731
        priv = H.derive_priv_batch(rows("sk"), rows("chain"), np.array([e["path"] for e in items], np.uint32), depth, 0, "sec1", "raw20")
        pub = H.derive_pub_batch(rows("pk"), rows("chain"), np.array([e["pub_path"] for e in items], np.uint32), depth, 0, "sec1", "raw20")
        for i, e in enumerate(items):
            assert {k: (bytes(v[i]).hex() if k != "status" else int(v[i])) for k, v in zip(("sk", "chain", "pk", "address", "status"), priv)} == e["priv"]
            assert {k: (bytes(v[i]).hex() if k != "status" else int(v[i])) for k, v in zip(("pk", "chain", "address", "status"), pub)} == e["pub"]
            seen |= {e["priv"]["status"], e["pub"]["status"]}
    assert seen == {0, H.BAD_SCALAR, H.HARDENED_PUB}
