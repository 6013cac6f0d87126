"""The restatement the Ethereum-address tests share (tests/_keccak.py): a pure-Python sponge with the domain byte as a parameter.  With 0x06 it must be hashlib's
SHA3-256 on lengths around the 136-byte rate, which pins the permutation and the padding position independently of any Keccak-256 vector; with 0x01 it must give the
public Keccak-256 vectors, the well-known addresses of the secret keys 1, 2, 3 and EIP-55's own examples (tests/golden/eth_address_kats.json).  CPU only."""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

from oracle import plume_oracle as O
from tests import _keccak as K

ROOT = Path(__file__).resolve().parent.parent
KATS = json.loads((ROOT / "tests" / "golden" / "eth_address_kats.json").read_text())


@pytest.mark.parametrize("n", [0, 3, 135, 136, 300])
def test_domain_06_is_sha3_256(n):
    msg = bytes((7 * i + n) & 0xFF for i in range(n))
    assert K.sponge256(msg, 0x06) == hashlib.sha3_256(msg).digest()


def test_keccak256_public_vectors():
    assert len(KATS["keccak256"]) == 2
    for v in KATS["keccak256"]:
        assert K.keccak256(v["msg_utf8"].encode()).hex() == v["digest"]
        assert K.sponge256(v["msg_utf8"].encode(), 0x06).hex() != v["digest"]


def test_addresses_of_the_secret_keys_1_2_3():
    assert [v["sk"] for v in KATS["addresses"]] == [1, 2, 3]
    for v in KATS["addresses"]:
        pk = bytes.fromhex(v["pk"])
        assert pk == O.pt_bytes(O.pt_mul(v["sk"], (O.GX, O.GY))) and bytes.fromhex(v["pk_sec1"]) == O.sec1_compress(O.pt_from_bytes(pk))
        for fmt, rec in (("affine64", pk), ("sec1", bytes.fromhex(v["pk_sec1"]))):
            a, st = K.eth_address_batch(np.frombuffer(rec, np.uint8), None, fmt, "eip55")
            assert a.tobytes().decode() == v["address"] and list(st) == [K.MATCH]
            a, st = K.eth_address_batch(np.frombuffer(rec, np.uint8), np.frombuffer(bytes.fromhex(v["address"][2:]), np.uint8), fmt, "record64")
            assert a.tobytes() == bytes(44) + bytes.fromhex(v["address"][2:]) and list(st) == [K.MATCH]


def test_eip55_examples():
    assert len(KATS["eip55"]) == 4
    for a in KATS["eip55"]:
        assert K.eip55(bytes.fromhex(a[2:])) == a


@pytest.mark.parametrize("fmt", ["affine64", "sec1"])
def test_what_is_no_ethereum_key(fmt):
    bad = K.invalid_keys(fmt)
    assert len(bad) >= 6
    for name, rec in bad:
        assert len(rec) == K.PK_WIDTH[fmt] and K.decode_pk(rec, fmt) is None, name
    a, st = K.eth_address_batch(np.frombuffer(b"".join(r for _, r in bad), np.uint8), np.zeros((len(bad), 20), np.uint8), fmt, "eip55")
    assert not a.any() and (st == K.INVALID).all()
    keys = K.sample_keys(6, 1, fmt)
    assert all(K.decode_pk(k.tobytes(), fmt) is not None for k in keys)
    if fmt == "sec1":
        assert {int(k[0]) for k in K.sample_keys(12, 2, fmt)} == {2, 3}
