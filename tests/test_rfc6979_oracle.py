"""The RFC 6979 oracle (tests/_rfc6979.py) against published vectors: RFC 6979 Appendix A.2.5 (P-256, SHA-256) and the widely used secp256k1 vector
x = 1, "Satoshi Nakamoto".  These pins carry over to the lane body (tests/test_nonce_lanes.py), which is compared with the oracle."""
import hashlib

import pytest

from tests import _rfc6979 as R

P256_Q = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
P256_X = bytes.fromhex("C9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721")


@pytest.mark.parametrize("msg,k", [(b"sample", 0xA6E3C57DD01ABE90086538398355DD4C3B17AA873382B0F24D6129493D8AAD60),
                                   (b"test", 0xD16B6AE827F17175E040871A1C7EC3500192C4C92677336EC2537ACAEE0008E0)])
def test_rfc6979_a25_p256_sha256(msg, k):
    assert R.rfc6979_k(P256_Q, P256_X, hashlib.sha256(msg).digest()) == (k, 1)


def test_secp256k1_satoshi_vector():
    k, used = R.rfc6979_k(R.N, (1).to_bytes(32, "big"), hashlib.sha256(b"Satoshi Nakamoto").digest())
    assert k == 0x8F8A276C19F4149656B280621E358CCE24F5F52542772691EE69063B74F15D15 and used == 1


def test_plume_preimage_and_separation():
    pk = bytes(range(64))
    assert R.plume_h1(1, b"m") == hashlib.sha256(b"PLUME-RFC6979\x01\x00m").digest()
    assert R.plume_h1(2, b"m", pk) == hashlib.sha256(b"PLUME-RFC6979\x02\x01" + pk + b"m").digest()
    sk = (7).to_bytes(32, "big")
    got = {R.plume_nonce(v, sk, b"m", p, a) for v in (1, 2) for p in (None, pk) for a in (None, b"\x55" * 32)}
    assert len(got) == 8


def test_hedged_input_is_appended_in_steps_d_and_f():
    """§3.6: k' changes the nonce; the same k' gives the same nonce"""
    h1 = hashlib.sha256(b"sample").digest()
    a, b = R.rfc6979_k(P256_Q, P256_X, h1, b"\x01" * 32), R.rfc6979_k(P256_Q, P256_X, h1, b"\x02" * 32)
    assert a != b and a == R.rfc6979_k(P256_Q, P256_X, h1, b"\x01" * 32)


def test_retry_path_with_a_modulus_just_above_two_to_the_255():
    """q = 2^255 + 19: about half of all candidates are out of range, so step h's retry is exercised"""
    q = (1 << 255) + 19
    needs = [R.rounds_needed(q, i.to_bytes(32, "big"), hashlib.sha256(i.to_bytes(4, "big")).digest()) for i in range(1, 200)]
    assert {1, 2, 3} <= set(needs)
    assert 0.3 < needs.count(1) / len(needs) < 0.7
