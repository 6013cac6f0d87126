"""The ECDSA restatement the recovery tests compare with (tests/_ecdsa.py), held to vectors it did not make and to the recovery rule of include/plume_hip.h: OpenSSL's keys
and signatures (tests/golden/ecdsa_recover_kats.json), sign-then-recover on seeded keys, the (r, n - s, v ^ 1) twin, every invalid rule, the crafted constructions."""
import numpy as np
import pytest

from tests import _ecdsa as E
from tests import _keccak as K

KATS = E.load_kats()
hx = lambda e, k: int(e[k], 16)  # noqa: E731


def test_openssl_signatures_recover_openssl_keys():
    assert len(KATS["openssl"]) >= 24
    seen_v, high = set(), 0
    for e in KATS["openssl"]:
        want = (int(e["pk"][:64], 16), int(e["pk"][64:], 16))
        h = bytes.fromhex(e["hash"])
        assert E.recover(h, hx(e, "r"), hx(e, "s"), e["v"]) == want
        assert E.recover(h, hx(e, "r"), hx(e, "s"), e["v"] ^ 1) != want                     # the other parity is another key (27 ^ 1 = 26: none at all)
        seen_v.add(e["v"]); high += hx(e, "s") > E.HALF_N
    assert seen_v == {0, 1, 27, 28} and 0 < high < len(KATS["openssl"])


def test_generator_and_small_multiples():
    assert E.mul(1) == (E.GX, E.GY) and E.mul(E.N) is None and E.mul(E.N - 1) == (E.GX, E.P - E.GY)
    assert K.eip55(K.address_of(E.mul(1))) == "0x7E5F4552091A69125d5DfCb7b8C2659029395Bdf"    # the well-known address of the secret key 1
    assert E.mul(E.LAMBDA)[1] == E.GY and E.mul(E.LAMBDA)[0] != E.GX and pow(E.LAMBDA, 3, E.N) == 1


def test_sign_then_recover_and_the_low_s_twin():
    H, R, S, V, PK = E.genuine(24, 7)
    for i in range(24):
        h, r, s, v = H[i].tobytes(), int.from_bytes(R[i].tobytes(), "big"), int.from_bytes(S[i].tobytes(), "big"), int(V[i])
        assert E.recover(h, r, s, v) == PK[i]
        v %= 27                                                                          # the twin flips the PARITY: 27 <-> 28, not 27 <-> 26
        assert E.recover(h, r, s, v) == PK[i] == E.recover(h, r, E.N - s, v ^ 1)
        low, lv = (s, v) if s <= E.HALF_N else (E.N - s, v ^ 1)
        assert E.recover(h, r, low, lv, E.LOW_S) == PK[i] and E.recover(h, r, E.N - low, lv ^ 1, E.LOW_S) is None


def test_sign_then_recover_twin_for_27_28():
    H, R, S, V, PK = E.genuine(6, 8)
    for i in range(6):
        h, r, s, p = H[i].tobytes(), int.from_bytes(R[i].tobytes(), "big"), int.from_bytes(S[i].tobytes(), "big"), int(V[i]) % 27
        assert E.recover(h, r, s, 27 + p) == PK[i] == E.recover(h, r, E.N - s, 27 + (p ^ 1))


def test_every_invalid_rule():
    H, R, S, V, PK = E.genuine(1, 9)
    h, r, s, v = H[0].tobytes(), int.from_bytes(R[0].tobytes(), "big"), int.from_bytes(S[0].tobytes(), "big"), int(V[0])
    assert E.recover(h, r, s, v) == PK[0]
    for bad_v in (2, 3, 26, 29, 255):
        assert E.recover(h, r, s, bad_v) is None
    for bad in (0, E.N, E.N + 1, 2**256 - 1):
        assert E.recover(h, bad, s, v) is None and E.recover(h, r, bad, v) is None
    assert E.lift_x(E.N - 1, 0) is None and E.recover(h, E.N - 1, s, 0) is None            # in range, no square root
    for x in (1, 2, 3, 4, E.N - 2):
        assert E.lift_x(x, 0) is not None and E.recover(h, x, s, 0) is not None
    assert E.recover(h, r, E.HALF_N, v, E.LOW_S) is not None and E.recover(h, r, E.HALF_N + 1, v, E.LOW_S) is None
    assert E.recover(h, r, E.HALF_N + 1, v) is not None
    assert E.recover(E.b32(0), r, s, v) == E.recover(E.b32(E.N), r, s, v) != E.recover(E.b32(E.N + 1), r, s, v)


def test_crafted_constructions_do_what_they_are_named_for():
    cases = {name: (h, r, s, v, flags) for name, h, r, s, v, flags in E.crafted_cases()}
    assert [c["name"] for c in KATS["crafted"]] == list(cases)                               # the committed file is what the generator writes today
    for c in KATS["crafted"]:
        h, r, s, v, flags = cases[c["name"]]
        assert (bytes.fromhex(c["hash"]), hx(c, "r"), hx(c, "s"), c["v"], c["flags"]) == (h, r, s, v, flags)
    for name, (h, r, s, v, flags) in cases.items():
        q = E.recover(h, r, s, v, flags)
        if "identity" in name:
            assert q is None and E.lift_x(r, v & 1) is not None, name
        if name.startswith("comb doubling"):
            assert q == E.mul(2), name
        elif "doubling" in name:
            R = E.lift_x(r, v & 1)
            ri = pow(r, -1, E.N)
            u1, u2 = -int.from_bytes(h, "big") * ri % E.N, s * ri % E.N
            assert E.mul(u1) == E.mul(u2, R) and q == E.mul(2 * u1) and q is not None, name
    assert E.recover(*cases["u2 = lambda, hash = 0"][:4]) == E.mul(E.LAMBDA, E.lift_x(cases["u2 = lambda, hash = 0"][1], cases["u2 = lambda, hash = 0"][3]))


@pytest.mark.parametrize("pk_format,addr_format", [("affine64", "record64"), ("sec1", "eip55")])
def test_batch_records(pk_format, addr_format):
    H, R, S, V, PK = E.genuine(4, 10)
    V[2] = 9
    expect = np.stack([np.frombuffer(K.address_of(q), np.uint8) for q in PK]).copy()
    expect[1, 3] ^= 4
    pk, addr, st = E.recover_batch(H, R, S, V, expect, pk_format, addr_format)
    assert list(st) == [E.MATCH, E.MISMATCH, E.INVALID, E.MATCH]
    assert not pk[2].any() and not addr[2].any() and pk[1].any() and addr[1].any()
    assert pk[0].tobytes() == E.pk_record(PK[0], pk_format) and addr[3].tobytes() == K.record_of(K.address_of(PK[3]), addr_format)
    assert pk.shape == (4, K.PK_WIDTH[pk_format]) and addr.shape == (4, K.ADDR_WIDTH[addr_format])
