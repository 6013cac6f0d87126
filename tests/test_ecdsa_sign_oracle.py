"""The restatement of plume_ecdsa_sign_batch and plume_eth_message_hash_batch (tests/_ecdsa_sign.py) against the committed vectors (tests/golden/ecdsa_sign_kats.json,
written and checked against the published RFC 6979 vectors and OpenSSL's verifier by tests/golden/make_ecdsa_sign_kats.py): the fixture is what the restatement says today,
every signature in it recovers to the signer's sk G through tests/_ecdsa.recover, and the rules of the header -- low s, the v rule, the status rules, the EIP-191
preimage -- hold on it.  CPU only."""
import hashlib

import pytest

from tests import _ecdsa as E
from tests import _ecdsa_sign as S
from tests import _keccak as K


@pytest.fixture(scope="module")
def kats():
    return S.load_kats()


def _aux(e):
    return None if e["aux"] is None else bytes.fromhex(e["aux"])


def test_the_published_vectors(kats):
    assert len(kats["public"]) == 3
    for p in kats["public"]:
        sk, h = bytes.fromhex(p["sk"]), hashlib.sha256(p["msg"].encode()).digest()
        assert h.hex() == p["hash"] and E.b32(S.nonce(sk, h)).hex() == p["k"]
        r, s, v, st = S.sign(sk, h)
        assert (E.b32(r).hex(), E.b32(s).hex(), v, st) == (p["r"], p["s"], p["v"], S.OK)
    assert kats["public"][0]["r"] == "934b1ea10a4b3c1757e2b0c017d0b6143ce3c9a7e6a4a49860d7a6ab210ee3d8" and kats["public"][0]["v"] == 1
    assert kats["public"][1]["s"].startswith("547fe644") and kats["public"][2]["r"].startswith("fd567d12")


def test_the_restatement_matches_the_fixture(kats):
    assert len(kats["sign"]) >= 36 + 2 * (len(S.SK_EDGES) + len(S.HASH_EDGES) + 16)
    for e in kats["sign"]:
        r, s, v, st = S.sign(bytes.fromhex(e["sk"]), bytes.fromhex(e["hash"]), _aux(e))
        assert S.sign(bytes.fromhex(e["sk"]), bytes.fromhex(e["hash"]), _aux(e), fast=True) == (r, s, v, st), e["name"]     # the batch form's window table
        assert (E.b32(r).hex(), E.b32(s).hex(), v, st) == (e["r"], e["s"], e["v"], e["status"]), e["name"]
        r27, s27, v27, st27 = S.sign(bytes.fromhex(e["sk"]), bytes.fromhex(e["hash"]), _aux(e), S.V27)
        assert (r27, s27, st27) == (r, s, st) and v27 == (v + 27 if st == S.OK else 0), e["name"]


def test_every_fixture_signature_recovers_to_the_signers_key(kats):
    for e in kats["sign"]:
        sk = int.from_bytes(bytes.fromhex(e["sk"]), "big")
        if e["status"] != S.OK:
            assert e["status"] == S.BAD_SCALAR and not 1 <= sk < E.N and (e["r"], e["s"], e["v"]) == ("00" * 32, "00" * 32, 0), e["name"]
            continue
        assert 1 <= sk < E.N, e["name"]
        r, s = int(e["r"], 16), int(e["s"], 16)
        assert 1 <= r < E.N and 1 <= s <= S.HALF_N, e["name"]                     # always low s
        for v in (e["v"], e["v"] + 27):
            assert E.recover(bytes.fromhex(e["hash"]), r, s, v, E.LOW_S) == E.mul(sk), e["name"]
        assert E.recover(bytes.fromhex(e["hash"]), r, s, e["v"] ^ 1) != E.mul(sk), e["name"]


def test_the_crafted_items_are_what_the_issue_asks_for(kats):
    plain = [e for e in kats["sign"] if e["aux"] is None]
    hedged = [e for e in kats["sign"] if e["aux"] is not None]
    for group in (plain, hedged):
        sks = {int(e["sk"], 16) for e in group}
        hashes = {int(e["hash"], 16) for e in group}
        assert set(S.SK_EDGES) <= sks and set(S.HASH_EDGES) <= hashes
        assert sum(1 for e in group if e["high"] is True) >= 8 and sum(1 for e in group if e["high"] is False) >= 8
    assert all(e["aux"] == S.FIXED_AUX.hex() for e in hedged)
    for e in kats["sign"]:
        if e["high"] is None:
            continue
        st, _, s, parity, _ = S.sign_raw(bytes.fromhex(e["sk"]), bytes.fromhex(e["hash"]), _aux(e))
        assert st == S.OK and (s > S.HALF_N) == e["high"], e["name"]
        assert int(e["s"], 16) == (E.N - s if e["high"] else s) and e["v"] == parity ^ (1 if e["high"] else 0), e["name"]   # the flip moves both
    # hedging changes the nonce, hence the signature, and not the status
    edges = len(S.SK_EDGES) + len(S.HASH_EDGES)
    for a, b in zip(plain[36:36 + edges], hedged[:edges]):
        assert a["name"] + ", hedged" == b["name"] and a["status"] == b["status"] and (a["status"] != S.OK or a["r"] != b["r"])


def test_the_hash_fixture_and_the_eip191_preimage(kats):
    assert K.keccak256(b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    assert K.keccak256(b"abc").hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"
    assert S.message_hash(b"hello world").hex() == "d9eba16ed0ecae432b71fe008c98cc872bb4cc214d3220a36f365326cf807d68"
    assert S.eip191_preimage(b"") == b"\x19Ethereum Signed Message:\n0" and len(S.EIP191_PREFIX) == 26
    assert S.eip191_preimage(b"x" * 1000)[:30] == b"\x19Ethereum Signed Message:\n1000"
    seen = {S.KECCAK256: [], S.EIP191: []}
    for e in kats["hash"]:
        msg = bytes.fromhex(e["msg"])
        assert S.message_hash(msg, e["mode"]).hex() == e["digest"]
        seen[e["mode"]].append(len(msg))
    assert set(S.HASH_LENGTHS[S.KECCAK256]) <= set(seen[S.KECCAK256]) and set(S.HASH_LENGTHS[S.EIP191]) <= set(seen[S.EIP191])
    # the lengths do sit on the rate's edges
    assert [26 + len(str(L)) + L for L in (106, 107, 108, 242, 243, 244)] == [135, 136, 137, 271, 272, 273]


def test_the_batch_forms_window_table_is_the_plain_multiplication():
    for k in (1, 2, 255, 256, 257, E.N - 1, E.N - 2, 2**255, 2**128 - 1, 0xFF << 248, 0x0123456789ABCDEF0123456789ABCDEF0123456789ABCDEF0123456789ABCDEF):
        for sk, z in ((1, 0), (E.N - 1, E.N - 1), (0x1234567, 2**200 + 5)):
            assert S.sign_given_nonce_fast(sk, z, k) == E.sign(sk, z, k), hex(k)
    sk, h, aux = S.seeded(24, 5)
    a = S.sign_batch(h, sk, aux, S.V27)
    for i in range(24):
        r, s, v, st = S.sign(sk[i].tobytes(), h[i].tobytes(), aux[i].tobytes(), S.V27)
        assert (a[0][i].tobytes(), a[1][i].tobytes(), a[2][i], a[3][i]) == (E.b32(r), E.b32(s), v, st)


def test_personal_sign_is_r_s_v27(kats):
    sk = bytes.fromhex(kats["sign"][0]["sk"])
    sig = S.personal_sign(sk, b"hello world")
    assert len(sig) == 65 and sig[64] in (27, 28)
    h = S.message_hash(b"hello world")
    assert E.recover(h, int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:64], "big"), sig[64], E.LOW_S) == E.mul(int.from_bytes(sk, "big"))
