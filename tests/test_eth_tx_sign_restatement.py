"""The restatement of plume_eth_tx_sign_batch (tests/_eth_tx_sign.py) against what it did not produce: EIP-155's published example, and the 108 signed low-s items of
tests/golden/eth_tx_kats.json, which tests/_eth_tx.build made field by field -- here each is taken apart into its unsigned serialization and signed again.  Then the
committed vectors of tests/golden/eth_tx_sign_kats.json and the slot layout.  CPU only."""
import numpy as np
import pytest

from tests import _ecdsa as E
from tests import _eth_tx as T
from tests import _eth_tx_sign as X
from tests import _keccak as K


@pytest.fixture(scope="module")
def kats():
    return T.load_kats()


@pytest.fixture(scope="module")
def signed_items(kats):
    """(name, raw, sk, unsigned, re-signed) of every fixture item that has a key and a low s"""
    out = []
    for e in kats["items"]:
        if e["sk"] is None or e["high_s"] or e["status"] != T.OK:
            continue
        raw, sk = bytes.fromhex(e["raw"]), bytes.fromhex(e["sk"])
        u = X.unsigned_of(raw)
        out.append((e["name"], raw, sk, u, X.sign_tx(u, sk), e))
    return out


def test_eip155_published_example(kats):
    ex = kats["eip155"]
    raw, h, r, s, parity, st = X.sign_tx(bytes.fromhex(ex["signing_data"]), bytes.fromhex(ex["sk"]))
    assert st == X.OK and raw.hex() == ex["raw"] and h.hex() == ex["hash"]
    assert (E.b32(r).hex(), E.b32(s).hex(), 35 + 2 + parity) == (ex["r"], ex["s"], ex["v"])
    assert X.unsigned_of(raw) == bytes.fromhex(ex["signing_data"])


def _payload(item):
    lst = 0 if item[0] >= 0xC0 else 1
    _, a, b = T.read_header(item, lst, len(item))
    return b - a


def test_every_signed_fixture_item_is_reproduced(signed_items):
    assert len(signed_items) == 108
    short_r = short_s = 0
    kinds, sides = set(), set()
    for name, raw, sk, u, (got, h, r, s, parity, st), e in signed_items:
        assert st == X.OK and got == raw, name
        assert h.hex() == e["hash"] == K.keccak256(u).hex(), name                       # the signing hash is Keccak-256 of the whole unsigned item
        assert len(got) <= len(u) + X.GROWTH, name                                      # the growth bound of the slot rule
        fr = X.frame_unsigned(u)
        assert (fr[0], fr[1]) == (e["tx_type"], int(e["chain_id"])), name
        short_r += r < 2**248
        short_s += s < 2**248
        kinds.add((fr[0], fr[2]))
        p = _payload(u)
        sides |= {(t, p > t) for t in (55, 255, 65535) if p in (t, t + 1)}
    assert short_r >= 1 and short_s >= 1, (short_r, short_s)
    assert (short_r, short_s) == (1, 2)                                                 # counted once, when the fixture was read for this test
    assert kinds == {(0, False), (0, True), (1, False), (2, False), (3, False), (4, False)}
    for t in (55, 255, 65535):                                                          # signing-list payloads on both sides of every header threshold
        assert (t, False) in sides and (t, True) in sides, (t, sorted(sides))


def test_growth_is_reached_but_never_exceeded(signed_items):
    grow = [len(got) - len(u) for _, _, _, u, (got, *_), _ in signed_items]
    assert max(grow) <= X.GROWTH
    # a typed item whose signed payload crosses a header threshold gains 1 + 33 + 33 payload bytes and one header byte
    crossing = [g for (_, _, _, u, (got, *_), _), g in zip(signed_items, grow) if u[0] < 0xC0 and len(T._header(_payload(got), 0xC0)) > len(T._header(_payload(u), 0xC0))]
    assert crossing and max(crossing) <= 68 and min(crossing) >= 66
    eip155 = [g for (_, _, _, u, _, _), g in zip(signed_items, grow) if X.frame_unsigned(u)[2]]
    assert eip155 and max(eip155) <= 33 + 33 + 1                                        # chainId 80 80 -> v is never a net gain: r, s and at most one header byte


def test_committed_vectors():
    kats = X.load_kats()
    names = [e["name"] for e in kats["items"]]
    assert len(set(names)) == len(names) == 57
    got_payloads, chains, statuses = set(), set(), {}
    for e in kats["items"]:
        u, sk = bytes.fromhex(e["unsigned"]), bytes.fromhex(e["sk"])
        raw, h, r, s, parity, st = X.sign_tx(u, sk)
        assert st == e["status"] and raw.hex() == e["raw"], e["name"]
        statuses[st] = statuses.get(st, 0) + 1
        if st != X.OK:
            assert raw == b"" and (h, r, s, parity) == (bytes(32), 0, 0, 0)
            continue
        assert len(raw) <= len(u) + X.GROWTH
        p = T.parse(raw)
        assert p is not None and p[0] == h and E.recover(h, r, s, parity, 0) == E.mul(int.from_bytes(sk, "big")), e["name"]
        got_payloads.add(_payload(raw))
        fr = X.frame_unsigned(u)
        if fr[2]:
            chains.add((fr[1], parity))
    assert {255, 256, 65535, 65536} <= got_payloads
    assert {(c, q) for c in (46, 47, 127, 128, 2**32) for q in (0, 1)} | {(2**63 - 18, 0)} <= chains
    assert statuses[X.BAD_TX] >= 30 and statuses[X.BAD_SCALAR] == 3 and statuses[X.IDENTITY] == 1


def test_bad_tx_is_reported_alone():
    assert X.sign_tx(b"\x05\xc0", bytes(32))[5] == X.BAD_TX                              # whatever the key is
    good = T.signing_data(2, T.default_fields(2, 1, b"", 3))
    assert X.sign_tx(good, bytes(32))[5] == X.BAD_SCALAR
    assert X.sign_tx(good, E.b32(E.N))[5] == X.BAD_SCALAR


def test_aux_hedges_the_nonce_and_nothing_else():
    u, sk = T.signing_data(0, T.default_fields(0, 5, b"abc", 1), 5), E.b32(7)
    a, b = X.sign_tx(u, sk), X.sign_tx(u, sk, bytes(range(32)))
    assert a[0] != b[0] and a[1] == b[1] and b[5] == X.OK
    p = T.parse(b[0])
    assert E.recover(p[0], p[1], p[2], p[3], 0) == E.mul(7) and p[4] == 5


def test_slot_layout_of_a_batch():
    items = [T.signing_data(0, T.default_fields(0, 0, b"", 1)), b"\x05", T.signing_data(2, T.default_fields(2, 1, b"x" * 60, 2)), b""]
    txs, off = T.pack(items)
    off = off + np.uint64(0)
    sk = b"".join(E.b32(k) for k in (3, 4, 5, 6))
    o = X.sign_batch(txs, off, sk)
    assert len(o["out"]) == len(txs) + X.GROWTH * 4
    assert list(o["status"]) == [0, X.BAD_TX, 0, X.BAD_TX]
    raws = X.compact(o["out"], o["out_len"], off)
    assert raws[0] == X.sign_tx(items[0], E.b32(3))[0] and raws[2] == X.sign_tx(items[2], E.b32(5))[0] and raws[1] == raws[3] == b""
    for (start, length), ln in zip(X.slot_bounds(off), o["out_len"]):
        assert not o["out"][start + int(ln):start + length].any()
    # the device form's limits: an out_bytes that cuts the third slot
    cut = X.slot_bounds(off)[2][0] + 10
    o2 = X.sign_batch(txs, off, sk, out_bytes=cut)
    assert list(o2["status"]) == [0, X.BAD_TX, X.BAD_TX, X.BAD_TX] and o2["out_len"][2] == 0
    assert bytes(o2["out"][:cut]) == bytes(o["out"][:X.slot_bounds(off)[2][0]]) + bytes(10)
