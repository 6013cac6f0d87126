#!/usr/bin/env python3
"""Writes tests/golden/eth_tx_sign_kats.json: the unsigned transactions the transaction-signing tests pin beyond what tests/golden/eth_tx_kats.json gives
(python tests/golden/make_eth_tx_sign_kats.py).  Everything is made by the restatement in tests/_eth_tx_sign.py from fixed keys, so the file is reproducible; while writing
it this script ASSERTS that every signed item parses (tests/_eth_tx.parse) to the hash of its unsigned form, to the chain id and type it was built with, and recovers to
its signer's key.
"items": SIGNED-list payloads of exactly 255, 256, 65535 and 65536 bytes (the data length tuned after signing: the signature's own length moves with the data); EIP-155
chain ids 46, 47 (v = 127, 128 with parity 0: the one-byte / two-byte edge of rlp_int(v)), 127, 128, 2^32, 2^63 - 18, each with both parities (the last with parity 1 has
v = 2^64: PLUME_STATUS_IDENTITY); one invalid unsigned item for each rule of the
header; a key of 0 and a key equal to n.  One row per item -- name, unsigned, sk, status, raw --, the two long items' repeated data counted instead of written out
(tests/_eth_tx_sign.load_kats undoes it)."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
from tests import _ecdsa as E  # noqa: E402
from tests import _ecdsa_sign as S  # noqa: E402
from tests import _eth_tx as T  # noqa: E402
from tests import _eth_tx_sign as X  # noqa: E402
from tests import _keccak as K  # noqa: E402

UNIT = 17


def key(j):
    return E.b32(int.from_bytes(K.keccak256(b"eth tx sign kats key %d" % j), "big") % (E.N - 1) + 1)


def data_of(length, salt):
    unit = bytes((31 * j + 5 * salt + 3) & 0xFF for j in range(UNIT))
    return (unit * (length // UNIT + 1))[:length]


def packed_hex(raw):
    raw = bytes(raw)
    if len(raw) <= 1000:
        return raw.hex()
    best = (0, 0)
    for a in range(64):
        n = 0
        while a + UNIT * (n + 2) <= len(raw) and raw[a + UNIT * (n + 1):a + UNIT * (n + 2)] == raw[a:a + UNIT]:
            n += 1
        best = max(best, (n + 1, -a))
    count, a = best[0], -best[1]
    assert count > 50 and raw[:a] + raw[a:a + UNIT] * count + raw[a + UNIT * count:] == raw
    return [raw[:a].hex(), [raw[a:a + UNIT].hex(), count], raw[a + UNIT * count:].hex()]


items = []


def add(name, unsigned, sk, expect_status, typ=None, chain=None):
    raw, h, r, s, parity, st = X.sign_tx(unsigned, sk)
    assert st == expect_status, (name, st)
    if st == X.OK:
        p = T.parse(raw)
        assert p is not None and p[0] == h == K.keccak256(unsigned) and (p[1], p[2], p[3]) == (r, s, parity), name
        assert (p[4], p[5]) == (chain, typ), name
        assert s <= E.HALF_N and E.recover(h, r, s, parity, 0) == E.mul(int.from_bytes(sk, "big")), name
        assert X.unsigned_of(raw) == unsigned and len(raw) <= len(unsigned) + X.GROWTH, name
    else:
        assert raw == b""
    items.append({"name": name, "unsigned": packed_hex(unsigned), "sk": sk.hex(), "status": st, "raw": packed_hex(raw)})
    return raw


def signed_payload(raw):
    lst = 0 if raw[0] >= 0xC0 else 1
    _, a, b = T.read_header(raw, lst, len(raw))
    return b - a


# ------------------------------------------------------------------------------------------------ signed-list payloads on the header's thresholds
j = 0
for typ, chain, L in ((2, 1, 255), (0, 1, 256), (0, 0, 65535), (2, 5, 65536)):
    j += 1
    d, seen = max(0, L - 200), set()
    while True:                                                             # the signature's length depends on the data: walk until the signed payload is L
        unsigned = T.signing_data(typ, T.default_fields(typ, chain, data_of(d, j), j), chain)
        got = signed_payload(X.sign_tx(unsigned, key(j))[0])
        if got == L:
            break
        assert d not in seen, (typ, L)                                      # (a cycle: another key would be needed)
        seen.add(d)
        d += L - got
    add(f"{'legacy' if typ == 0 else 'type 0%d' % typ} chain {chain}, signed payload {L}", unsigned, key(j), X.OK, typ, chain)

# ------------------------------------------------------------------------------------------------ EIP-155 chain ids
for chain in (46, 47, 127, 128, 2**32, 2**63 - 18):
    for par in (0, 1):                                                      # both parities of each: v = 35 + 2 chain + parity sits on both sides of an edge
        jj = j
        while True:
            jj += 1
            unsigned = T.signing_data(0, T.default_fields(0, chain, data_of(jj % 5, jj), jj), chain)
            over = par == 1 and chain == 2**63 - 18                           # v = 2^64: no representation, PLUME_STATUS_IDENTITY
            if S.sign(key(jj), K.keccak256(unsigned), fast=True)[2] == par:
                break
        j = jj
        add(f"legacy EIP-155, chain id {chain}, parity {par}", unsigned, key(j), X.IDENTITY if over else X.OK, 0, chain)

# ------------------------------------------------------------------------------------------------ invalid unsigned items
f0 = T.default_fields(0, 0, b"\x01\x02", 3)
sk = key(900)


def legacy_with(extra):
    return T.list_of(b"".join(T.rlp(x) for x in f0) + extra)


signed_legacy = X.sign_tx(T.signing_data(0, f0, 1), sk)[0]
signed_typed = X.sign_tx(T.signing_data(2, T.default_fields(2, 1, b"", 3)), sk)[0]
bad = [
    ("a signed legacy transaction as input", signed_legacy),
    ("a signed type 02 transaction as input", signed_typed),
    ("legacy, 5 items", T.rlp(f0[:5])),
    ("legacy, 7 items", legacy_with(T.rlp(1))),
    ("legacy, 8 items", legacy_with(T.rlp(1) + b"\x80")),
    ("legacy, 10 items", legacy_with(T.rlp(1) + b"\x80\x80\x80")),
    ("legacy, nine items ending 80 01", legacy_with(T.rlp(1) + b"\x80\x01")),
    ("legacy, nine items ending 01 80", legacy_with(T.rlp(1) + b"\x01\x80")),
    ("legacy, nine items, an empty list for the ninth", legacy_with(T.rlp(1) + b"\x80\xc0")),
    ("legacy, chainId 0", legacy_with(b"\x80\x80\x80")),
    ("legacy, chainId 2^63 - 17", legacy_with(T.rlp(2**63 - 17) + b"\x80\x80")),
    ("legacy, chainId of 9 bytes", legacy_with(T.rlp(2**64) + b"\x80\x80")),
    ("legacy, chainId with a leading zero", legacy_with(b"\x82\x00\x01\x80\x80")),
    ("legacy, chainId a list", legacy_with(b"\xc1\x01\x80\x80")),
    ("the empty item", b""),
    ("type byte 00", b"\x00" + T.rlp(T.default_fields(2, 1, b"", 3))),
    ("type byte 05", b"\x05" + T.rlp(T.default_fields(2, 1, b"", 3))),
    ("type byte 7f", b"\x7f" + T.rlp(T.default_fields(2, 1, b"", 3))),
    ("a string, not a list", T.rlp(b"\x01" * 40)),
    ("type 02, the type byte alone", b"\x02"),
    ("type 02, a chainId of 9 bytes", b"\x02" + T.rlp([2**64] + T.default_fields(2, 1, b"", 3)[1:])),
    ("type 02, chainId with a leading zero", b"\x02" + T.list_of(b"\x82\x00\x01" + b"".join(T.rlp(x) for x in T.default_fields(2, 1, b"", 3)[1:]))),
]
for typ in (1, 2, 3, 4):
    f = T.default_fields(typ, 1, b"", 3)
    bad.append((f"type 0{typ}, one field too few", bytes([typ]) + T.rlp(f[:-1])))
    bad.append((f"type 0{typ}, one field too many", bytes([typ]) + T.rlp(f + [0])))
good6 = T.rlp(f0)
long6 = T.rlp(T.default_fields(0, 0, data_of(100, 1), 1))                   # a long-form header: f8 LL
assert good6[0] < 0xF8 and long6[0] == 0xF8
bad += [
    ("legacy, outer header in the long form for a short payload", bytes([0xF8, good6[0] - 0xC0]) + good6[1:]),
    ("legacy, outer length with a leading zero", bytes([0xF9, 0x00, long6[1]]) + long6[2:]),
    ("legacy, payload one byte longer than the item", bytes([good6[0] + 1]) + good6[1:]),
    ("legacy, payload one byte shorter than the item", bytes([good6[0] - 1]) + good6[1:]),
    ("legacy, a trailing byte behind the list", good6 + b"\x00"),
    ("legacy, a one-byte string below 0x80 in the long form", T.list_of(b"\x81\x05" + good6[2:])),
    ("legacy, the last field overruns the list", T.list_of(good6[1:-3] + b"\x85\x01\x02")),
]
for name, unsigned in bad:
    assert X.frame_unsigned(unsigned) is None, name
    add(name, unsigned, sk, X.BAD_TX)

# ------------------------------------------------------------------------------------------------ keys out of range
for name, k in (("a key of 0", 0), ("a key equal to n", E.N), ("a key of 2^256 - 1", 2**256 - 1)):
    add(f"type 02, {name}", T.signing_data(2, T.default_fields(2, 1, b"", 3)), E.b32(k), X.BAD_SCALAR)
add("an ill-framed item with a key of 0: BAD_TX alone", b"\x05\xc0", E.b32(0), X.BAD_TX)

out = ROOT / "tests" / "golden" / "eth_tx_sign_kats.json"
text = "{\n\"items\": [\n" + ",\n".join(json.dumps(e, separators=(",", ":")) for e in items) + "\n]\n}\n"
out.write_text(text)
print(f"{len(items)} items, {len(text)} bytes -> {out}")
