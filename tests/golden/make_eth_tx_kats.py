#!/usr/bin/env python3
"""Writes tests/golden/eth_tx_kats.json: the raw transactions the transaction tests pin (python tests/golden/make_eth_tx_kats.py).  Everything is made by the restatement
in tests/_eth_tx.py from fixed keys, so the file is reproducible; while writing it this script ASSERTS EIP-155's worked example (signing data, hash, v, r, s, the raw
transaction, its id and its sender), re-derived here from the fields and the key, and that every signed item recovers to its signer's key.
"items": every kind (legacy unprotected, EIP-155, types 01-04); signing-list payloads either side of 55 / 56, 255 / 256 and 65535 / 65536; streams of 134, 135, 0 and 1
bytes mod 136; the body / suffix boundary on both sides of and across a block boundary; every reachable prefix length (1 .. 6 bytes: the prefix starts the stream, and a
list header of more than five bytes needs an item of 2^32 bytes); the chain ids on the edges of each encoding width; r / s of every length from 1 to 32 bytes; r = 0; a high
s; and one framing-invalid item for each rule of the header.  The file is kept small: one row of tests/_eth_tx.COLUMNS per item, the two long items' repeated data counted
instead of written out, nothing but name, raw and status for an invalid item (tests/_eth_tx.load_kats undoes all three)."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
from tests import _ecdsa as E  # noqa: E402
from tests import _eth_tx as T  # noqa: E402
from tests import _keccak as K  # noqa: E402


class Raw(bytes):
    """an item that is already encoded"""


def enc(x):
    return bytes(x) if isinstance(x, Raw) else T.rlp(x)


def wrap(typ, items, header=None):
    body = b"".join(enc(x) for x in items)
    return (b"" if typ == 0 else bytes([typ])) + (T._header(len(body), 0xC0) if header is None else header) + body


def key(j):
    return E.b32(int.from_bytes(K.keccak256(b"eth tx kats key %d" % j), "big") % (E.N - 1) + 1)


UNIT = 17                                                                   # a long data field repeats 17 bytes: odd against the 8-byte lanes and the 136-byte rate


def data_of(length, salt):
    if length > 1000:
        unit = bytes((29 * j + 7 * salt + 1) & 0xFF for j in range(UNIT))
        return (unit * (length // UNIT + 1))[:length]
    return bytes((29 * j + 7 * salt + (j >> 8)) & 0xFF for j in range(length))


def packed_hex(raw):
    """the hex of raw; a long item as [hex, [unit hex, count], hex], the run of its repeated unit counted instead of written out (tests/_eth_tx.load_kats undoes it)"""
    raw = bytes(raw)
    if len(raw) <= 1000:
        return raw.hex()
    best = (0, 0)
    for a in range(64):                                                     # the data field begins within the first few fields
        n = 0
        while a + UNIT * (n + 2) <= len(raw) and raw[a + UNIT * (n + 1):a + UNIT * (n + 2)] == raw[a:a + UNIT]:
            n += 1
        best = max(best, (n + 1, -a))
    count, a = best[0], -best[1]
    assert count > 50 and raw[:a] + raw[a:a + UNIT] * count + raw[a + UNIT * count:] == raw
    return [raw[:a].hex(), [raw[a:a + UNIT].hex(), count], raw[a + UNIT * count:].hex()]


items = []


def add(name, raw, sk=None, high_s=False):
    p = T.parse(raw)
    e = {"name": name, "raw": packed_hex(raw), "sk": None if sk is None else sk.hex(), "high_s": high_s}
    if p is None:
        e["status"] = T.INVALID                                             # every record of an invalid item is zero: load_kats fills them in
    else:
        e.update(status=T.OK, hash=p[0].hex(), r=E.b32(p[1]).hex(), s=E.b32(p[2]).hex(), v=p[3], chain_id=str(p[4]), tx_type=p[5])
        if sk is not None:
            assert E.recover(p[0], p[1], p[2], p[3], 0) == E.mul(int.from_bytes(sk, "big")), name
            assert (p[2] > E.HALF_N) == high_s, name
    items.append(e)
    return p


def signed(name, typ, j, chain_id=0, data=b"", fields=None, high_s=False):
    sk = key(j)
    raw, h, r, s, parity = T.build(typ, sk, chain_id, data, salt=j, fields=fields, high_s=high_s)
    t = 0
    while typ == 0 and 35 + 2 * chain_id + parity >= 2**64:                 # the largest chain id has a v of 8 bytes with parity 0 alone: another key
        t += 1
        sk = key(j + 5000 * t)
        raw, h, r, s, parity = T.build(typ, sk, chain_id, data, salt=j, fields=fields, high_s=high_s)
    p = add(name, raw, sk, high_s)
    assert p == (h, r, s, parity, chain_id, typ), name
    return raw


def data_for(typ, j, chain_id, want, what, monotone=False):
    """the data length at which `what(signing data)` is `want`"""
    val = lambda d: what(T.signing_data(typ, T.default_fields(typ, chain_id, data_of(d, j), j), chain_id))  # noqa: E731
    if monotone:
        lo, hi = 0, 70000
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if val(mid) >= want else (mid + 1, hi)
        assert val(lo) == want, (typ, want)
        return data_of(lo, j)
    for d in range(600):
        if val(d) == want:
            return data_of(d, j)
    raise AssertionError((typ, want))


def payload_len(sd):
    """the payload length of the signing data's list header"""
    lst = 0 if sd[0] >= 0xC0 else 1
    _, a, b = T.read_header(sd, lst, len(sd))
    return b - a


# ------------------------------------------------------------------------------------------------ EIP-155's worked example
sk155 = bytes([0x46]) * 32
f155 = [9, 20 * 10**9, 21000, bytes([0x35]) * 20, 10**18, b""]
sd = T.signing_data(0, f155, 1)
assert sd.hex() == "ec098504a817c800825208943535353535353535353535353535353535353535880de0b6b3a764000080018080"
raw155, h155, r155, s155, par155 = T.build(0, sk155, 1, fields=f155)
assert h155.hex() == "daf5a779ae972f972197303d7b574746c7ef83eadac0f2791ad23db92e4c8e53"
assert par155 + 35 + 2 == 37
assert E.b32(r155).hex() == "28ef61340bd939bc2195fe537567866003e1a15d3c71ff63e1590620aa636276"
assert E.b32(s155).hex() == "67cbe9d8997f761aecb703304b3800ccf555c9f3dc64214b297fb1966a3b6d83"
assert len(raw155) == 110 and raw155.hex().startswith("f86c0985") and raw155.hex().endswith("6d83") and "25a028ef" in raw155.hex()
assert K.keccak256(raw155).hex() == "33469b22e9f636356c4160a87eb19df52b7412e8eac32a4a55ffe88ea8350788"
addr155 = T.sender_of(sk155)[1]
assert K.eip55(addr155) in ("0x9d8A62f656a8d1615C1294fd71e9CFb3E4855A4F", b"0x9d8A62f656a8d1615C1294fd71e9CFb3E4855A4F")
eip155 = {"sk": sk155.hex(), "signing_data": sd.hex(), "hash": h155.hex(), "v": 37, "r": E.b32(r155).hex(), "s": E.b32(s155).hex(), "raw": raw155.hex(),
          "id": K.keccak256(raw155).hex(), "sender": "0x9d8A62f656a8d1615C1294fd71e9CFb3E4855A4F"}
add("EIP-155 worked example", raw155, sk155)

# ------------------------------------------------------------------------------------------------ valid items
KINDS = [("legacy unprotected", 0, 0), ("legacy EIP-155", 0, 1), ("type 01", 1, 1), ("type 02", 2, 1), ("type 03", 3, 1), ("type 04", 4, 1)]
j = 0
for name, typ, chain in KINDS:
    for d in (0, 1, 36, 100):
        j += 1
        signed(f"{name}, data {d}", typ, j, chain, data_of(d, j))
for name, typ, chain in KINDS:                                              # the list header's forms (and with them the prefix lengths 1 .. 6)
    for L in (55, 56, 255, 256, 65535, 65536):
        if L >= 65535 and (typ, chain) != (0, 0):                           # (two long items are enough: the file stays small)
            continue
        j += 1
        try:
            d = data_for(typ, j, chain, L, payload_len, monotone=True)
        except AssertionError:
            if payload_len(T.signing_data(typ, T.default_fields(typ, chain, b"", j), chain)) > L:       # (this item's shortest body is longer)
                continue
            j += 128                                                        # the data's own header grew past L: a nonce of one byte more
            d = data_for(typ, j, chain, L, payload_len, monotone=True)
        signed(f"{name}, signing payload {L}", typ, j, chain, d)
for name, typ, chain in KINDS:                                              # the stream's length on the rate's edges
    for m in (134, 135, 0, 1):
        for blocks in ((1, 2) if (typ, chain) in ((0, 1), (2, 1)) else (1,)):
            j += 1
            d = data_for(typ, j, chain, m, lambda sd: len(sd) % 136 if len(sd) > 136 * (blocks - 1) + 100 else -1)
            signed(f"{name}, stream {m} mod 136, {blocks} block(s) of body", typ, j, chain, d)
BIG = 2**63 - 18
for k in range(0, 13):                                                      # the 11-byte suffix of the largest chain id starts k bytes in front of a block boundary
    j += 1
    d = data_for(0, j, BIG, (136 - k + 11) % 136, lambda sd: len(sd) % 136 if len(sd) > 150 else -1)
    signed(f"EIP-155, suffix {k} bytes in front of a block boundary", 0, j, BIG, d)
for chain in (1, 127, 128, 255, 256, 2**32, BIG):
    j += 1
    signed(f"legacy EIP-155, chain id {chain}", 0, j, chain, data_of(j % 5, j))
for typ in (1, 2, 3, 4):
    for chain in ((0, 127, 128, 2**64 - 1) if typ == 2 else (2**64 - 1,)):
        j += 1
        signed(f"type 0{typ}, chain id {chain}", typ, j, chain, data_of(j % 7, j))
short = {"r": None, "s": None}                                              # r / s of 31 bytes: by search
jj = 1000
while None in short.values():
    jj += 1
    raw, h, r, s, parity = T.build(2, key(jj), 1, salt=jj)
    for which, val in (("r", r), ("s", s)):
        if short[which] is None and val < 2**248:
            short[which] = jj
            add(f"type 02, {which} of 31 bytes", raw, key(jj))
j += 1
signed("legacy EIP-155, high s", 0, j, 1, high_s=True)
j += 1
signed("type 02, high s", 2, j, 1, high_s=True)
for typ, chain in ((0, 0), (0, 5), (2, 5)):                                 # nobody signed these: the framing alone
    f = T.default_fields(typ, chain, b"", 3)
    v0 = 0 if typ else (35 + 2 * chain if chain else 27)
    add(f"type {typ} chain {chain}, r and s of 1 byte", T.assemble(typ, f, v0 + 1, 1, 0x7F))
    add(f"type {typ} chain {chain}, r of 1 byte above 0x7f", T.assemble(typ, f, v0, 0x80, 0xFF))
    add(f"type {typ} chain {chain}, r = 0: framing-valid, recover-invalid", T.assemble(typ, f, v0, 0, 5))
    add(f"type {typ} chain {chain}, s = 0", T.assemble(typ, f, v0, 5, 0))
    add(f"type {typ} chain {chain}, r = s = 2^256 - 1", T.assemble(typ, f, v0, 2**256 - 1, 2**256 - 1))
for L in range(1, 33):                                                      # every length of r and s: the left padding (nobody signed these either)
    rv, sv = int.from_bytes(bytes(range(0x81, 0x81 + L)), "big"), int.from_bytes(bytes(range(0x91, 0x91 + 33 - L)), "big")
    add(f"shortest legacy, r of {L} bytes, s of {33 - L}", T.assemble(0, [0, 1, 1, b"", 0, b""], 27 + L % 2, rv, sv))
    if L % 2:
        add(f"shortest type 02, r of {L} bytes, s of {33 - L}", T.assemble(2, [1, 0, 1, 1, 1, b"", 0, b"", []], L // 2 % 2, rv, sv))
nvalid = len(items)
assert all(e["status"] == T.OK for e in items)

# ------------------------------------------------------------------------------------------------ one invalid item for each rule
base = {name: (typ, chain, T.default_fields(typ, chain, data_of(5, typ), 2 * typ)) for name, typ, chain in KINDS}
sig = [1, 0x1234, 0x5678]                                                   # yParity, r, s for a typed item
add("the empty item", b"")
good2 = wrap(2, base["type 02"][2] + sig)
assert T.parse(good2) is not None and T.parse(wrap(0, base["legacy unprotected"][2] + [27, 1, 1])) is not None
for b in (0x00, 0x05, 0x7F, 0x80, 0xBF):
    add(f"first byte {b:02x} alone", bytes([b]))
    add(f"first byte {b:02x} in front of a type 02 list", bytes([b]) + good2[1:])
for name, typ, chain in KINDS:
    f = base[name][2]
    tail = [27 if not chain else 37, 0x1234, 0x5678] if typ == 0 else sig
    ok = wrap(typ, f + tail)
    assert T.parse(ok) is not None, name
    if typ in (0, 2):
        add(f"{name}, the list one byte short", ok[:-1])
        add(f"{name}, the list one byte long", ok + b"\x00")
    add(f"{name}, one item fewer", wrap(typ, f[:-1] + tail))
    add(f"{name}, one item more", wrap(typ, f + [b""] + tail))
    add(f"{name}, one item more behind s", wrap(typ, f + tail + [b""]))
tiny = [0, 1, 1, b"", 0, b"", 27, 1, 1]
assert T.parse(wrap(0, tiny)) is not None
add("outer header f8 with a length of 9", wrap(0, tiny, header=bytes([0xF8, 9])))
add("typed, outer header f8 with a length below 56", wrap(1, [1, 0, 1, 1, b"", 0, b"", [], 1, 1, 1], header=bytes([0xF8, 13])))
lf = base["legacy EIP-155"][2] + [37, 2**255, 2**254]
plen = len(b"".join(enc(x) for x in lf))
assert 56 <= plen < 256
add("outer header with a leading zero length byte", wrap(0, lf, header=bytes([0xF9, 0, plen])))
add("typed, outer header with a leading zero length byte", wrap(2, base["type 02"][2] + [1, 2**255, 2**254], header=bytes([0xF9, 0, len(wrap(2, base["type 02"][2] + [1, 2**255, 2**254])) - 3])))
add("outer header with eight length bytes", wrap(0, lf, header=bytes([0xFF]) + plen.to_bytes(8, "big")))
add("outer header with five length bytes, the first not zero", wrap(0, lf, header=bytes([0xFC, 1, 0, 0, 0, plen])))
add("outer header cut off behind its first byte", bytes([0xF9]))
add("the outer item is a string", b"\xb8" + bytes([plen]) + b"".join(enc(x) for x in lf))
add("s overruns the payload", wrap(0, base["legacy EIP-155"][2] + [37, 2**255, Raw(b"\xa1" + E.b32(2**254))]))
add("data overruns the payload", wrap(0, base["legacy EIP-155"][2][:5] + [Raw(b"\xb9\xff\xff" + bytes(40)), 37, 1, 1]))
add("the last item's header is cut off", wrap(0, base["legacy EIP-155"][2] + [37, 2**255, Raw(b"\xb8")]))
add("nonce as 81 05", wrap(0, [Raw(b"\x81\x05")] + base["legacy EIP-155"][2][1:] + [37, 1, 1]))
add("data in the long form for 5 bytes", wrap(0, base["legacy EIP-155"][2][:5] + [Raw(b"\xb8\x05" + bytes(5)), 37, 1, 1]))
add("the access list in the long form for an empty list", wrap(2, base["type 02"][2][:-1] + [Raw(b"\xf8\x00")] + sig))
add("to with a leading zero length byte", wrap(0, base["legacy EIP-155"][2][:3] + [Raw(b"\xb9\x00\x38" + bytes(56))] + base["legacy EIP-155"][2][4:] + [37, 1, 1]))
add("v as a list", wrap(0, base["legacy unprotected"][2] + [[], 1, 1]))
add("v as a list of one", wrap(0, base["legacy unprotected"][2] + [[27], 1, 1]))
for v in (0, 1, 26, 29, 34, 35, 36):
    add(f"v = {v}", wrap(0, base["legacy unprotected"][2] + [v, 1, 1]))
add("v of 9 bytes", wrap(0, base["legacy unprotected"][2] + [2**64, 1, 1]))
add("v with a leading zero", wrap(0, base["legacy unprotected"][2] + [b"\x00\x1b", 1, 1]))
assert T.parse(wrap(0, base["legacy unprotected"][2] + [2**64 - 1, 1, 1]))[4] == BIG
for name, typ, chain in KINDS[2:]:
    f = base[name][2]
    add(f"{name}, yParity 2", wrap(typ, f + [2, 1, 1]))
    if typ != 2:                                                            # (the other forms once: the rule does not depend on the type)
        continue
    add(f"{name}, yParity 00", wrap(typ, f + [b"\x00", 1, 1]))
    add(f"{name}, yParity 81 01", wrap(typ, f + [Raw(b"\x81\x01"), 1, 1]))
    add(f"{name}, yParity 27", wrap(typ, f + [27, 1, 1]))
    add(f"{name}, yParity 256", wrap(typ, f + [256, 1, 1]))
    add(f"{name}, yParity as a list", wrap(typ, f + [[], 1, 1]))
    add(f"{name}, chainId of 9 bytes", wrap(typ, [2**64] + f[1:] + sig))
    add(f"{name}, chainId with a leading zero", wrap(typ, [b"\x00\x01"] + f[1:] + sig))
    add(f"{name}, chainId as a list", wrap(typ, [[]] + f[1:] + sig))
for typ, f, v in ((0, base["legacy EIP-155"][2], 37), (2, base["type 02"][2], 1)):
    add(f"type {typ}, r as a list", wrap(typ, f + [v, [], 1]))
    add(f"type {typ}, s as a list", wrap(typ, f + [v, 1, [1]]))
    add(f"type {typ}, r of 33 bytes", wrap(typ, f + [v, 2**256, 1]))
    add(f"type {typ}, s of 33 bytes", wrap(typ, f + [v, 1, 2**263]))
    add(f"type {typ}, r with a leading 00", wrap(typ, f + [v, b"\x00" + E.b32(2**255)[1:], 1]))
    add(f"type {typ}, s with a leading 00", wrap(typ, f + [v, 1, b"\x00\x01"]))
    add(f"type {typ}, r = 00", wrap(typ, f + [v, b"\x00", 1]))
add("the EIP-4844 network wrapper", b"\x03" + T.rlp([base["type 03"][2] + sig, [bytes(32)], [bytes(48)], [bytes(48)]]))
assert all(e["status"] == T.INVALID for e in items[nvalid:])

rows = [[e[c] for c in (T.COLUMNS if e["status"] == T.OK else T.COLUMNS[:3])] for e in items]          # one item per line, as a row of T.COLUMNS
T.KATS.write_text('{"eip155": ' + json.dumps(eip155) + ',\n"columns": ' + json.dumps(list(T.COLUMNS)) + ',\n"items": [\n' + ",\n".join(json.dumps(r) for r in rows) + "\n]}\n")
print(f"wrote {T.KATS.name}: {nvalid} valid and {len(items) - nvalid} invalid items, {T.KATS.stat().st_size} bytes")
