"""A restatement of plume_eth_tx_parse_batch / plume_eth_tx_sender_batch (include/plume_hip.h) in plain Python, shared by the transaction tests: an RLP encoder, the
per-item rule -- envelope, top-level framing, v, the signing hash -- as a parser that returns (hash, r, s, v, chain_id, type) or None, and a builder that signs with
tests/_ecdsa_sign.sign.  Written from the rule as the header states it, over Python lists and integers; nothing here is taken from the library's code.  Its independent
pin is EIP-155's worked example (tests/test_eth_tx_restatement.py); tests/golden/eth_tx_kats.json holds what it says of every kind of item."""
import json
from pathlib import Path

import numpy as np

from tests import _ecdsa as E
from tests import _ecdsa_sign as S
from tests import _keccak as K

OK, INVALID = 1, 3                                               # PLUME_ETH_TX_*
KATS = Path(__file__).resolve().parent / "golden" / "eth_tx_kats.json"
ITEMS = {0: 9, 1: 11, 2: 12, 3: 14, 4: 13}                       # top-level items per tx_type
COLUMNS = ("name", "raw", "status", "sk", "high_s", "hash", "r", "s", "v", "chain_id", "tx_type")      # a row of the fixture
b32 = E.b32


# ------------------------------------------------------------------------------------------------ RLP
def rlp_int(v: int) -> bytes:
    """the big-endian bytes of a canonical integer: none for zero"""
    return v.to_bytes((v.bit_length() + 7) // 8, "big")


def _header(n: int, base: int) -> bytes:
    if n <= 55:
        return bytes([base + n])
    nb = rlp_int(n)
    return bytes([base + 55 + len(nb)]) + nb


def rlp(x) -> bytes:
    """bytes -> a string, int -> a canonical integer, list / tuple -> a list"""
    if isinstance(x, int):
        x = rlp_int(x)
    if isinstance(x, (bytes, bytearray)):
        x = bytes(x)
        return x if len(x) == 1 and x[0] < 0x80 else _header(len(x), 0x80) + x
    body = b"".join(rlp(e) for e in x)
    return _header(len(body), 0xC0) + body


def list_of(body: bytes) -> bytes:
    return _header(len(body), 0xC0) + body


def read_header(buf: bytes, pos: int, end: int):
    """the canonical header at buf[pos:end]: (is_list, payload start, payload end), or None"""
    if pos >= end:
        return None
    b = buf[pos]
    if b < 0x80:
        return False, pos, pos + 1
    is_list, t = b >= 0xC0, b - (0xC0 if b >= 0xC0 else 0x80)
    if t <= 55:
        start, n = pos + 1, t
        if start + n > end:
            return None
        if not is_list and n == 1 and buf[start] < 0x80:
            return None
    else:
        ll = t - 55
        start = pos + 1 + ll
        if start > end or buf[pos + 1] == 0:
            return None
        n = int.from_bytes(buf[pos + 1:start], "big")
        if n <= 55 or start + n > end:
            return None
    return is_list, start, start + n


def _canonical_int(buf, item, max_bytes):
    is_list, a, b = item
    if is_list or b - a > max_bytes or (b > a and buf[a] == 0):
        return None
    return int.from_bytes(buf[a:b], "big")


# ------------------------------------------------------------------------------------------------ the per-item rule
def parse(raw: bytes):
    """(hash32, r, s, v, chain_id, tx_type) with r, s integers, or None for an invalid item"""
    raw = bytes(raw)
    if not raw or len(raw) >= 2**32:
        return None
    if raw[0] >= 0xC0:
        typ, lst = 0, 0
    elif 1 <= raw[0] <= 4:
        typ, lst = raw[0], 1
    else:
        return None
    outer = read_header(raw, lst, len(raw))
    if outer is None or not outer[0] or outer[2] != len(raw):
        return None
    pos, items, starts = outer[1], [], []
    for _ in range(ITEMS[typ]):
        it = read_header(raw, pos, len(raw))
        if it is None:
            return None
        items.append(it)
        starts.append(pos)
        pos = it[2]
    if pos != len(raw):
        return None
    v = _canonical_int(raw, items[-3], 8)
    r = _canonical_int(raw, items[-2], 32)
    s = _canonical_int(raw, items[-1], 32)
    if v is None or r is None or s is None:
        return None
    body = raw[outer[1]:starts[-3]]
    if typ == 0:
        if v in (27, 28):
            parity, chain, pre = v - 27, 0, list_of(body)
        elif v >= 37:
            parity, chain = (v - 35) & 1, (v - 35) >> 1
            pre = list_of(body + rlp(chain) + b"\x80\x80")
        else:
            return None
    else:
        chain = _canonical_int(raw, items[0], 8)
        if chain is None or v > 1:
            return None
        parity, pre = v, bytes([typ]) + list_of(body)
    return K.keccak256(pre), r, s, parity, chain, typ


def parse_batch(txs, off, txs_bytes=None):
    """what plume_eth_tx_parse_batch writes: hash, r, s uint8[n, 32]; v, tx_type, status uint8[n]; chain_id uint64[n].  An item whose offsets decrease or reach past
    txs_bytes is invalid"""
    tb = bytes(txs) if isinstance(txs, (bytes, bytearray)) else np.ascontiguousarray(txs, dtype=np.uint8).tobytes()
    nbytes = len(tb) if txs_bytes is None else txs_bytes
    n = len(off) - 1
    out = {"hash": np.zeros((n, 32), np.uint8), "r": np.zeros((n, 32), np.uint8), "s": np.zeros((n, 32), np.uint8), "v": np.zeros(n, np.uint8),
           "chain_id": np.zeros(n, np.uint64), "tx_type": np.zeros(n, np.uint8), "status": np.full(n, INVALID, np.uint8)}
    for i in range(n):
        o0, o1 = int(off[i]), int(off[i + 1])
        p = parse(tb[o0:o1]) if o0 <= o1 <= nbytes else None
        if p is None:
            continue
        out["hash"][i], out["r"][i], out["s"][i] = np.frombuffer(p[0], np.uint8), np.frombuffer(b32(p[1]), np.uint8), np.frombuffer(b32(p[2]), np.uint8)
        out["v"][i], out["chain_id"][i], out["tx_type"][i], out["status"][i] = p[3], p[4], p[5], OK
    return out


def pack(raws):
    """(txs uint8[], tx_off uint64[n + 1])"""
    off = np.concatenate([[0], np.cumsum([len(r) for r in raws])]).astype(np.uint64)
    return np.frombuffer(b"".join(raws), np.uint8).copy(), off


# ------------------------------------------------------------------------------------------------ the builder
def default_fields(typ: int, chain_id: int, data: bytes = b"", salt: int = 0):
    """the unsigned fields of a plausible transaction of the kind, in order (typed: chainId first)"""
    to = bytes((0x35 + salt + j) & 0xFF for j in range(20))
    access = [[to, [b32(salt + 1), b32(salt + 2)]]] if salt % 4 == 1 else []
    if typ == 0:
        return [9 + salt, 20 * 10**9, 21000, to, 10**18 + salt, data]
    if typ == 1:
        return [chain_id, salt, 20 * 10**9, 21000, to, 10**18, data, access]
    if typ == 2:
        return [chain_id, salt, 2 * 10**9, 30 * 10**9, 21000, to, 10**18, data, access]
    if typ == 3:
        return [chain_id, salt, 2 * 10**9, 30 * 10**9, 21000, to, 0, data, access, 10**9, [b"\x01" + bytes(31)]]
    if typ == 4:
        return [chain_id, salt, 2 * 10**9, 30 * 10**9, 21000, to, 0, data, access, [[chain_id, to, 1, 0, 1, 1]]]
    raise ValueError("type")


def signing_data(typ: int, fields, chain_id: int = 0) -> bytes:
    """what the sender hashes; legacy: chain_id 0 = unprotected"""
    if typ == 0:
        return rlp(list(fields) + ([chain_id, 0, 0] if chain_id else []))
    return bytes([typ]) + rlp(fields)


def assemble(typ: int, fields, v: int, r, s) -> bytes:
    """the raw item: fields, then v / yParity, r, s (each an int, or bytes / a list taken as given)"""
    return (b"" if typ == 0 else bytes([typ])) + rlp(list(fields) + [v, r, s])


def build(typ: int, sk32: bytes, chain_id: int = 0, data: bytes = b"", salt: int = 0, fields=None, high_s: bool = False):
    """a signed transaction: (raw, hash32, r, s, parity).  high_s: the other s of the same signature, above (n - 1) / 2"""
    fields = default_fields(typ, chain_id, data, salt) if fields is None else fields
    h = K.keccak256(signing_data(typ, fields, chain_id))
    r, s, parity, st = S.sign(sk32, h, fast=True)
    assert st == S.OK
    if high_s:
        s, parity = E.N - s, parity ^ 1
    v = parity if typ else parity + (35 + 2 * chain_id if chain_id else 27)
    return assemble(typ, fields, v, r, s), h, r, s, parity


def sender_of(sk32: bytes):
    """(pk point, address20) of a key"""
    q = E.mul(int.from_bytes(sk32, "big"))
    return q, K.address_of(q)


def mutants(raws, count: int, seed: int):
    """`count` seeded single-byte mutants of the given items: one byte replaced, inserted or deleted"""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(count):
        raw = bytearray(raws[int(rng.integers(len(raws)))])
        pos, kind = int(rng.integers(len(raw))), int(rng.integers(4))
        if kind <= 1:
            raw[pos] = int(rng.integers(256)) if kind == 0 else raw[pos] ^ (1 << int(rng.integers(8)))
        elif kind == 2:
            raw.insert(pos, int(rng.integers(256)))
        else:
            del raw[pos]
        out.append(bytes(raw))
    return out


def load_kats():
    """the committed vectors: {"eip155": {...}, "items": [{name, raw, sk, status, hash, r, s, v, chain_id, tx_type, high_s}]}: hex strings, chain_id a decimal string,
    sk null for an item nobody signed.  The file holds an item as a row of COLUMNS, writes a long item's raw as [hex, [unit hex, count], hex] and ends the row of an
    invalid item, whose records are all zero, behind its status: all three are undone here"""
    kats = json.loads(KATS.read_text())
    assert tuple(kats.pop("columns")) == COLUMNS
    zero = {"sk": None, "high_s": False, "hash": bytes(32).hex(), "r": bytes(32).hex(), "s": bytes(32).hex(), "v": 0, "chain_id": "0", "tx_type": 0}
    for i, row in enumerate(kats["items"]):
        e = dict(zero, **dict(zip(COLUMNS, row)))
        if not isinstance(e["raw"], str):
            head, (unit, count), tail = e["raw"]
            e["raw"] = head + unit * count + tail
        assert (len(row) == len(COLUMNS)) == (e["status"] == OK)
        kats["items"][i] = e
    return kats
