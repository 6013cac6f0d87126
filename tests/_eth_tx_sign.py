"""A restatement of plume_eth_tx_sign_batch (include/plume_hip.h) in plain Python, shared by the transaction-signing tests: the framing of an UNSIGNED transaction, the
signed item it becomes, the slot layout of a batch.  Written from the rule as the header states it, over tests/_eth_tx (RLP, the parser), tests/_keccak and
tests/_ecdsa_sign (the signature); nothing here is taken from the library's code.  Its independent pin is EIP-155's worked example and the 108 signed items of
tests/golden/eth_tx_kats.json (tests/test_eth_tx_sign_restatement.py); tests/golden/eth_tx_sign_kats.json holds what it says of the cases that fixture cannot give."""
import json
from pathlib import Path

import numpy as np

from tests import _ecdsa_sign as S
from tests import _eth_tx as T
from tests import _keccak as K

OK, BAD_SCALAR, IDENTITY, SELFCHECK_FAILED, BAD_TX = 0, 2, 4, 8, 16          # PLUME_STATUS_*
GROWTH = 68                                                                  # PLUME_ETH_TX_SIGN_GROWTH
UNSIGNED_ITEMS = {1: 8, 2: 9, 3: 11, 4: 10}                                  # top-level items of an unsigned typed item: the signed count less three
MAX_CHAIN_155 = 2**63 - 18
KATS = Path(__file__).resolve().parent / "golden" / "eth_tx_sign_kats.json"
b32 = T.b32


def frame_unsigned(item: bytes):
    """(tx_type, chain_id, eip155, first, body_end) of a well-framed unsigned item -- body = item[first:body_end] -- or None"""
    item = bytes(item)
    if not item or len(item) >= 2**32:
        return None
    if item[0] >= 0xC0:
        typ, lst = 0, 0
    elif 1 <= item[0] <= 4:
        typ, lst = item[0], 1
    else:
        return None
    outer = T.read_header(item, lst, len(item))
    if outer is None or not outer[0] or outer[2] != len(item):
        return None
    pos, items, starts = outer[1], [], []
    while pos < len(item):                                           # the top-level items tile the payload exactly
        it = T.read_header(item, pos, len(item))
        if it is None or len(items) == 16:
            return None
        items.append(it)
        starts.append(pos)
        pos = it[2]
    if typ:
        if len(items) != UNSIGNED_ITEMS[typ]:
            return None
        chain = T._canonical_int(item, items[0], 8)
        return None if chain is None else (typ, chain, False, outer[1], len(item))
    if len(items) == 6:
        return 0, 0, False, outer[1], len(item)
    if len(items) != 9:
        return None
    chain = T._canonical_int(item, items[6], 8)
    if chain is None or not 1 <= chain <= MAX_CHAIN_155:
        return None
    if item[starts[7]:] != b"\x80\x80":                              # the eighth and ninth: each exactly the empty string
        return None
    return 0, chain, True, outer[1], starts[6]


def assemble(item: bytes, frame, r: int, s: int, parity: int) -> bytes:
    """the signed item of a framed unsigned one, for ANY r and s (the lane tests choose values no signer produces)"""
    typ, chain, eip155, first, body_end = frame
    v = parity if typ else parity + (35 + 2 * chain if eip155 else 27)
    payload = bytes(item[first:body_end]) + T.rlp(v) + T.rlp(r) + T.rlp(s)
    return (bytes([typ]) if typ else b"") + T.list_of(payload)


def sign_tx(item: bytes, sk32: bytes, aux: bytes = None):
    """(raw, hash32, r, s, parity, status) as plume_eth_tx_sign_batch reports item: BAD_TX alone for an ill-framed item, else the signer's status; any status: raw empty,
    the records zero"""
    item = bytes(item)
    fr = frame_unsigned(item)
    if fr is None:
        return b"", bytes(32), 0, 0, 0, BAD_TX
    h = S._hash_cached(item, S.KECCAK256)                                # (cached: the GPU tests ask for the same batch several times)
    r, s, parity, st = S._sign_cached(bytes(sk32), h, None if aux is None else bytes(aux))
    if st == OK and fr[2] and 35 + 2 * fr[1] + parity >= 2**64:         # chainId 2^63 - 18 with parity 1: a v that 64 bits (and the parser) do not hold
        st = IDENTITY
    if st != OK:
        return b"", bytes(32), 0, 0, 0, st
    return assemble(item, fr, r, s, parity), h, r, s, parity, OK


def unsigned_of(raw: bytes) -> bytes:
    """the unsigned serialization of a valid signed item: what its sender hashed"""
    raw = bytes(raw)
    p = T.parse(raw)
    assert p is not None
    _, _, _, _, chain, typ = p
    lst = 1 if typ else 0
    outer = T.read_header(raw, lst, len(raw))
    pos, starts = outer[1], []
    for _ in range(T.ITEMS[typ]):
        starts.append(pos)
        pos = T.read_header(raw, pos, len(raw))[2]
    body = raw[outer[1]:starts[-3]]
    if typ:
        return bytes([typ]) + T.list_of(body)
    v = int.from_bytes(raw[T.read_header(raw, starts[-3], len(raw))[1]:starts[-2]], "big")
    return T.list_of(body + (T.rlp(chain) + b"\x80\x80" if v >= 37 else b""))


def slot_bounds(off):
    """(start, length) of every slot for offsets off[0 .. n]"""
    off = [int(o) for o in off]
    return [(off[i] - off[0] + GROWTH * i, off[i + 1] - off[i] + GROWTH) for i in range(len(off) - 1)]


def sign_batch(txs, off, sk, aux=None, out_bytes=None, txs_bytes=None):
    """what plume_eth_tx_sign_batch* writes: {"out" uint8[out_bytes], "out_len" uint32[n], "hash" "r" "s" uint8[n, 32], "v" "tx_type" "status" uint8[n], "chain_id"
    uint64[n]}.  out_bytes / txs_bytes: the device form's limits (an item whose offsets are rejected or whose slot reaches past out_bytes reports BAD_TX and writes nothing)"""
    tb = bytes(txs) if isinstance(txs, (bytes, bytearray)) else np.ascontiguousarray(txs, dtype=np.uint8).tobytes()
    as_bytes = lambda a: a if isinstance(a, (bytes, bytearray)) else np.ascontiguousarray(a, dtype=np.uint8).tobytes()  # noqa: E731
    sb, ab = as_bytes(sk), None if aux is None else as_bytes(aux)
    n = len(off) - 1
    full = int(off[n]) - int(off[0]) + GROWTH * n if n else 0
    out_bytes = full if out_bytes is None else out_bytes
    nbytes = len(tb) if txs_bytes is None else txs_bytes
    o = {"out": np.zeros(out_bytes, np.uint8), "out_len": np.zeros(n, np.uint32), "hash": np.zeros((n, 32), np.uint8), "r": np.zeros((n, 32), np.uint8),
         "s": np.zeros((n, 32), np.uint8), "v": np.zeros(n, np.uint8), "chain_id": np.zeros(n, np.uint64), "tx_type": np.zeros(n, np.uint8), "status": np.zeros(n, np.uint8)}
    for i in range(n):
        o0, o1 = int(off[i]), int(off[i + 1])
        start = o0 - int(off[0]) + GROWTH * i
        if not (int(off[0]) <= o0 <= o1 <= nbytes) or start + (o1 - o0) + GROWTH > out_bytes:
            o["status"][i] = BAD_TX
            continue
        item = tb[o0:o1]
        raw, h, r, s, parity, st = sign_tx(item, sb[32 * i:32 * i + 32], None if ab is None else ab[32 * i:32 * i + 32])
        o["status"][i] = st
        if st != OK:
            continue
        fr = frame_unsigned(item)
        o["out"][start:start + len(raw)] = np.frombuffer(raw, np.uint8)
        o["out_len"][i] = len(raw)
        o["hash"][i], o["r"][i], o["s"][i] = np.frombuffer(h, np.uint8), np.frombuffer(b32(r), np.uint8), np.frombuffer(b32(s), np.uint8)
        o["v"][i], o["chain_id"][i], o["tx_type"][i] = parity, fr[1], fr[0]
    return o


def compact(out, out_len, off):
    """the signed items of a slotted buffer, as a list of bytes"""
    ob = np.ascontiguousarray(out, dtype=np.uint8).tobytes()
    return [ob[st:st + int(out_len[i])] for i, (st, _) in enumerate(slot_bounds(off))]


def fixture_batch():
    """(unsigned items, keys) of both fixtures as one batch of about 300 items: the 108 signed low-s items of eth_tx_kats.json taken apart, each followed by the signed
    (or invalid) item itself as an input the framing rejects, and after every fourth of them one of the new vectors -- valid and invalid items interleaved inside every
    64-lane wavefront, the two ~65 KB items next to 100-byte ones"""
    old_items, old_keys = [], []
    for e in T.load_kats()["items"]:
        raw = bytes.fromhex(e["raw"])
        sk = bytes.fromhex(e["sk"]) if e["sk"] else b32(len(old_items) + 1)
        if e["sk"] and not e["high_s"] and e["status"] == T.OK:
            old_items.append(unsigned_of(raw))
            old_keys.append(sk)
        if len(raw) < 1000:
            old_items.append(raw)
            old_keys.append(sk)
    new = [(bytes.fromhex(e["unsigned"]), bytes.fromhex(e["sk"])) for e in load_kats()["items"]]
    items, keys = [], []
    for j, (it, sk) in enumerate(zip(old_items, old_keys)):
        items.append(it)
        keys.append(sk)
        if j % 4 == 3 and new:
            it2, sk2 = new.pop(0)
            items.append(it2)
            keys.append(sk2)
    for it2, sk2 in new:
        items.append(it2)
        keys.append(sk2)
    # the fixtures end in runs of invalid items: deal the framed and the unframed items out evenly, each kind in its order
    good = [j for j, it in enumerate(items) if frame_unsigned(it) is not None]
    bad = [j for j, it in enumerate(items) if frame_unsigned(it) is None]
    order, a, b = [], 0, 0
    while a < len(good) or b < len(bad):
        if b >= len(bad) or (a < len(good) and a * len(bad) <= b * len(good)):
            order.append(good[a])
            a += 1
        else:
            order.append(bad[b])
            b += 1
    return [items[j] for j in order], [keys[j] for j in order]


def load_kats():
    """the committed vectors: {"items": [{name, unsigned, sk, status, raw}]}: hex strings, raw empty unless status is 0.  A long unsigned / raw is written as
    [hex, [unit hex, count], hex], as tests/golden/eth_tx_kats.json writes them; undone here"""
    kats = json.loads(KATS.read_text())

    def expand(x):
        if isinstance(x, str):
            return x
        head, (unit, count), tail = x
        return head + unit * count + tail
    for e in kats["items"]:
        e["unsigned"], e["raw"] = expand(e["unsigned"]), expand(e["raw"])
    return kats
