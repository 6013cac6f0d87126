"""The lane bodies of plume_eth_tx_sign_batch (zk-nullifier-sig_amd/csrc/plume_eth_tx_sign.h) on the host: tests/eth_tx_sign/eth_tx_sign_lanes.cpp, a stand-alone program
built by its Makefile with g++ under AddressSanitizer + UBSan and -Werror, against the restatement of tests/_eth_tx_sign.py.  Both fixtures go through frame -> the
restatement's ECDSA -> assemble as one batch, at several start residues of the input and the output, in allocations that end with their last byte, the lanes run in both
orders; every item alone with its slot between guard bytes at each of the eight residues; the assemble body with CHOSEN r and s that no signer produces (the single-byte
form, leading zeros, the short signed-list header); offsets the span rule rejects and an out_bytes that cuts a slot."""
import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import _ecdsa_sign as S
from tests import _eth_tx as T
from tests import _eth_tx_sign as X
from tests import _keccak as K

ROOT = Path(__file__).resolve().parent.parent
G = b"\xAA" * 32
RECORDS = ("hash", "r", "s", "v", "chain_id", "tx_type")
UNWRITTEN = 0x55                                                             # what the harness fills out with


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("no g++ / make")
    out = tmp_path_factory.mktemp("eth_tx_sign_lanes")
    subprocess.run(["make", "-C", str(ROOT / "tests" / "eth_tx_sign"), f"OUT={out}"], check=True, capture_output=True, text=True, timeout=900)
    return out / "eth_tx_sign_lanes"


def staged_signature(item, sk):
    """what the sign stages leave for the item: the signature over its hash for a framed item, over the zero hash for any other (discarded by the assemble)"""
    h = K.keccak256(item) if X.frame_unsigned(item) is not None else bytes(32)
    r, s, v, st = S._sign_cached(bytes(sk), h, None)
    return S.b32(r), S.b32(s), v, st


@pytest.fixture(scope="module")
def batch():
    items, keys = X.fixture_batch()
    txs, off = T.pack(items)
    sig = [staged_signature(it, sk) for it, sk in zip(items, keys)]
    return items, keys, txs, off, sig


def _exec(harness, mode, tmp_path, mis, mis_out, present, off, buf, sig, out_bytes=None, nbytes=None):
    n = len(off) - 1
    nbytes = len(buf) if nbytes is None else nbytes
    out_bytes = int(off[n]) - int(off[0]) + X.GROWTH * n if out_bytes is None else out_bytes
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<4IQQ", n, mis, mis_out, present, nbytes, out_bytes) + np.asarray(off, np.uint64).tobytes() + bytes(buf[:nbytes]) +
                    b"".join(g[0] for g in sig) + b"".join(g[1] for g in sig) + bytes(g[2] for g in sig) + bytes(g[3] for g in sig))
    r = subprocess.run([str(harness), mode, str(fin), str(fout)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "eth_tx_sign_lanes ok" in r.stdout, (mode, r.returncode, r.stdout[-500:], r.stderr[-4000:])
    return fout.read_bytes(), out_bytes


def _check_batch(got, out_bytes, want, off, present, what, staged_hash=None):
    n = len(off) - 1
    pos = 48 * n
    if staged_hash is not None:
        assert got[16 * n:48 * n] == staged_hash, f"the staged hash ({what})"
    out = np.frombuffer(got[pos:pos + out_bytes], np.uint8)
    pos += out_bytes
    written = np.zeros(out_bytes, bool)
    for i, (start, length) in enumerate(X.slot_bounds(off)):
        if want["slotted"][i]:
            written[start:start + length] = True
    assert (out[~written] == UNWRITTEN).all(), f"bytes of out that belong to no slot were written ({what})"
    bad = np.flatnonzero(written & (out != want["out"][:out_bytes]))
    assert bad.size == 0, f"out differs first at byte {bad[:1]} ({what})"
    for name, data in [("out_len", want["out_len"].tobytes()), ("status", want["status"].tobytes())] + [(k, want[k].tobytes()) for j, k in enumerate(RECORDS) if (present >> j) & 1]:
        seg = got[pos:pos + 64 + len(data)]
        pos += len(seg)
        assert seg[:32] == G and seg[-32:] == G, f"{name}: bytes outside the array were written ({what})"
        assert seg[32:-32] == data, f"{name} ({what})"
    assert pos == len(got)


def _want(txs, off, keys, out_bytes=None, txs_bytes=None):
    w = X.sign_batch(txs, off, b"".join(keys), out_bytes=out_bytes, txs_bytes=txs_bytes)
    nbytes = len(txs) if txs_bytes is None else txs_bytes
    ob = len(w["out"])
    # an item with sound offsets whose slot ends inside out has a slot (written, zero if it reports a status); any other writes no byte of out
    w["slotted"] = [int(off[0]) <= int(off[i]) <= int(off[i + 1]) <= nbytes and st + ln <= ob for i, (st, ln) in enumerate(X.slot_bounds(off))]
    return w


def test_both_fixtures_as_one_batch(harness, tmp_path, batch):
    items, keys, txs, off, sig = batch
    assert len(items) > 250
    want = _want(txs, off, keys)
    assert (want["status"] == 0).sum() == 108 + 4 + 11 and (want["status"] == X.BAD_TX).sum() > 100 and (want["status"] == X.BAD_SCALAR).sum() == 3
    assert (want["status"] == X.IDENTITY).sum() == 1                          # chainId 2^63 - 18 with parity 1: decided by the assemble
    assert (want["out_len"] <= np.diff(off).astype(np.int64) + X.GROWTH).all()
    hashes = b"".join(K.keccak256(it) if X.frame_unsigned(it) is not None else bytes(32) for it in items)
    for mis, mis_out, present in ((0, 0, 63), (1, 3, 63), (2, 5, 0), (3, 7, 21), (4, 8, 42), (5, 9, 63), (7, 15, 63)):
        got, ob = _exec(harness, "batch", tmp_path, mis, mis_out, present, off, txs.tobytes(), sig)
        _check_batch(got, ob, want, off, present, f"misalign={mis}, outputs at {mis_out}, present={present:06b}", hashes)


def test_every_item_alone_at_each_slot_residue(harness, tmp_path, batch):
    items, keys, txs, off, sig = batch
    want = _want(txs, off, keys)
    got, _ = _exec(harness, "each", tmp_path, 0, 0, 63, off, txs.tobytes(), sig)
    pos = 0
    for m in range(8):
        for i, (start, length) in enumerate(X.slot_bounds(off)):
            slot, ln, st = got[pos:pos + length], struct.unpack_from("<I", got, pos + length)[0], got[pos + length + 4]
            pos += length + 5
            assert (ln, st) == (int(want["out_len"][i]), int(want["status"][i])), (m, i)
            assert slot == want["out"][start:start + length].tobytes(), f"item {i} at slot residue {m}"
    assert pos == len(got)


CHOSEN = (1, 0x7F, 0x80, 2**8, 2**240 - 1, 2**248, 2**256 - 1)


def test_assemble_with_chosen_r_and_s(harness, tmp_path):
    """values no signer produces: the single-byte form of rlp_int, two and more leading zero bytes, a signed list short enough for the one-byte header"""
    shortest = {0: T.rlp([0, 1, 1, b"", 0, b""]), 155: T.rlp([0, 1, 1, b"", 0, b"", 1, 0, 0]), 2: b"\x02" + T.rlp([1, 0, 1, 1, 1, b"", 0, b"", []])}
    longer = {0: T.signing_data(0, T.default_fields(0, 0, b"\x07" * 40, 2)), 155: T.signing_data(0, T.default_fields(0, 2**40, b"", 2), 2**40),
              2: T.signing_data(2, T.default_fields(2, 1, b"\x07" * 200, 2))}
    items, sig, raws = [], [], []
    for unsigned in list(shortest.values()) + list(longer.values()):
        fr = X.frame_unsigned(unsigned)
        assert fr is not None
        for r in CHOSEN:
            for s in CHOSEN:
                parity = (r ^ s) & 1
                items.append(unsigned)
                sig.append((S.b32(r), S.b32(s), parity, 0))
                raws.append(X.assemble(unsigned, fr, r, s, parity))
    assert min(len(r) for r in raws) < 20 and any(r[0] < 0xF8 and r[0] >= 0xC0 for r in raws)       # the short signed-list header is reached
    txs, off = T.pack(items)
    n = len(items)
    want = {"out": np.zeros(len(txs) + X.GROWTH * n, np.uint8), "out_len": np.array([len(r) for r in raws], np.uint32), "status": np.zeros(n, np.uint8),
            "slotted": [True] * n, "r": np.frombuffer(b"".join(g[0] for g in sig), np.uint8), "s": np.frombuffer(b"".join(g[1] for g in sig), np.uint8),
            "v": np.array([g[2] for g in sig], np.uint8)}
    for (start, _), raw in zip(X.slot_bounds(off), raws):
        want["out"][start:start + len(raw)] = np.frombuffer(raw, np.uint8)
        assert T.parse(raw) is not None
    for mis, mis_out in ((0, 0), (3, 5), (6, 1)):
        got, ob = _exec(harness, "batch", tmp_path, mis, mis_out, 2 | 4 | 8, off, txs.tobytes(), sig)
        _check_batch(got, ob, want, off, 2 | 4 | 8, f"chosen r, s; misalign={mis}, outputs at {mis_out}")


def test_rejected_offsets_and_a_cut_slot(harness, tmp_path, batch):
    items, keys = batch[0], batch[1]
    pick = [i for i, it in enumerate(items) if len(it) < 1000 and X.frame_unsigned(it) is not None][:12]
    items, keys = [items[i] for i in pick], [keys[i] for i in pick]
    sig = [staged_signature(it, sk) for it, sk in zip(items, keys)]
    txs, off = T.pack(items)
    bad = off.copy()
    bad[2] = bad[1] - 3                                                      # item 1 runs backwards; item 2 starts inside item 0's tail and overlaps its slot
    sig_bad = list(sig)
    sig_bad[2] = staged_signature(txs.tobytes()[int(bad[2]):int(bad[3])], keys[2])
    want = _want(txs, bad, keys)
    assert want["status"][1] == X.BAD_TX and want["status"][2] == X.BAD_TX   # (a slice that starts mid-item is no transaction)
    got, ob = _exec(harness, "batch", tmp_path, 5, 3, 63, bad, txs.tobytes(), sig_bad)
    n = len(items)
    assert got[48 * n + ob + 32 + 4 * n + 32 + 32:][:n] == want["status"].tobytes()
    # the buffer ends inside item 6: it and everything behind it reach past the allocation and never read it
    cut = int(off[6]) + 1
    want = _want(txs, off, keys, txs_bytes=cut)
    assert (want["status"][6:] == X.BAD_TX).all() and (want["status"][:6] == 0).all()
    got, ob = _exec(harness, "batch", tmp_path, 0, 1, 63, off, txs.tobytes(), sig, nbytes=cut)
    _check_batch(got, ob, want, off, 63, "offsets past the buffer")
    # an out_bytes that cuts the last slot by one byte, and one that cuts slot 4
    for cut_item, spare in ((n - 1, -1), (4, 10)):
        start, length = X.slot_bounds(off)[cut_item]
        ob = start + (length + spare if spare < 0 else spare)
        want = _want(txs, off, keys, out_bytes=ob)
        assert (want["status"][:cut_item] == 0).all() and (want["status"][cut_item:] == X.BAD_TX).all()
        got, ob2 = _exec(harness, "batch", tmp_path, 2, 7, 63, off, txs.tobytes(), sig, out_bytes=ob)
        _check_batch(got, ob2, want, off, 63, f"out_bytes cuts slot {cut_item}")
    got, _ = _exec(harness, "batch", tmp_path, 0, 0, 63, np.zeros(1, np.uint64), b"", [], out_bytes=0)
    assert got == (G + G) * 8
