"""The lane body of plume_eth_tx_parse_batch (zk-nullifier-sig_amd/csrc/plume_eth_tx.h, over the stream of csrc/plume_keccak.h) on the host: tests/eth_tx/eth_tx_lanes.cpp,
a stand-alone program built by its Makefile with g++ under AddressSanitizer + UBSan and -Werror, against the restatement of tests/_eth_tx.py.  The whole fixture as one
batch, at every start residue of the buffer, outputs at odd offsets with the bytes around them untouched and each optional array absent in turn; every item alone at each
of the eight start residues in an allocation that ends with its last byte (the bounds of the aligned loads); 2 000 seeded single-byte mutants of valid items in every
output; offsets the span rule rejects."""
import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import _eth_tx as T

ROOT = Path(__file__).resolve().parent.parent
G = b"\xAA" * 32
NAMES = ("hash", "r", "s", "v", "chain_id", "tx_type", "status")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("no g++ / make")
    out = tmp_path_factory.mktemp("eth_tx_lanes")
    subprocess.run(["make", "-C", str(ROOT / "tests" / "eth_tx"), f"OUT={out}"], check=True, capture_output=True, text=True, timeout=900)
    return out / "eth_tx_lanes"


@pytest.fixture(scope="module")
def kats():
    items = T.load_kats()["items"]
    raws = [bytes.fromhex(e["raw"]) for e in items]
    txs, off = T.pack(raws)
    want = {"hash": b"".join(bytes.fromhex(e["hash"]) for e in items), "r": b"".join(bytes.fromhex(e["r"]) for e in items), "s": b"".join(bytes.fromhex(e["s"]) for e in items),
            "v": bytes(e["v"] for e in items), "chain_id": np.array([int(e["chain_id"]) for e in items], np.uint64).tobytes(), "tx_type": bytes(e["tx_type"] for e in items),
            "status": bytes(e["status"] for e in items)}
    return raws, txs, off, want


def _exec(harness, mode, tmp_path, n, mis, mis_out, present, nbytes, off, buf):
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<4IQ", n, mis, mis_out, present, nbytes) + np.asarray(off, np.uint64).tobytes() + bytes(buf[:nbytes]))
    r = subprocess.run([str(harness), mode, str(fin), str(fout)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "eth_tx_lanes ok" in r.stdout, (mode, r.returncode, r.stdout[-500:], r.stderr[-4000:])
    return fout.read_bytes()


def _check_batch(got, want, present, what):
    pos = 0
    for k, name in enumerate(NAMES):
        if k >= 4 and not (present >> (k - 4)) & 1:
            continue
        seg = got[pos:pos + 64 + len(want[name])]
        pos += len(seg)
        assert seg[:32] == G and seg[-32:] == G, f"{name}: bytes outside the array were written ({what})"
        assert seg[32:-32] == want[name], f"{name} ({what})"
    assert pos == len(got)


def _as_bytes(out):
    return {k: out[k].tobytes() for k in NAMES}


def test_the_whole_fixture_as_one_batch(harness, tmp_path, kats):
    raws, txs, off, want = kats
    for mis, mis_out, present in ((0, 0, 7), (1, 3, 7), (2, 5, 6), (3, 7, 5), (4, 8, 3), (5, 9, 7), (6, 13, 0), (7, 15, 7), (9, 1, 7)):
        got = _exec(harness, "parse", tmp_path, len(raws), mis, mis_out, present, len(txs), off, txs.tobytes())
        _check_batch(got, want, present, f"misalign={mis}, outputs at {mis_out}, present={present:03b}")


def test_every_item_alone_at_each_start_residue(harness, tmp_path, kats):
    raws, txs, off, want = kats
    n = len(raws)
    got = _exec(harness, "each", tmp_path, n, 0, 0, 7, len(txs), off, txs.tobytes())
    per = sum(len(want[k]) for k in NAMES)
    assert len(got) == 8 * per
    for m in range(8):
        pos = m * per
        for name in NAMES:
            seg = got[pos:pos + len(want[name])]
            pos += len(seg)
            if seg != want[name]:
                w = len(seg) // n
                bad = [T.load_kats()["items"][i]["name"] for i in range(n) if seg[w * i:w * i + w] != want[name][w * i:w * i + w]]
                raise AssertionError(f"{name} at start residue {m}: {bad[:5]}")


def test_two_thousand_single_byte_mutants(harness, tmp_path, kats):
    raws = [r for r, st in zip(kats[0], kats[3]["status"]) if st == T.OK and len(r) < 1000]
    muts = T.mutants(raws, 2000, 20261018)
    txs, off = T.pack(muts)
    want = T.parse_batch(txs, off)
    valid = int((want["status"] == T.OK).sum())
    assert 200 <= valid <= 1800, valid                                       # both outcomes are well represented
    got = _exec(harness, "parse", tmp_path, len(muts), 3, 1, 7, len(txs), off, txs.tobytes())
    _check_batch(got, _as_bytes(want), 7, "mutants")


def test_rejected_offsets_are_invalid_and_never_read(harness, tmp_path, kats):
    raws = [r for r in kats[0] if len(r) < 1000][:12]
    txs, off = T.pack(raws)
    bad = off.copy()
    bad[2] = bad[1] - 3                                                      # item 1 runs backwards; item 2 starts inside item 0's tail
    got = _exec(harness, "parse", tmp_path, len(raws), 5, 0, 7, len(txs), bad, txs.tobytes())
    _check_batch(got, _as_bytes(T.parse_batch(txs, bad)), 7, "decreasing offsets")
    cut = int(off[6]) + 1                                                    # the buffer ends inside item 6: it and everything behind it reach past the allocation
    want = T.parse_batch(txs, off, txs_bytes=cut)
    assert (want["status"][6:] == T.INVALID).all()
    got = _exec(harness, "parse", tmp_path, len(raws), 0, 0, 7, cut, off, txs.tobytes())
    _check_batch(got, _as_bytes(want), 7, "offsets past the buffer")
    got = _exec(harness, "parse", tmp_path, 0, 0, 0, 7, 0, np.zeros(1, np.uint64), b"")
    assert got == (G + G) * 7
