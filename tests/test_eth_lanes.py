"""k_eth_address's lane body (zk-nullifier-sig_amd/csrc/plume_keccak.h) on the host: tests/eth/eth_lanes.cpp compiled with g++ under AddressSanitizer + UBSan and
-Werror, against the restatement of tests/_keccak.py (itself pinned by tests/test_eth_keccak_restatement.py).  Both key formats x the three address formats x expect
absent / matching / wrong in each of its 20 bytes x every kind of invalid key x odd and even y x NULL address / NULL status x all sixteen offsets of the arrays from a
16-byte boundary (offset 0 takes the 16-byte loads and stores, the others the byte + quad + byte paths) x batch sizes that end inside a quad; the bytes around every
array stay at their pre-fill and the inputs are not written."""
import itertools
import json
import os
import shutil
import struct
import subprocess
from pathlib import Path

import pytest

from tests import _keccak as K

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "zk-nullifier-sig_amd" / "csrc"
KATS = json.loads((ROOT / "tests" / "golden" / "eth_address_kats.json").read_text())
PKF = {"affine64": 0, "sec1": 1}
ADF = {"raw20": 0, "record64": 1, "eip55": 2}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("eth_lanes") / "eth_lanes"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}",
                    str(ROOT / "tests" / "eth" / "eth_lanes.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True, timeout=600)
    return exe


@pytest.fixture(scope="module")
def batches():
    """per key format: 47 keys -- valid ones of both parities with every invalid kind planted among them -- and their raw addresses (None: invalid), computed once"""
    out = {}
    for fmt in PKF:
        keys = [k.tobytes() for k in K.sample_keys(40, 11 + PKF[fmt], fmt)]
        assert {k[-1] & 1 for k in keys} == {0, 1} if fmt == "affine64" else {k[0] for k in keys} == {2, 3}
        for j, (_, rec) in enumerate(K.invalid_keys(fmt)):
            keys.insert(5 * j, rec)
        keys = keys[:48]
        pts = [K.decode_pk(k, fmt) for k in keys]
        out[fmt] = (keys, [None if p is None else K.address_of(p) for p in pts])
        assert sum(a is None for a in out[fmt][1]) == len(K.invalid_keys(fmt))
    return out


def _expected(addrs, expect, addr_format):
    W = K.ADDR_WIDTH[addr_format]
    recs = b"".join(bytes(W) if a is None else K.record_of(a, addr_format) for a in addrs)
    st = bytes(K.INVALID if a is None else K.MATCH if expect is None or expect[i] == a else K.MISMATCH for i, a in enumerate(addrs))
    return recs, st


def _run(harness, tmp_path, keys, addrs, pk_format, addr_format, mis, expect=None, address=True, status=True):
    n = len(keys)
    present = (1 if address else 0) | (2 if status else 0) | (4 if expect is not None else 0)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<5I", n, PKF[pk_format], ADF[addr_format], mis, present) + b"".join(keys) + (b"".join(expect) if expect is not None else b""))
    r = subprocess.run([str(harness), str(fin), str(fout)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    what = f"n={n}, {pk_format}, {addr_format}, misalign={mis}, present={present:03b}"
    assert r.returncode == 0 and "eth_lanes ok" in r.stdout, (what, r.returncode, r.stdout[-500:], r.stderr[-4000:])
    got, pos = fout.read_bytes(), 0
    for given, want, name in zip((address, status), _expected(addrs, expect, addr_format), ("address", "status")):
        if not given:
            continue
        seg = got[pos:pos + 64 + len(want)]
        pos += len(seg)
        assert seg[:32] == b"\xAA" * 32 and seg[-32:] == b"\xAA" * 32, f"{name}: bytes outside the array were written ({what})"
        assert seg[32:-32] == want, f"{name} ({what})"
    assert pos == len(got)


def test_public_vectors_through_the_lane_body(harness, tmp_path):
    for fmt, key in (("affine64", "pk"), ("sec1", "pk_sec1")):
        keys = [bytes.fromhex(v[key]) for v in KATS["addresses"]]
        addrs = [bytes.fromhex(v["address"][2:]) for v in KATS["addresses"]]
        assert _expected(addrs, None, "eip55")[0] == "".join(v["address"] for v in KATS["addresses"]).encode()
        for af in ADF:
            _run(harness, tmp_path, keys, addrs, fmt, af, 0, expect=addrs)


def test_every_format_invalid_kind_parity_and_alignment(harness, tmp_path, batches):
    for pf, af, mis in itertools.product(PKF, ADF, range(16)):
        keys, addrs = batches[pf]
        _run(harness, tmp_path, keys, addrs, pf, af, mis)


def test_expect_matching_and_wrong_in_each_byte(harness, tmp_path, batches):
    for pf, af in itertools.product(PKF, ADF):
        keys, addrs = batches[pf]
        good = [a if a is not None else bytes(20) for a in addrs]                    # (an invalid item is status 3 whatever expect holds: here the zero record it writes)
        _run(harness, tmp_path, keys, addrs, pf, af, 3, expect=good)
        wrong = list(good)
        valid = [i for i, a in enumerate(addrs) if a is not None]
        assert len(valid) >= 20
        for byte, i in enumerate(valid[:20]):                                        # item valid[b] is wrong in byte b only, one bit
            wrong[i] = good[i][:byte] + bytes([good[i][byte] ^ (1 << (byte % 8))]) + good[i][byte + 1:]
        _run(harness, tmp_path, keys, addrs, pf, af, 4 * ADF[af], expect=wrong)         # (expect sits one byte behind the others: byte loads here, word loads at misalign 3 above)


def test_null_address_and_null_status(harness, tmp_path, batches):
    for pf, af in itertools.product(PKF, ADF):
        keys, addrs = batches[pf]
        good = [a if a is not None else bytes(20) for a in addrs]
        _run(harness, tmp_path, keys, addrs, pf, af, 7, expect=good, address=False)
        _run(harness, tmp_path, keys, addrs, pf, af, 15, expect=None, status=False)
        _run(harness, tmp_path, keys, addrs, pf, af, 0, expect=good, status=False)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 7, 16, 17])
def test_batch_sizes_that_end_inside_a_quad(harness, tmp_path, batches, n):
    for pf, af, mis in itertools.product(PKF, ADF, (0, 4, 9)):
        keys, addrs = batches[pf]
        _run(harness, tmp_path, keys[3:3 + n], addrs[3:3 + n], pf, af, mis)
