"""The lane bodies of plume_pbkdf2_sha512_batch (zk-nullifier-sig_amd/csrc/plume_kdf.h, plume_sha512.h) on the host: tests/kdf/kdf_lanes.cpp, a stand-alone program
built by its Makefile with g++ under AddressSanitizer + UBSan and -Werror, against the restatement of tests/_kdf.py (hashlib.pbkdf2_hmac), bit for bit and item for item.
Password lengths: one item for every length 0 .. 260 -- 111 / 112, 128 / 129 (the last raw key, the first hashed one), 239 / 240 (two and three blocks of key hashing).
Salt lengths: every length 0 .. 256 with and without PLUME_KDF_BIP39 -- the inner message crosses one, two and three blocks at 107 / 108, 235 / 236 and at 99 / 100, 227 /
228.  Iteration counts 1, 2, 3, 257 (one slice and one round) and 2048; dklen 1, 31, 32, 63, 64; per-item and shared salts; refused items among good ones.  Every array
sits off its alignment, the outputs between guard bytes, the password buffer and the salt in allocations that end with their last byte."""
import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import _kdf as D

ROOT = Path(__file__).resolve().parent.parent
G = b"\xAA" * 32


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("no g++ / make")
    out = tmp_path_factory.mktemp("kdf_lanes")
    subprocess.run(["make", "-C", str(ROOT / "tests" / "kdf"), f"OUT={out}"], check=True, capture_output=True, text=True, timeout=900)
    return out / "kdf_lanes"


def _case(buf, off, salt, salt_len, iterations, dklen, flags, mis, order, pw_bytes=None):
    """(the case's bytes for the program, what the restatement says of it)"""
    n = len(off) - 1
    pw_bytes = len(buf) if pw_bytes is None else pw_bytes
    blob = struct.pack("<7IQ", n, flags, salt_len, iterations, dklen, mis, order, pw_bytes) + np.asarray(off, np.uint64).tobytes() + bytes(buf[:pw_bytes]) + salt.tobytes()
    return blob, D.pbkdf2_batch(buf, off, pw_bytes, salt, salt_len, iterations, dklen, flags)


def _run(harness, tmp_path, cases):
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<I", len(cases)) + b"".join(c[0] for c in cases))
    r = subprocess.run([str(harness), str(fin), str(fout)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "kdf_lanes ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    got, pos = fout.read_bytes(), 0
    for k, (_, (out, status)) in enumerate(cases):
        for want in (out, status):
            length = want.size
            assert got[pos:pos + 32] == G and got[pos + 32 + length:pos + 64 + length] == G, k
            have = np.frombuffer(got[pos + 32:pos + 32 + length], np.uint8).reshape(want.shape)
            bad = np.flatnonzero((have != want).reshape(len(want), -1).any(axis=1))
            assert bad.size == 0, (k, bad[:8])
            pos += 64 + length
    assert pos == len(got)


def _salt(rng, rows, salt_len):
    return rng.integers(0, 256, (rows, salt_len), dtype=np.uint8)


def test_every_password_length_from_0_to_260(harness, tmp_path):
    rng = np.random.default_rng(261)
    lens = np.arange(261, dtype=np.uint64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    buf = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    cases = [_case(buf, off, _salt(rng, 261, 8), 8, 3, 64, 0, 1, 0),
             _case(buf, off, _salt(rng, 1, 8), 8, 2, 64, D.SHARED_SALT | D.BIP39, 7, 1)]
    _run(harness, tmp_path, cases)


@pytest.mark.parametrize("flags", [0, D.BIP39, D.SHARED_SALT, D.BIP39 | D.SHARED_SALT])
def test_every_salt_length_from_0_to_256(harness, tmp_path, flags):
    rng = np.random.default_rng(257 + flags)
    buf, off = D.planted_passwords(3, 11, lengths=(12, 129, 0))
    cases = [_case(buf, off, _salt(rng, 1 if flags & D.SHARED_SALT else 3, sl), sl, 2, 64, flags, sl, sl & 1) for sl in range(257)]
    _run(harness, tmp_path, cases)


def test_iteration_counts_and_output_lengths(harness, tmp_path):
    rng = np.random.default_rng(2048)
    buf, off = D.planted_passwords(len(D.PLANTED), 12)
    cases = []
    for iterations in (1, 2, 3, 257, 2048):
        cases.append(_case(buf, off, _salt(rng, 1, 10), 10, iterations, 64, D.BIP39 | D.SHARED_SALT, iterations, iterations & 1))
    for dklen in (1, 31, 32, 63, 64):
        cases.append(_case(buf, off, _salt(rng, len(D.PLANTED), 5), 5, 3, dklen, 0, dklen, dklen & 1))
    _run(harness, tmp_path, cases)


def test_the_known_answers(harness, tmp_path):
    import json
    cases = []
    for k in json.loads((ROOT / "tests" / "golden" / "kdf_kats.json").read_text())["kats"]:
        pw, salt = np.frombuffer(k["password"].encode(), np.uint8), np.frombuffer(k["salt"].encode(), np.uint8).reshape(1, -1)
        blob, (out, status) = _case(pw, np.array([0, len(pw)], np.uint64), salt, salt.shape[1], k["iterations"], 64, D.SHARED_SALT | (D.BIP39 if k["bip39"] else 0), 3, 0)
        assert out[0].tobytes().hex() == k["out"] and status[0] == 0
        cases.append((blob, (out, status)))
    _run(harness, tmp_path, cases)


def test_refused_items_read_nothing_and_come_out_zero(harness, tmp_path):
    rng = np.random.default_rng(128)
    buf, off = D.planted_passwords(12, 13, lengths=(5, 130, 64))
    off = off.copy()
    off[4] = off[3] - 2                                     # item 3 runs backwards (and item 4 is longer for it)
    off[9] = len(buf) + 1                                   # item 8 reaches past the buffer; item 9 then runs backwards
    off[12] = 2**63                                         # the last one far past it
    blob, (out, status) = _case(buf, off, _salt(rng, 12, 16), 16, 3, 33, D.BIP39, 2, 0)
    assert list(np.flatnonzero(status)) == [3, 8, 9, 11] and (status[[3, 8, 9, 11]] == D.BAD_INPUT).all() and not out[[3, 8, 9, 11]].any() and out[4].any()
    _run(harness, tmp_path, [(blob, (out, status))])
    # a buffer that is shorter than the offsets say: the items beyond pw_bytes are refused, the buffer ends where pw_bytes says
    buf, off = D.planted_passwords(6, 14, lengths=(40, 140))
    cut = int(off[4]) + 7
    blob, (out, status) = _case(buf, off, _salt(rng, 1, 0), 0, 2, 64, D.SHARED_SALT, 0, 1, pw_bytes=cut)
    assert list(status) == [0, 0, 0, 0, D.BAD_INPUT, D.BAD_INPUT]
    _run(harness, tmp_path, [(blob, (out, status))])
