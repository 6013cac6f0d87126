"""The lane bodies of plume_ecdsa_recover_batch (zk-nullifier-sig_amd/csrc/plume_ecdsa.h) on the host: tests/ecdsa/ecdsa_lanes.cpp compiled with g++ under
AddressSanitizer + UBSan and -Werror, against Python's pow(x, -1, n) and the restatement of tests/_ecdsa.py (itself pinned to OpenSSL by
tests/test_ecdsa_restatement.py).  sc_inv on its edge values and a few hundred seeded ones; fe_inv unchanged on the same kind of vectors; prepare, tables, multiply (the
unchecked chain, then the checked redo of what it filed), conversion and finalize lane by lane on the OpenSSL vectors and on every crafted item, both key formats x the
three address formats, expect absent / matching / wrong, each output NULL in turn, arrays at odd offsets with the bytes around them untouched."""
import itertools
import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import _ecdsa as E
from tests import _keccak as K

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "zk-nullifier-sig_amd" / "csrc"
PKF = {"affine64": 0, "sec1": 1}
ADF = {"raw20": 0, "record64": 1, "eip55": 2}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("ecdsa_lanes") / "ecdsa_lanes"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-DPLUME_COMB_W=10",
                    f"-I{CSRC}", str(ROOT / "tests" / "ecdsa" / "ecdsa_lanes.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True, timeout=900)
    return exe


def _exec(harness, mode, tmp_path, blob):
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(blob)
    r = subprocess.run([str(harness), mode, str(fin), str(fout)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "ecdsa_lanes ok" in r.stdout, (mode, r.returncode, r.stdout[-500:], r.stderr[-4000:])
    return fout.read_bytes()


def _values(mod, seed):
    rng = np.random.default_rng(seed)
    edge = [1, 2, mod - 1, mod - 2, (mod + 1) // 2, 2**255, E.LAMBDA, 3, 2**128, 2**128 - 1, 2**30, 2**30 - 1, 2**240]
    return edge + [int.from_bytes(rng.bytes(32), "big") % (mod - 1) + 1 for _ in range(300)]


def test_sc_inv_against_pow(harness, tmp_path):
    xs = _values(E.N, 31)
    got = _exec(harness, "scinv", tmp_path, struct.pack("<I", len(xs)) + b"".join(E.b32(x) for x in xs))
    assert got == b"".join(E.b32(pow(x, -1, E.N)) for x in xs)


def test_fe_inv_is_unchanged_on_its_own_vectors(harness, tmp_path):
    xs = _values(E.P, 32)
    got = _exec(harness, "feinv", tmp_path, struct.pack("<I", len(xs)) + b"".join(E.b32(x) for x in xs))
    assert got == b"".join(E.b32(pow(x, -1, E.P)) for x in xs)


@pytest.fixture(scope="module")
def items():
    """the OpenSSL vectors, then every crafted item (its own flags dropped: a batch has one flags word), as lists of (hash, r, s, v)"""
    kats = E.load_kats()
    rows = [(bytes.fromhex(e["hash"]), bytes.fromhex(e["r"]), bytes.fromhex(e["s"]), e["v"]) for e in kats["openssl"] + kats["crafted"]]
    return rows, len(kats["openssl"])


def _recover(harness, tmp_path, rows, pk_format, addr_format, mis=0, flags=0, expect=None, pk=True, address=True, status=True):
    n = len(rows)
    present = (1 if pk else 0) | (2 if address else 0) | (4 if status else 0) | (8 if expect is not None else 0)
    H, R, S = (b"".join(row[k] for row in rows) for k in range(3))
    V = bytes(row[3] for row in rows)
    blob = struct.pack("<6I", n, flags, PKF[pk_format], ADF[addr_format], mis, present) + H + R + S + V + (expect.tobytes() if expect is not None else b"")
    got = _exec(harness, "recover", tmp_path, blob)
    wpk, wad, wst = E.recover_batch(H, R, S, V, expect, pk_format, addr_format, flags)
    what = f"n={n}, {pk_format}, {addr_format}, misalign={mis}, flags={flags}, present={present:04b}"
    filed, pos = struct.unpack("<I", got[:4])[0], 4
    for given, want, name in zip((pk, address, status), (wpk.tobytes(), wad.tobytes(), wst.tobytes()), ("pk", "address", "status")):
        if not given:
            continue
        seg = got[pos:pos + 64 + len(want)]
        pos += len(seg)
        assert seg[:32] == b"\xAA" * 32 and seg[-32:] == b"\xAA" * 32, f"{name}: bytes outside the array were written ({what})"
        assert seg[32:-32] == want, f"{name} ({what})"
    assert pos == len(got)
    return filed, wst


def test_openssl_vectors_recover_openssl_keys(harness, tmp_path, items):
    rows, nk = items
    want = [e["pk"] for e in E.load_kats()["openssl"]]
    filed, st = _recover(harness, tmp_path, rows[:nk], "affine64", "raw20")
    assert list(st) == [E.MATCH] * nk and filed == 0
    H, R, S = (b"".join(row[k] for row in rows[:nk]) for k in range(3))
    assert E.recover_batch(H, R, S, bytes(row[3] for row in rows[:nk]))[0].tobytes().hex() == "".join(want)


def test_every_format_pair_on_the_vectors_and_the_crafted_items(harness, tmp_path, items):
    rows, nk = items
    for (pf, af), flags in zip(itertools.product(PKF, ADF), (0, 1, 0, 1, 1, 0)):
        filed, st = _recover(harness, tmp_path, rows, pf, af, mis=0, flags=flags)
        # every identity construction (five of them) ends in p == -q at the last addition of the unchecked chain: the checked redo ran, and gave the identity.  (The
        # doubling constructions need not file: the comb's terms join the accumulator one by one, so u1 G never stands alone beside u2 R.)
        assert filed >= 5 and set(st) == {E.MATCH, E.INVALID}


def test_expect_right_wrong_and_on_invalid_items(harness, tmp_path, items):
    rows, _ = items
    H, R, S = (b"".join(row[k] for row in rows) for k in range(3))
    _, addr, st0 = E.recover_batch(H, R, S, bytes(row[3] for row in rows))
    good = addr.copy()
    _, st = _recover(harness, tmp_path, rows, "affine64", "record64", mis=5, expect=good)
    assert (st == st0).all()
    wrong = good.copy()
    wrong[np.arange(len(rows)), np.arange(len(rows)) % 20] ^= (1 << (np.arange(len(rows)) % 8)).astype(np.uint8)      # one flipped bit per item, invalid items included
    _, st = _recover(harness, tmp_path, rows, "sec1", "eip55", mis=0, expect=wrong)
    assert ((st == E.MISMATCH) == (st0 == E.MATCH)).all() and ((st == E.INVALID) == (st0 == E.INVALID)).all()


def test_each_output_null_in_turn_and_odd_offsets(harness, tmp_path, items):
    rows, nk = items
    some = rows[nk - 6:nk + 30]
    for (pf, af), mis in zip(itertools.product(PKF, ADF), (1, 3, 7, 9, 13, 15)):
        _recover(harness, tmp_path, some, pf, af, mis=mis, pk=False)
        _recover(harness, tmp_path, some, pf, af, mis=mis, address=False)
        _recover(harness, tmp_path, some, pf, af, mis=mis, status=False)
        _recover(harness, tmp_path, some, pf, af, mis=mis, pk=False, address=False)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 7, 8, 9, 17])
def test_batch_sizes_around_the_shared_inversions(harness, tmp_path, items, n):
    rows, nk = items
    _recover(harness, tmp_path, rows[nk - 3:nk - 3 + n], "sec1", "raw20", mis=2)
