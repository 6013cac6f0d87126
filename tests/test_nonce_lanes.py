"""The derived-nonce lane body (zk-nullifier-sig_amd/csrc/plume_nonce.h) on the host against the RFC 6979 oracle (tests/_rfc6979.py): tests/nonce/nonce_lanes.cpp
compiled with g++ under AddressSanitizer + UBSan and -Werror.  The published vectors through the generic core rfc6979_k; the PLUME h1 and nonce for ragged message lengths
around SHA-256's block edges, both versions, both modes, with and without the hedging input; secret keys taken as given (0, 1, n-1, n, 2^256-1); rejected message
offsets (the empty span, msgs never read); and step h's retry under q = 2^255 + 19, where about half of all candidates are rejected, with a cap of 4 candidates."""
import hashlib
import os
import random
import shutil
import subprocess
from pathlib import Path

import pytest

from tests import _rfc6979 as R

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "zk-nullifier-sig_amd" / "csrc"
P256_Q = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
P256_X = "C9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721"
LENS = [0, 1, 33, 34, 55, 56, 63, 64, 65, 119, 120, 300, 1000]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("nonce_lanes") / "nonce_lanes"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}",
                    str(ROOT / "tests" / "nonce" / "nonce_lanes.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True, timeout=600)
    return exe


def _run(harness, tmp_path, lines, seed=1):
    f = tmp_path / "cases.txt"
    f.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(harness), str(f), str(seed)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    out = r.stdout.splitlines()
    assert out[-1].startswith("nonce_lanes ok")
    return out[:-1]


def _k(cap, q, x, h1, aux=None):
    return f"K {cap} {q:064x} {x} {h1.hex()} {aux.hex() if aux else '-'}"


def test_published_vectors_through_the_core(harness, tmp_path):
    lines = [_k(16, P256_Q, P256_X, hashlib.sha256(b"sample").digest()), _k(16, P256_Q, P256_X, hashlib.sha256(b"test").digest()),
             _k(16, R.N, "00" * 31 + "01", hashlib.sha256(b"Satoshi Nakamoto").digest())]
    assert _run(harness, tmp_path, lines) == ["a6e3c57dd01abe90086538398355dd4c3b17aa873382b0f24d6129493d8aad60 1",
                                              "d16b6ae827f17175e040871a1c7ec3500192c4c92677336ec2537acaee0008e0 1",
                                              "8f8a276c19f4149656b280621e358cce24f5f52542772691ee69063b74f15d15 1"]


def _batch(version, msgs_list, sks, auxs=None, pks=None, off=None, msgs_bytes=None):
    buf = b"".join(msgs_list)
    if off is None:
        off = [0]
        for m in msgs_list:
            off.append(off[-1] + len(m))
    n = len(off) - 1
    lines = [f"B {version} {n} {int(auxs is not None)} {int(pks is not None)} {len(buf)} {buf.hex() or '-'}", " ".join(map(str, off))]
    for i in range(n):
        lines.append(f"{sks[i].hex()} {auxs[i].hex() if auxs else '-'} {pks[i].hex() if pks else '-'}")
    return lines


@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("hedged", [False, True])
def test_plume_h1_and_nonce_match_the_oracle(harness, tmp_path, version, mode, hedged):
    rng = random.Random(version * 4 + mode * 2 + hedged)
    msgs = [bytes(rng.randrange(256) for _ in range(L)) for L in LENS]
    sks = [rng.randrange(1, R.N).to_bytes(32, "big") for _ in LENS]
    auxs = [rng.randbytes(32) for _ in LENS] if hedged else None
    pks = [rng.randbytes(64) for _ in LENS] if mode else None
    out = _run(harness, tmp_path, _batch(version, msgs, sks, auxs, pks), seed=rng.randrange(1 << 30))
    for i, line in enumerate(out):
        h1, r, used = line.split()
        pk = pks[i] if pks else None
        assert h1 == R.plume_h1(version, msgs[i], pk).hex(), (LENS[i], "h1")
        assert r == R.plume_nonce(version, sks[i], msgs[i], pk, auxs[i] if auxs else None).hex(), (LENS[i], "r")
        assert used == "1"


def test_secret_keys_are_taken_as_given(harness, tmp_path):
    sks = [v.to_bytes(32, "big") for v in (0, 1, R.N - 1, R.N, (1 << 256) - 1)]
    msgs = [b"same message"] * len(sks)
    for aux in (None, [b"\x33" * 32] * len(sks)):
        out = _run(harness, tmp_path, _batch(1, msgs, sks, aux))
        rs = [line.split()[1] for line in out]
        assert rs == [R.plume_nonce(1, sk, msgs[0], None, aux[0] if aux else None).hex() for sk in sks]
        assert len(set(rs)) == len(sks)


def test_rejected_offsets_hash_the_empty_span_without_reading_msgs(harness, tmp_path):
    """decreasing offsets and offsets past msgs_bytes: the lane hashes the empty span; msgs is exactly sized, so ASan would see a read"""
    msgs = [b"abcdefgh", b"ijklmnop"]
    sks = [(5).to_bytes(32, "big")] * 4
    off = [0, 8, 4, 1 << 40, 16]
    out = _run(harness, tmp_path, _batch(2, msgs, sks, off=off))
    want = [b"abcdefgh", b"", b"", b""]
    for line, m in zip(out, want):
        h1, r, _ = line.split()
        assert h1 == R.plume_h1(2, m).hex() and r == R.plume_nonce(2, sks[0], m).hex()


def test_retry_path_and_the_cap(harness, tmp_path):
    """q = 2^255 + 19: candidates at or above q are rejected (about half).  With a cap of 4 candidates the lane must flag exactly the items the oracle says need more"""
    q = (1 << 255) + 19
    rng = random.Random(6979)
    lines, want = [], []
    for i in range(400):
        x = rng.randbytes(32)
        h1 = rng.randbytes(32)
        aux = rng.randbytes(32) if i & 1 else None
        need = R.rounds_needed(q, x, h1, aux, limit=4)
        lines.append(_k(4, q, x.hex(), h1, aux))
        if need <= 4:
            k = next(k for k in R.candidates(q, x, h1, aux) if 1 <= k < q)
            want.append((f"{k:064x}", str(need)))
        else:
            want.append(("00" * 32, "0"))
    got = [tuple(line.split()) for line in _run(harness, tmp_path, lines)]
    assert got == want
    used = [int(u) for _, u in want]
    assert used.count(1) and used.count(2) and used.count(3) and used.count(4) and used.count(0)
