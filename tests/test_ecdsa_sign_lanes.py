"""The lane bodies of plume_ecdsa_sign_batch (zk-nullifier-sig_amd/csrc/plume_ecdsa_sign.h) and the ragged Keccak body of plume_eth_message_hash_batch
(csrc/plume_keccak.h) on the host: tests/ecdsa_sign/ecdsa_sign_lanes.cpp built by its Makefile with g++ under AddressSanitizer + UBSan and -Werror, run over the whole
fixture (tests/golden/ecdsa_sign_kats.json) against the restatement of tests/_ecdsa_sign.py: nonces, r, s, v and status at the three uniform levels, plain and hedged, both
v encodings, arrays at odd offsets with the bytes around them untouched; the digests of both modes with the messages at every start residue mod 8 in an allocation of
exactly their size; the r-from-x step on synthetic x around n (the one branch no real input reaches); the release body's verdicts on staged records whose recovered key
differs."""
import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import _ecdsa as E
from tests import _ecdsa_sign as S

ROOT = Path(__file__).resolve().parent.parent
G = b"\xAA" * 32


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("no g++ / make")
    out = tmp_path_factory.mktemp("ecdsa_sign_lanes")
    subprocess.run(["make", "-C", str(ROOT / "tests" / "ecdsa_sign"), f"OUT={out}"], check=True, capture_output=True, text=True, timeout=900)
    return out / "ecdsa_sign_lanes"


def _exec(harness, mode, tmp_path, blob):
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(blob)
    r = subprocess.run([str(harness), mode, str(fin), str(fout)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "ecdsa_sign_lanes ok" in r.stdout, (mode, r.returncode, r.stdout[-500:], r.stderr[-4000:])
    return fout.read_bytes()


def _guarded(got, pos, want, name, what):
    seg = got[pos:pos + 64 + len(want)]
    assert seg[:32] == G and seg[-32:] == G, f"{name}: bytes outside the array were written ({what})"
    assert seg[32:-32] == want, f"{name} ({what})"
    return pos + len(seg)


@pytest.fixture(scope="module")
def kats():
    return S.load_kats()


def _sign(harness, tmp_path, rows, aux, flags, uniform, mis, staged=False):
    """rows: [(sk32, hash32)]; aux: None or 32 bytes for every item"""
    n = len(rows)
    H, SK = b"".join(h for _, h in rows), b"".join(sk for sk, _ in rows)
    AUX = None if aux is None else aux * n
    got = _exec(harness, "sign", tmp_path, struct.pack("<6I", n, flags, uniform, mis, 0 if aux is None else 1, 1 if staged else 0) + H + SK + (AUX or b""))
    r, s, v, st = S.sign_batch(H, SK, AUX, flags)
    what = f"n={n}, flags={flags}, uniform={uniform}, misalign={mis}, aux={'yes' if aux else 'no'}"
    used = struct.unpack(f"<{n}I", got[:4 * n])
    pos = 4 * n
    for i, (sk, h) in enumerate(rows):
        k = S.nonce(sk, h, aux) if st[i] != S.BAD_SCALAR else None
        assert got[pos + 32 * i:pos + 32 * i + 32] == (E.b32(k) if k else bytes(32)), (what, i)
        if k:
            assert used[i] == 1                                              # (a second candidate has probability 2^-128)
    pos += 32 * n
    for want, name in ((r, "r"), (s, "s"), (v, "v"), (st, "status")):
        pos = _guarded(got, pos, want.tobytes(), name, what)
    if staged:
        pk = b"".join(E.pk_record(E.mul(int.from_bytes(sk, "big")), "affine64") if st[i] == S.OK else bytes(64) for i, (sk, _) in enumerate(rows))
        pos = _guarded(got, pos, pk, "sk G", what)
    assert pos == len(got)
    return st


@pytest.mark.parametrize("uniform", [0, 1, 2])
def test_the_whole_fixture_at_every_uniform_level(harness, tmp_path, kats, uniform):
    for aux in (None, S.FIXED_AUX):
        rows = [(bytes.fromhex(e["sk"]), bytes.fromhex(e["hash"])) for e in kats["sign"] if (e["aux"] is None) == (aux is None)]
        st = _sign(harness, tmp_path, rows, aux, S.V27 if uniform == 1 else 0, uniform, mis=uniform)
        want = [e["status"] for e in kats["sign"] if (e["aux"] is None) == (aux is None)]
        assert list(st) == want and S.BAD_SCALAR in want and want.count(S.OK) >= 25


def test_the_published_vectors_and_odd_offsets(harness, tmp_path, kats):
    rows = [(bytes.fromhex(p["sk"]), bytes.fromhex(p["hash"])) for p in kats["public"]]
    for mis in (0, 1, 5, 8, 15):
        _sign(harness, tmp_path, rows, None, 0, 1, mis)
    _sign(harness, tmp_path, rows[:1], None, S.V27, 0, 3)
    _sign(harness, tmp_path, [], None, 0, 1, 0)


def test_the_staged_key_of_the_selfcheck(harness, tmp_path, kats):
    rows = [(bytes.fromhex(e["sk"]), bytes.fromhex(e["hash"])) for e in kats["sign"][30:52]]          # seeded items and the sk edges
    for uniform in (0, 1, 2):
        _sign(harness, tmp_path, rows, None, S.V27, uniform, mis=2, staged=True)


def test_r_from_x_on_both_sides_of_n(harness, tmp_path):
    """x >= n has a recovery id the one-byte v does not represent: status 4.  No real input reaches that branch (probability 2^-128), so the step is fed directly"""
    xs = [E.N - 1, E.N, E.N + 1, E.P - 1, 1, 0, E.N - 2, 2**255]
    got = _exec(harness, "rfromx", tmp_path, struct.pack("<I", len(xs)) + b"".join(E.b32(x) for x in xs))
    for i, x in enumerate(xs):
        r, st = int.from_bytes(got[36 * i:36 * i + 32], "big"), struct.unpack("<I", got[36 * i + 32:36 * i + 36])[0]
        assert r == x % E.N, hex(x)
        assert st == (S.IDENTITY if x >= E.N or x == 0 else 0), hex(x)


def _hash(harness, tmp_path, msgs, mode, mis_msgs, mis_out, off=None, nbytes=None):
    buf = b"".join(msgs)
    if off is None:
        off = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint64)
    nbytes = len(buf) if nbytes is None else nbytes
    n = len(off) - 1
    got = _exec(harness, "hash", tmp_path, struct.pack("<4IQ", n, mode, mis_msgs, mis_out, nbytes) + np.asarray(off, np.uint64).tobytes() + buf[:nbytes])
    return got


def test_message_digests_at_every_start_residue(harness, tmp_path, kats):
    for mode in (S.KECCAK256, S.EIP191):
        msgs = [bytes.fromhex(e["msg"]) for e in kats["hash"] if e["mode"] == mode]
        want = b"".join(bytes.fromhex(e["digest"]) for e in kats["hash"] if e["mode"] == mode)
        starts = set()
        for mis in range(8):
            got = _hash(harness, tmp_path, msgs, mode, mis, (3 * mis + 1) % 16)
            assert _guarded(got, 0, want, "digest", f"mode={mode}, misalign={mis}") == len(got)
            starts |= {(mis + sum(len(m) for m in msgs[:i])) % 8 for i in range(len(msgs)) if len(msgs[i]) >= 16}
        assert starts == set(range(8))                                       # every long message began at every residue
        # the other mode over the same bytes: the two preimages differ
        other = b"".join(S.message_hash(m, 1 - mode) for m in msgs)
        got = _hash(harness, tmp_path, msgs, 1 - mode, 1, 0)
        assert _guarded(got, 0, other, "digest", f"mode={1 - mode}") == len(got) and other != want


def test_rejected_offsets_hash_the_empty_message(harness, tmp_path):
    msgs = [S.message_of(L, L) for L in (5, 300, 0, 40)]
    off = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint64)
    for mode in (S.KECCAK256, S.EIP191):
        empty = S.message_hash(b"", mode)
        bad = off.copy()
        bad[2] = 3                                                           # item 1 runs backwards, item 2 gets a start before its neighbour's: [5, 3) and [3, 305)
        got = _hash(harness, tmp_path, msgs, mode, 3, 0, off=bad)
        buf = b"".join(msgs)
        want = S.message_hash(msgs[0], mode) + empty + S.message_hash(buf[3:305], mode) + S.message_hash(msgs[3], mode)
        assert _guarded(got, 0, want, "digest", "decreasing offsets") == len(got)
        got = _hash(harness, tmp_path, msgs, mode, 0, 0, nbytes=200)         # the buffer ends inside item 1: items 1, 2, 3 reach past it and never read it
        want = S.message_hash(msgs[0], mode) + empty * 3
        assert _guarded(got, 0, want, "digest", "offsets past the buffer") == len(got)
    got = _hash(harness, tmp_path, [], S.EIP191, 0, 0)
    assert got == G + G


def test_release_verdicts(harness, tmp_path, kats):
    """the failing verdict of the self-check, which no honest run produces: staged records whose recovered key differs come out all zero with status 8; an item with a
    status of its own is released as staged whatever was recovered; a matching key releases the staged bytes"""
    es = [e for e in kats["sign"] if e["aux"] is None][28:44]                # seeded items, then sk = 0 (status 2), 1, 2, n - 1, n and n + 1 (status 2) ...
    n = len(es)
    r = b"".join(bytes.fromhex(e["r"]) for e in es)
    s = b"".join(bytes.fromhex(e["s"]) for e in es)
    v = bytes(e["v"] + 27 if e["status"] == S.OK else 0 for e in es)
    st = bytes(e["status"] for e in es)
    pk = [E.pk_record(E.mul(int(e["sk"], 16)), "affine64") if e["status"] == S.OK else bytes(64) for e in es]
    rec, recst, want_ok = [], [], []
    for i, e in enumerate(es):
        kind = i % 4                                                         # 0: the right key; 1: one bit of it flipped; 2: nothing recovered; 3: another item's key
        key = pk[i] if kind == 0 else bytes([pk[i][0] ^ 1]) + pk[i][1:] if kind == 1 else bytes(64) if kind == 2 else pk[(i + 1) % 8]
        rec.append(key)
        recst.append(3 if kind == 2 or e["status"] != S.OK else 1)
        want_ok.append(e["status"] != S.OK or kind == 0)
    assert S.BAD_SCALAR in st and want_ok.count(False) >= 6 and any(ok and e["status"] == S.OK for ok, e in zip(want_ok, es))
    for mis in (0, 7):
        got = _exec(harness, "release", tmp_path, struct.pack("<2I", n, mis) + r + s + v + st + b"".join(pk) + b"".join(rec) + bytes(recst))
        z32 = bytes(32)
        pos = _guarded(got, 0, b"".join(r[32 * i:32 * i + 32] if ok else z32 for i, ok in enumerate(want_ok)), "r", mis)
        pos = _guarded(got, pos, b"".join(s[32 * i:32 * i + 32] if ok else z32 for i, ok in enumerate(want_ok)), "s", mis)
        pos = _guarded(got, pos, bytes(v[i] if ok else 0 for i, ok in enumerate(want_ok)), "v", mis)
        pos = _guarded(got, pos, bytes(st[i] if ok else S.SELFCHECK_FAILED for i, ok in enumerate(want_ok)), "status", mis)
        assert pos == len(got)
