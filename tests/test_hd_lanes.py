"""The lane bodies of the key derivation (zk-nullifier-sig_amd/csrc/plume_hd.h, plume_sha512.h) on the host: tests/hd/hd_lanes.cpp, a stand-alone program built by its Makefile
with g++ under AddressSanitizer + UBSan and -Werror, against hashlib / hmac and the restatement of tests/_hd.py.  SHA-512 and HMAC-SHA-512 for every data length the
one-block shape takes and both key lengths in use; master nodes for every seed length 16 .. 64 (the padding position moves), the seeds in an allocation that ends with their
last byte; whole private and public derivations at every level of the comb, every record format, both SHARED flags, invalid parents planted among good ones, with every
caller array off its alignment and between guard bytes; the tweak functions with CHOSEN IL, which no HMAC will ever give: n - 1, n, n + 1, 2^256 - 1, n - k_par, and the IL
with IL G = -K_par."""
import hashlib
import hmac
import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import _ecdsa as E
from tests import _hd as H
from tests import _keccak as K

ROOT = Path(__file__).resolve().parent.parent
G = b"\xAA" * 32
N = H.N


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("no g++ / make")
    out = tmp_path_factory.mktemp("hd_lanes")
    subprocess.run(["make", "-C", str(ROOT / "tests" / "hd"), f"OUT={out}"], check=True, capture_output=True, text=True, timeout=900)
    return out / "hd_lanes"


def _exec(harness, mode, tmp_path, blob):
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(blob)
    r = subprocess.run([str(harness), mode, str(fin), str(fout)], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "hd_lanes ok" in r.stdout, (mode, r.returncode, r.stdout[-500:], r.stderr[-4000:])
    return fout.read_bytes()


def _guarded(buf, pos, length):
    """the array of `length` bytes that starts behind the 32 guard bytes at pos; returns (array, position behind its trailing guard)"""
    assert buf[pos:pos + 32] == G and buf[pos + 32 + length:pos + 64 + length] == G
    return np.frombuffer(buf[pos + 32:pos + 32 + length], np.uint8), pos + 64 + length


def test_sha512_and_hmac_for_every_length_of_the_one_block_shape(harness, tmp_path):
    rng = np.random.default_rng(512)
    recs, want = [], []
    for length in list(range(0, 112)):
        data = rng.integers(0, 256, length, dtype=np.uint8).tobytes()
        recs.append((0, b"", data)); want.append(hashlib.sha512(data).digest())
    for klen in (12, 32):
        for length in range(16, 65):                                         # every seed length
            key, data = rng.integers(0, 256, klen, dtype=np.uint8).tobytes(), rng.integers(0, 256, length, dtype=np.uint8).tobytes()
            recs.append((1, key, data)); want.append(hmac.new(key, data, hashlib.sha512).digest())
    recs.append((1, b"Bitcoin seed", H.V1_SEED)); want.append(hmac.new(b"Bitcoin seed", H.V1_SEED, hashlib.sha512).digest())
    for first in (0, 2, 3, 0xFF):
        key = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
        data = bytes([first]) + rng.integers(0, 256, 36, dtype=np.uint8).tobytes()
        recs.append((2, key, data)); want.append(hmac.new(key, data, hashlib.sha512).digest())
    blob = struct.pack("<I", len(recs)) + b"".join(struct.pack("<3I", kind, len(key), len(data)) + key.ljust(32, b"\0") + data for kind, key, data in recs)
    got = _exec(harness, "sha512", tmp_path, blob)
    assert len(got) == 64 * len(recs)
    for i, w in enumerate(want):
        assert got[64 * i:64 * i + 64] == w, (i, recs[i][0], len(recs[i][1]), len(recs[i][2]))


@pytest.mark.parametrize("seed_len", [16, 17, 31, 32, 33, 47, 48, 55, 56, 63, 64])
def test_master_nodes(harness, tmp_path, seed_len):
    rng = np.random.default_rng(seed_len)
    n = 5
    seeds = rng.integers(0, 256, (n, seed_len), dtype=np.uint8)
    if seed_len == 16:
        seeds[2] = np.frombuffer(H.V1_SEED, np.uint8)
    if seed_len == 64:
        seeds[2] = np.frombuffer(bytes.fromhex(H.HARDHAT_SEED), np.uint8)
    buf = _exec(harness, "master", tmp_path, struct.pack("<3I", n, seed_len, seed_len % 7) + seeds.tobytes())
    sk, pos = _guarded(buf, 0, 32 * n)
    chain, pos = _guarded(buf, pos, 32 * n)
    status, pos = _guarded(buf, pos, n)
    assert pos == len(buf)
    w_sk, w_chain, w_status = H.master_batch(seeds, seed_len)
    assert np.array_equal(sk.reshape(n, 32), w_sk) and np.array_equal(chain.reshape(n, 32), w_chain) and np.array_equal(status, w_status)
    if seed_len == 16:
        assert sk.reshape(n, 32)[2].tobytes().hex() == H.V1["m"][0] and chain.reshape(n, 32)[2].tobytes().hex() == H.V1["m"][1]


def _derive(harness, tmp_path, pub, parent, chain, path, depth, flags, pk_format, addr_format, uniform, mis, present, order):
    n = len(path) if not flags & H.SHARED_PATH else (len(parent) if not flags & H.SHARED_PARENT else 3)
    blob = struct.pack("<10I", int(pub), n, flags, K.PK_WIDTH[pk_format] == 33, list(K.ADDR_WIDTH).index(addr_format), depth, uniform, mis, present, order)
    blob += np.ascontiguousarray(parent, np.uint8).tobytes() + np.ascontiguousarray(chain, np.uint8).tobytes() + np.ascontiguousarray(path, np.uint32).tobytes()
    buf = _exec(harness, "derive", tmp_path, blob)
    pos, out = 0, {}
    for name, width, there in (("sk", 32, not pub), ("chain", 32, present & 1), ("pk", K.PK_WIDTH[pk_format], present & 2), ("address", K.ADDR_WIDTH[addr_format], present & 4),
                               ("status", 1, True)):
        if there:
            arr, pos = _guarded(buf, pos, width * n)
            out[name] = arr.reshape(n, width) if width > 1 else arr
    assert pos == len(buf)
    return out


def _check(got, want, names):
    for name, w in zip(names, want):
        if name in got:
            assert np.array_equal(got[name], w), (name, np.flatnonzero((got[name] != w).reshape(len(w), -1).any(axis=1))[:8])


BAD_SK = (0, N, 2**256 - 1)


@pytest.mark.parametrize("depth,uniform,pk_format,addr_format,flags", [
    (1, 0, "affine64", "raw20", 0), (5, 1, "sec1", "eip55", 0), (8, 2, "affine64", "record64", 0), (2, 0, "sec1", "record64", H.SHARED_PARENT),
    (3, 1, "affine64", "eip55", H.SHARED_PATH), (2, 2, "sec1", "raw20", H.SHARED_PARENT | H.SHARED_PATH)])
def test_private_derivation(harness, tmp_path, depth, uniform, pk_format, addr_format, flags):
    n = 3 if flags == 3 else 21
    sk, chain = H.seeded_nodes(1 if flags & H.SHARED_PARENT else n, 100 + depth)
    if not flags & H.SHARED_PARENT:
        for j, v in enumerate(BAD_SK):                                       # invalid parents among good ones
            sk[4 + 5 * j] = np.frombuffer(H.b32(v), np.uint8)
    path = H.seeded_paths(1 if flags & H.SHARED_PATH else n, depth, 200 + depth)
    want = H.derive_priv_batch(sk, chain, path, depth, flags, pk_format, addr_format, n=n)
    if not flags & H.SHARED_PARENT:
        assert [int(want[4][4 + 5 * j]) for j in range(3)] == [H.BAD_SCALAR] * 3 and not want[0][4].any() and not want[2][9].any() and not want[3][14].any()
    for present, order in ((7, 0), (0, 1), (5, 1)) if depth == 1 else ((7, depth & 1),):
        got = _derive(harness, tmp_path, False, sk, chain, path, depth, flags, pk_format, addr_format, uniform, depth + 1, present, order)
        _check(got, want, ("sk", "chain", "pk", "address", "status"))


@pytest.mark.parametrize("depth,pk_format,addr_format,flags", [(1, "affine64", "raw20", 0), (5, "sec1", "eip55", 0), (8, "sec1", "record64", H.SHARED_PARENT),
                                                              (2, "affine64", "eip55", H.SHARED_PATH | H.SHARED_PARENT)])
def test_public_derivation(harness, tmp_path, depth, pk_format, addr_format, flags):
    n = 3 if flags == 3 else 21
    sk, chain = H.seeded_nodes(1 if flags & H.SHARED_PARENT else n, 300 + depth)
    pk = H.pk_of(sk, pk_format)
    path = H.seeded_paths(1 if flags & H.SHARED_PATH else n, depth, 400 + depth) & np.uint32(0x7FFFFFFF)
    if not flags & H.SHARED_PATH:
        path[7, depth - 1] = 2**31 + 5                                        # a hardened index in the public form
        path[8, 0] = 2**32 - 1
    if not flags & H.SHARED_PARENT:
        bad = K.invalid_keys(pk_format)
        for j, (_, rec) in enumerate(bad[:6]):
            pk[1 + 3 * j] = np.frombuffer(bytes(rec), np.uint8)
    want = H.derive_pub_batch(pk, chain, path, depth, flags, pk_format, addr_format, n=n)
    if flags == 0:
        assert want[3][8] == H.HARDENED_PUB and want[3][1] == H.BAD_SCALAR and not want[0][1].any() and not want[2][8].any()   # (item 7 is an invalid key too: the key decides)
    got = _derive(harness, tmp_path, True, pk, chain, path, depth, flags, pk_format, addr_format, 0, depth, 7, depth & 1)
    _check(got, want, ("pk", "chain", "address", "status"))
    if depth == 1:
        got = _derive(harness, tmp_path, True, pk, chain, path, depth, flags, pk_format, addr_format, 0, 3, 2, 0)
        _check(got, want, ("pk", "chain", "address", "status"))


def test_public_and_private_agree_and_known_answers(harness, tmp_path):
    seed = H.hardhat_seed()
    m = H.master(seed)
    path = np.array([H.parse_path(H.HARDHAT_ACCOUNT_PATH + f"/{i}") for i in range(3)], np.uint32)
    got = _derive(harness, tmp_path, False, np.frombuffer(H.b32(m[0]), np.uint8), np.frombuffer(m[1], np.uint8), path, 5, H.SHARED_PARENT, "affine64", "raw20", 1, 0, 7, 0)
    assert [r.tobytes().hex() for r in got["sk"]] == [c[0] for c in H.HARDHAT_CHILDREN]
    assert [r.tobytes().hex() for r in got["address"]] == [c[1] for c in H.HARDHAT_CHILDREN]
    acct = H.derive(m[0], m[1], H.HARDHAT_ACCOUNT_PATH)
    pub = _derive(harness, tmp_path, True, H.pk_of(np.frombuffer(H.b32(acct[0]), np.uint8)), np.frombuffer(acct[1], np.uint8), np.arange(3, dtype=np.uint32).reshape(3, 1), 1,
                  H.SHARED_PARENT, "affine64", "raw20", 0, 0, 7, 0)
    assert np.array_equal(pub["address"], got["address"]) and np.array_equal(pub["pk"], got["pk"]) and np.array_equal(pub["chain"], got["chain"])
    # BIP-32 vector 1
    m1 = H.master(H.V1_SEED)
    v1 = _derive(harness, tmp_path, False, np.frombuffer(H.b32(m1[0]), np.uint8), np.frombuffer(m1[1], np.uint8), np.array([[H.H, 1]], np.uint32), 2, 0, "sec1", "raw20", 0, 1, 7, 0)
    assert v1["sk"][0].tobytes().hex() == H.V1["m/0'/1"][0] and v1["chain"][0].tobytes().hex() == H.V1["m/0'/1"][1]


def test_the_tweaks_with_chosen_IL(harness, tmp_path):
    rng = np.random.default_rng(32)
    k_par = [int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "big") % (N - 1) + 1 for _ in range(3)] + [1, N - 1]
    cases = []
    for kp in k_par:
        cases += [(N - 1, kp), (N, kp), (N + 1, kp), (2**256 - 1, kp), (N - kp, kp), (0, kp), (1, kp), (N - kp - 1, kp), ((N - kp + 1) % N, kp)]
    got = _exec(harness, "privtweak", tmp_path, struct.pack("<I", len(cases)) + b"".join(H.b32(il) + H.b32(kp) for il, kp in cases))
    for i, (il, kp) in enumerate(cases):
        child, st = int.from_bytes(got[36 * i:36 * i + 32], "big"), struct.unpack_from("<I", got, 36 * i + 32)[0]
        want = H.priv_tweak(il, kp)
        assert (child, st) == ((want, 0) if want is not None else (0, H.NO_KEY)), (hex(il), hex(kp))
    for il, kp in ((N, k_par[0]), (N + 1, k_par[0]), (2**256 - 1, k_par[0]), (N - k_par[0], k_par[0])):
        assert H.priv_tweak(il, kp) is None
    assert H.priv_tweak(N - 1, k_par[0]) == k_par[0] - 1
    # the public form: IL G = -K_par gives the identity
    pcases = []
    for kp in k_par[:3]:
        Kp = H.g_mul(kp)
        pcases += [(N - 1, Kp), (N, Kp), (N + 1, Kp), (2**256 - 1, Kp), (N - kp, Kp), (1, Kp), (kp, Kp), (N - kp - 1, Kp)]       # (kp, Kp): the doubling
    got = _exec(harness, "pubtweak", tmp_path, struct.pack("<I", len(pcases)) + b"".join(H.b32(il) + E.pk_record(Kp, "affine64") for il, Kp in pcases))
    for i, (il, Kp) in enumerate(pcases):
        rec, st = got[68 * i:68 * i + 64], struct.unpack_from("<I", got, 68 * i + 64)[0]
        want = H.pub_tweak(il, Kp)
        assert (rec, st) == ((E.pk_record(want, "affine64"), 0) if want is not None else (bytes(64), H.NO_KEY)), (hex(il), i)
    assert H.pub_tweak(N - k_par[0], H.g_mul(k_par[0])) is None
