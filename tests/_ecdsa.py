"""A restatement of ECDSA over secp256k1 -- signing with a given nonce, and public-key recovery as plume_ecdsa_recover_batch (include/plume_hip.h) defines it: Ethereum's
ecrecover with a one-byte v that may also be 0 or 1 -- in plain Python, shared by the ECDSA tests.  Nothing here is taken from the library's code: the group law is the
textbook Jacobian one on Python integers, scalars are multiplied bit by bit (no endomorphism, no tables, no digits), the inverse mod n is pow(x, -1, n).  Addresses come
from tests/_keccak.py.  tests/golden/ecdsa_recover_kats.json pins it to OpenSSL: keys and signatures it did not make (tests/golden/make_ecdsa_recover_kats.py)."""
import functools
import json
from pathlib import Path

import numpy as np

from tests import _keccak as K

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
GX = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
GY = 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72      # lambda (x, y) = (beta x, y): only the crafted cases use it, as a scalar
HALF_N = (N - 1) // 2
MISMATCH, MATCH, INVALID = K.MISMATCH, K.MATCH, K.INVALID
LOW_S = 1
KATS = Path(__file__).resolve().parent / "golden" / "ecdsa_recover_kats.json"


# ------------------------------------------------------------------------------------------------ the group: Jacobian (X, Y, Z), None = identity
def _dbl(a):
    if a is None:
        return None
    x, y, z = a
    s = 4 * x * y * y % P
    m = 3 * x * x % P
    x3 = (m * m - 2 * s) % P
    return (x3, (m * (s - x3) - 8 * y**4) % P, 2 * y * z % P)


def _add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    x1, y1, z1 = a
    x2, y2, z2 = b
    u1, u2 = x1 * z2 * z2 % P, x2 * z1 * z1 % P
    s1, s2 = y1 * z2**3 % P, y2 * z1**3 % P
    if u1 == u2:
        return _dbl(a) if s1 == s2 else None
    h, r = (u2 - u1) % P, (s2 - s1) % P
    x3 = (r * r - h**3 - 2 * u1 * h * h) % P
    return (x3, (r * (u1 * h * h - x3) - s1 * h**3) % P, h * z1 * z2 % P)


def _affine(a):
    if a is None:
        return None
    zi = pow(a[2], -1, P)
    return (a[0] * zi * zi % P, a[1] * zi**3 % P)


def mul2(k1, p1, k2, p2):
    """k1 p1 + k2 p2 for affine points (or None), affine result (or None): one bit of each scalar per doubling"""
    j1 = None if p1 is None else (p1[0], p1[1], 1)
    j2 = None if p2 is None else (p2[0], p2[1], 1)
    j12 = _add(j1, j2)
    acc = None
    for bit in range(max(k1.bit_length(), k2.bit_length()) - 1, -1, -1):
        acc = _dbl(acc)
        sel = ((k1 >> bit) & 1) | (((k2 >> bit) & 1) << 1)
        if sel:
            acc = _add(acc, (j1, j2, j12)[sel - 1])
    return _affine(acc)


def mul(k, pt=(GX, GY)):
    return mul2(k % N, pt, 0, None)


def lift_x(x, parity):
    """the curve point with this x (an integer below p) and y of this parity, or None"""
    rhs = (x**3 + 7) % P
    y = pow(rhs, (P + 1) // 4, P)
    if y * y % P != rhs:
        return None
    return (x, y if (y & 1) == parity else P - y)


# ------------------------------------------------------------------------------------------------ ECDSA
def sign(sk, z, k):
    """(r, s, v) over the digest integer z with the nonce k; v in {0, 1}: the parity of R's y.  None when r or s comes out 0 or R's x is at least n (the recovery rule has
    no candidate x = r + n)"""
    R = mul(k)
    if R is None or R[0] >= N or R[0] == 0:
        return None
    r = R[0]
    s = pow(k, -1, N) * (z + r * sk) % N
    return None if s == 0 else (r, s, R[1] & 1)


def recover(hash32, r, s, v, flags=0):
    """the recovered public key (x, y), or None for an invalid item.  r, s: integers below 2^256; v: one byte; hash32: 32 bytes"""
    if v in (0, 1):
        parity = v
    elif v in (27, 28):
        parity = v - 27
    else:
        return None
    if not (1 <= r < N and 1 <= s < N):
        return None
    if (flags & LOW_S) and s > HALF_N:
        return None
    R = lift_x(r, parity)
    if R is None:
        return None
    z = int.from_bytes(hash32, "big") % N
    ri = pow(r, -1, N)
    return mul2(-z * ri % N, (GX, GY), s * ri % N, R)


def pk_record(pt, pk_format):
    return pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big") if pk_format == "affine64" else bytes([2 + (pt[1] & 1)]) + pt[0].to_bytes(32, "big")


def recover_batch(hash, r, s, v, expect=None, pk_format="affine64", addr_format="raw20", flags=0):
    """(pk uint8[n, P], address uint8[n, W], status uint8[n]) as include/plume_hip.h defines them"""
    as_bytes = lambda a: np.frombuffer(a, np.uint8) if isinstance(a, (bytes, bytearray)) else np.ascontiguousarray(a, dtype=np.uint8)  # noqa: E731
    hash, r, s, v = as_bytes(hash).reshape(-1, 32), as_bytes(r).reshape(-1, 32), as_bytes(s).reshape(-1, 32), as_bytes(v).reshape(-1)
    n = len(v)
    expect = None if expect is None else as_bytes(expect).reshape(n, 20)
    Pw, W = K.PK_WIDTH[pk_format], K.ADDR_WIDTH[addr_format]
    pk, address, status = np.zeros((n, Pw), np.uint8), np.zeros((n, W), np.uint8), np.full(n, INVALID, np.uint8)
    for i in range(n):
        q = _recover_cached(hash[i].tobytes(), r[i].tobytes(), s[i].tobytes(), int(v[i]), flags)
        if q is None:
            continue
        a = K.address_of(q)
        pk[i] = np.frombuffer(pk_record(q, pk_format), np.uint8)
        address[i] = np.frombuffer(_record_cached(a, addr_format), np.uint8)
        status[i] = MATCH if expect is None or expect[i].tobytes() == a else MISMATCH
    return pk, address, status


@functools.lru_cache(maxsize=None)
def _recover_cached(h, r, s, v, flags):
    return recover(h, int.from_bytes(r, "big"), int.from_bytes(s, "big"), v, flags)


@functools.lru_cache(maxsize=None)
def _record_cached(a, addr_format):
    return K.record_of(a, addr_format)


# ------------------------------------------------------------------------------------------------ inputs the tests share
def b32(x):
    return x.to_bytes(32, "big")


def genuine(n, seed, with_pk=True):
    """n genuine signatures on seeded keys, digests and nonces: (hash, r, s, v) as uint8 arrays, v drawn from both encodings, and the signers' public keys (None each
    when with_pk is false: a scalar multiplication per item saved)"""
    rng = np.random.default_rng(seed)
    H, R, S, V, PK = [], [], [], [], []
    while len(V) < n:
        sk, k = (int.from_bytes(rng.bytes(32), "big") % (N - 1) + 1 for _ in range(2))
        h = rng.bytes(32)
        sig = sign(sk, int.from_bytes(h, "big") % N, k)
        if sig is None:
            continue
        H.append(h); R.append(b32(sig[0])); S.append(b32(sig[1])); V.append(sig[2] + (27 if len(V) % 3 == 0 else 0)); PK.append(mul(sk) if with_pk else None)
    arr = lambda xs: np.frombuffer(b"".join(xs), np.uint8).reshape(n, 32).copy()  # noqa: E731
    return arr(H), arr(R), arr(S), np.array(V, np.uint8), PK


def load_kats():
    """the committed vectors: {"openssl": [{hash, r, s, v, pk}], "crafted": [{name, hash, r, s, v, flags}]}, hex strings"""
    return json.loads(KATS.read_text())


def crafted_cases():
    """every crafted item of the issue as (name, hash32, r, s, v, flags).  k, s0 are arbitrary fixed scalars"""
    k, s0 = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF, 0x0FEDCBA987654321FEDCBA987654321FEDCBA987654321FEDCBA9876543210
    h0 = bytes(range(32))
    out = []
    add = lambda name, h, r, s, v, flags=0: out.append((name, h if isinstance(h, bytes) else b32(h), r, s, v, flags))  # noqa: E731
    for name, r in [("r = 0", 0), ("r = n", N), ("r = n + 1", N + 1), ("r = n - 1", N - 1), ("r = n - 2", N - 2), ("r = 1", 1), ("r = 2", 2), ("r = 3", 3), ("r = 4", 4)]:
        for v in (0, 1):
            add(f"{name}, v = {v}", h0, r, s0, v)
    Rk = mul(k)
    for name, s in [("s = 0", 0), ("s = n", N), ("s = n - 1", N - 1), ("s = 1", 1), ("s = (n - 1) / 2", HALF_N), ("s = (n + 1) / 2", HALF_N + 1)]:
        for flags in (0, LOW_S):
            add(f"{name}, flags = {flags}", h0, Rk[0], s, Rk[1] & 1, flags)
    for v in (2, 3, 26, 29, 255):
        add(f"v = {v}", h0, Rk[0], s0, v)
    for name, h in [("hash = 0", 0), ("hash = n", N), ("hash = n + 1", N + 1), ("hash = 2^256 - 1", 2**256 - 1)]:
        add(name, h, Rk[0], s0, 27 + (Rk[1] & 1))
    add("identity: R = k G, hash = s k", s0 * k % N, Rk[0], s0, Rk[1] & 1)
    add("doubling: R = k G, hash = -s k", -s0 * k % N, Rk[0], s0, Rk[1] & 1)
    # u2 R = G and u1 = 1: the accumulator IS the comb's first term when that term arrives -- a doubling inside the chain of additions; u1 = -1: the identity there
    ki = pow(k, -1, N)
    add("comb doubling: u2 R = G, u1 = 1", -Rk[0] % N, Rk[0], ki * Rk[0] % N, Rk[1] & 1)
    add("comb identity: u2 R = G, u1 = -1", Rk[0] % N, Rk[0], ki * Rk[0] % N, Rk[1] & 1)
    for name, m in [("R = G", 1), ("R = -G", N - 1), ("R = 2G", 2), ("R = 3G", 3)]:
        Rm = mul(m)
        add(name, h0, Rm[0], s0, Rm[1] & 1)
        add(name + ", identity", s0 * m % N, Rm[0], s0, Rm[1] & 1)
        add(name + ", doubling", -s0 * m % N, Rm[0], s0, Rm[1] & 1)
    for name, u2 in [("u2 = 1", 1), ("u2 = n - 1", N - 1), ("u2 = lambda", LAMBDA), ("u2 = lambda + 1", LAMBDA + 1), ("u2 = 2^128", 2**128), ("u2 = 2^128 - 1", 2**128 - 1)]:
        add(name, h0, Rk[0], u2 * Rk[0] % N, 28 - (~Rk[1] & 1))
        add(name + ", hash = 0", 0, Rk[0], u2 * Rk[0] % N, Rk[1] & 1)
    return out
