"""A restatement of plume_ecdsa_sign_batch and plume_eth_message_hash_batch (include/plume_hip.h) in plain Python, shared by the ECDSA signing tests: deterministic ECDSA
over secp256k1 with RFC 6979 nonces over the digest itself, always low s, a one-byte recovery id, the library's status rules; and the digest a wallet signs (Keccak-256,
plain or behind the EIP-191 prefix).  Built on tests/_rfc6979.candidates (h1 = hash), tests/_ecdsa.sign and tests/_keccak.keccak256; nothing here is taken from the
library's code.  tests/golden/ecdsa_sign_kats.json pins it to the published RFC 6979 / secp256k1 vectors and to OpenSSL's verifier (tests/golden/make_ecdsa_sign_kats.py)."""
import functools
import json
from pathlib import Path

import numpy as np

from tests import _ecdsa as E
from tests import _keccak as K
from tests import _rfc6979 as R

N, HALF_N = E.N, E.HALF_N
OK, BAD_SCALAR, IDENTITY, SELFCHECK_FAILED = 0, 2, 4, 8          # PLUME_STATUS_* (include/plume_hip.h)
V27 = 1                                                          # PLUME_ECDSA_SIGN_V27
KECCAK256, EIP191 = 0, 1                                         # PLUME_ETH_HASH_*
EIP191_PREFIX = b"\x19Ethereum Signed Message:\n"
KATS = Path(__file__).resolve().parent / "golden" / "ecdsa_sign_kats.json"
b32 = E.b32


# ------------------------------------------------------------------------------------------------ the digest
def eip191_preimage(msg: bytes) -> bytes:
    return EIP191_PREFIX + str(len(msg)).encode("ascii") + bytes(msg)


def message_hash(msg: bytes, mode: int = EIP191) -> bytes:
    if mode not in (KECCAK256, EIP191):
        raise ValueError("mode")
    return K.keccak256(eip191_preimage(msg) if mode == EIP191 else bytes(msg))


def message_hash_batch(msgs, off, mode):
    mb = bytes(msgs) if isinstance(msgs, (bytes, bytearray)) else np.ascontiguousarray(msgs, dtype=np.uint8).tobytes()
    out = b"".join(_hash_cached(mb[int(off[i]):int(off[i + 1])], mode) for i in range(len(off) - 1))
    return np.frombuffer(out, np.uint8).reshape(-1, 32).copy()


@functools.lru_cache(maxsize=None)
def _hash_cached(msg, mode):
    return message_hash(msg, mode)


# ------------------------------------------------------------------------------------------------ the signature
def nonce(sk32: bytes, hash32: bytes, aux: bytes = None):
    """RFC 6979 section 3.2 with q = n, x = sk as given, h1 = hash (aux: section 3.6's k'): the first of the first R.CAP candidates in [1, n - 1], or None"""
    for used, k in enumerate(R.candidates(N, bytes(sk32), bytes(hash32), None if aux is None else bytes(aux)), start=1):
        if 1 <= k < N:
            return k
        if used >= R.CAP:
            return None


@functools.lru_cache(maxsize=None)
def _g_windows():
    """[w][d] = d 256^w G in Jacobian coordinates, d = 1 .. 255, w = 0 .. 31: the table of the batch form's k G (32 additions instead of tests/_ecdsa.mul's 256 doublings)"""
    rows, base = [], (E.GX, E.GY, 1)
    for _ in range(32):
        row, acc = [None], None
        for _ in range(255):
            acc = E._add(acc, base)
            row.append(acc)
        rows.append(row)
        base = E._add(acc, base)
    return rows


def sign_given_nonce_fast(sk: int, z: int, k: int):
    """tests/_ecdsa.sign(sk, z, k) with k G from the window table: what sign_batch uses for thousands of items.  tests/test_ecdsa_sign_oracle.py holds the two together"""
    acc = None
    for w, row in enumerate(_g_windows()):
        d = (k >> (8 * w)) & 0xFF
        if d:
            acc = E._add(acc, row[d])
    Rp = E._affine(acc)
    if Rp is None or Rp[0] >= N or Rp[0] == 0:
        return None
    s = pow(k, -1, N) * (z + Rp[0] * sk) % N
    return None if s == 0 else (Rp[0], s, Rp[1] & 1)


def sign_raw(sk32: bytes, hash32: bytes, aux: bytes = None, fast: bool = False):
    """the signature BEFORE the low-s rule: (status, r, s, parity, k); r = s = parity = 0 unless status is OK"""
    sk = int.from_bytes(sk32, "big")
    if not 1 <= sk < N:
        return BAD_SCALAR, 0, 0, 0, None
    k = nonce(sk32, hash32, aux)
    if k is None:
        return BAD_SCALAR, 0, 0, 0, None
    sig = (sign_given_nonce_fast if fast else E.sign)(sk, int.from_bytes(hash32, "big") % N, k)           # None: r = 0, s = 0 or R.x >= n
    if sig is None:
        return IDENTITY, 0, 0, 0, k
    return OK, sig[0], sig[1], sig[2], k


def sign(sk32: bytes, hash32: bytes, aux: bytes = None, flags: int = 0, fast: bool = False):
    """(r, s, v, status) as plume_ecdsa_sign_batch writes them: integers r, s; v 0 / 1, or 27 / 28 under V27; all zero unless status is OK"""
    if flags & ~V27:
        raise ValueError("flags")
    st, r, s, parity, _ = sign_raw(sk32, hash32, aux, fast)
    if st != OK:
        return 0, 0, 0, st
    if s > HALF_N:
        s, parity = N - s, parity ^ 1
    return r, s, parity + (27 if flags & V27 else 0), OK


def sign_batch(hash, sk, aux=None, flags=0):
    """(r uint8[n, 32], s uint8[n, 32], v uint8[n], status uint8[n])"""
    as_bytes = lambda a: a if isinstance(a, (bytes, bytearray)) else np.ascontiguousarray(a, dtype=np.uint8).tobytes()  # noqa: E731
    hb, sb = as_bytes(hash), as_bytes(sk)
    ab = None if aux is None else as_bytes(aux)
    n = len(sb) // 32
    r, s, v, st = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    for i in range(n):
        ri, si, vi, sti = _sign_cached(sb[32 * i:32 * i + 32], hb[32 * i:32 * i + 32], None if ab is None else ab[32 * i:32 * i + 32])
        r[i], s[i] = np.frombuffer(b32(ri), np.uint8), np.frombuffer(b32(si), np.uint8)
        v[i], st[i] = (vi + (27 if flags & V27 else 0)) if sti == OK else 0, sti
    return r, s, v, st


@functools.lru_cache(maxsize=None)
def _sign_cached(sk32, hash32, aux):
    return sign(sk32, hash32, aux, 0, fast=True)


def personal_sign(sk32: bytes, msg: bytes, aux: bytes = None) -> bytes:
    r, s, v, st = sign(sk32, message_hash(msg, EIP191), aux, V27)
    if st != OK:
        raise ValueError(f"status {st}")
    return b32(r) + b32(s) + bytes([v])


# ------------------------------------------------------------------------------------------------ inputs the tests share
def seeded(n, seed):
    """n seeded (sk, hash, aux) triples with sk in [1, n - 1]: uint8 arrays n x 32"""
    rng = np.random.default_rng(seed)
    sk = b"".join(b32(int.from_bytes(rng.bytes(32), "big") % (N - 1) + 1) for _ in range(n))
    arr = lambda b: np.frombuffer(b, np.uint8).reshape(n, 32).copy()  # noqa: E731
    return arr(sk), arr(rng.bytes(32 * n)), arr(rng.bytes(32 * n))


SK_EDGES = (0, 1, 2, N - 1, N, N + 1, 2**256 - 1)
HASH_EDGES = (0, 1, N - 1, N, N + 1, 2**256 - 1)
FIXED_AUX = bytes(range(0xA0, 0xC0))
HASH_LENGTHS = {KECCAK256: (0, 1, 7, 8, 9, 135, 136, 137, 271, 272, 273, 1000),
                EIP191: (106, 107, 108, 242, 243, 244, 0, 9, 10, 99, 100, 999, 1000)}      # the rate's edges (26 + digits + L = 135, 136, 137 and 271, 272, 273), then the decimal widths


def message_of(length, salt):
    """a fixed message of `length` bytes"""
    return bytes((37 * j + 11 * salt + (j >> 8)) & 0xFF for j in range(length))


def load_kats():
    """the committed vectors: {"public": [...], "sign": [{name, sk, hash, aux, r, s, v, status, high}], "hash": [{mode, msg, digest}]}, hex strings (aux: hex or null)"""
    return json.loads(KATS.read_text())
