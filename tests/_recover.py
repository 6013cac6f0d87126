"""The definition of plume_recover_batch (include/plume_hip.h), restated for the tests: item by item from the oracles, never from the library.
    validity   c, s in [1, n-1]; pk and nullifier with coordinates below p, on the curve or the all-zero identity            -> else status 3, zero records
    points     R = s G + (n - c) pk,  Hr = s H + (n - c) nullifier,  H = hash_to_curve(msg, pk)        (C oracle's point_mul, Python oracle's pt_add)
    status     the oracle's verify(version, msg, pk, nullifier, c, s, R, Hr): V2 ignores the two points it is handed and hashes its own -- the same ones
recover_item states it with the Python oracle alone (slow: a quarter of a second per item); recover_batch is the same definition over arrays with the C oracle's
hash_to_curve and verify, for the batches the GPU tests compare against.  tests/test_recover_lanes.py holds the two against each other, against the reference's
vector and against the golden sign records before anything else trusts them."""
import numpy as np

from oracle import plume_oracle as O
from tests import _oracle_c as OC

MISMATCH, MATCH, INVALID = 0, 1, 3
FMT_AFFINE64, FMT_SEC1, FMT_REGISTERS = 0, 1, 2
G_BYTES = O.pt_bytes(O.G)


def valid_point(rec: bytes) -> bool:
    """a 64-byte record the reference's types can hold: the all-zero identity, or coordinates below p on the curve"""
    if rec == bytes(64):
        return True
    x, y = int.from_bytes(rec[:32], "big"), int.from_bytes(rec[32:], "big")
    return x < O.P and y < O.P and O.is_on_curve((x, y))


def valid_item(pk: bytes, nul: bytes, c: bytes, s: bytes) -> bool:
    ci, si = int.from_bytes(c, "big"), int.from_bytes(s, "big")
    return 1 <= ci < O.N and 1 <= si < O.N and valid_point(pk) and valid_point(nul)


def _mul(k: int, rec: bytes):
    """k * point as an oracle Point (None = identity); k in [1, n-1]"""
    if rec == bytes(64):
        return None
    out = OC.point_mul(k.to_bytes(32, "big"), rec)
    assert out is not None
    return O.pt_from_bytes(out)


def points(pk: bytes, nul: bytes, c: bytes, s: bytes, h: bytes):
    """(R, Hr) as 64-byte records for a valid item"""
    ci, si = int.from_bytes(c, "big"), int.from_bytes(s, "big")
    r = O.pt_add(_mul(si, G_BYTES), _mul(O.N - ci, pk))
    hr = O.pt_add(_mul(si, h), _mul(O.N - ci, nul))
    return O.pt_bytes(r), O.pt_bytes(hr)


def recover_item(version, msg: bytes, pk: bytes, nul: bytes, c: bytes, s: bytes):
    """(r_point, hashed_to_curve_r, hashed_to_curve, status) of one item, 64-byte records; Python oracle only"""
    if not valid_item(pk, nul, c, s):
        return bytes(64), bytes(64), bytes(64), INVALID
    pkp, nulp = O.pt_from_bytes(pk), O.pt_from_bytes(nul)
    h = O.pt_bytes(O.hash_to_curve(msg, pkp))
    r, hr = points(pk, nul, c, s, h)
    ok = O.verify(version, msg, pkp, nulp, int.from_bytes(c, "big"), int.from_bytes(s, "big"), O.pt_from_bytes(r), O.pt_from_bytes(hr))
    return r, hr, h, MATCH if ok else MISMATCH


def recover_batch(version, msgs, off, pk, nul, c, s, nthreads=8):
    """dict(r_point, hashed_to_curve_r, hashed_to_curve: (n, 64) uint8; status: (n,) uint8) -- the definition over arrays"""
    n = len(off) - 1
    pk, nul, c, s = (np.ascontiguousarray(a, dtype=np.uint8) for a in (pk, nul, c, s))
    valid = np.array([valid_item(pk[i].tobytes(), nul[i].tobytes(), c[i].tobytes(), s[i].tobytes()) for i in range(n)], dtype=bool)
    pk_h = pk.copy()
    pk_h[~valid] = 0                                                   # (an invalid pk is never hashed)
    h = OC.hash_to_curve_batch(msgs, off, pk_h, nthreads=nthreads)
    out = dict(r_point=np.zeros((n, 64), np.uint8), hashed_to_curve_r=np.zeros((n, 64), np.uint8), hashed_to_curve=np.zeros((n, 64), np.uint8),
               status=np.full(n, INVALID, np.uint8))
    for i in np.flatnonzero(valid):
        r, hr = points(pk[i].tobytes(), nul[i].tobytes(), c[i].tobytes(), s[i].tobytes(), h[i].tobytes())
        out["r_point"][i] = np.frombuffer(r, np.uint8)
        out["hashed_to_curve_r"][i] = np.frombuffer(hr, np.uint8)
        out["hashed_to_curve"][i] = h[i]
    ok = OC.verify_batch(version, msgs, off, pk, nul, c, s, out["r_point"], out["hashed_to_curve_r"], nthreads=nthreads)
    out["status"][valid] = ok[valid]
    assert not ok[~valid].any()
    return out


def sec1_of(rec64):
    """(n, 64) records -> (n, 33): 02|03 || x, the identity 00 + 32 zero bytes"""
    rec64 = np.ascontiguousarray(rec64, dtype=np.uint8).reshape(-1, 64)
    out = np.zeros((len(rec64), 33), np.uint8)
    nz = rec64.any(axis=1)
    out[nz, 0] = 2 + (rec64[nz, 63] & 1)
    out[nz, 1:] = rec64[nz, :32]
    return out


def registers_of(rec64):
    """(n, 64) records -> (n, 64) bytes of uint64[2][4]: x then y as four little-endian 64-bit registers (circuits/circom/utils.ts pointToCircuitValue): each
    32-byte coordinate byte-reversed"""
    rec64 = np.ascontiguousarray(rec64, dtype=np.uint8).reshape(-1, 64)
    return np.concatenate([rec64[:, 31::-1], rec64[:, :31:-1]], axis=1)


def as_format(rec64, fmt):
    return rec64 if fmt == FMT_AFFINE64 else sec1_of(rec64) if fmt == FMT_SEC1 else registers_of(rec64)
