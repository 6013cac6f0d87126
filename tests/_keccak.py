"""A restatement of the Keccak sponge and of plume_eth_address_batch (include/plume_hip.h) in plain Python, shared by the Ethereum-address tests.  Nothing here is taken
from the library's code: the round constants come from the LFSR of FIPS 202 §3.2.5, the rotation offsets from the (t + 1)(t + 2) / 2 rule of §3.2.2, the state is a
5 x 5 list of integers.  The domain byte is a parameter: 0x06 gives SHA3-256, which hashlib can check; 0x01 gives Keccak-256, what Ethereum uses."""
import numpy as np

from oracle import plume_oracle as O

MASK = (1 << 64) - 1
MISMATCH, MATCH, INVALID = 0, 1, 3
PK_WIDTH = {"affine64": 64, "sec1": 33}
ADDR_WIDTH = {"raw20": 20, "record64": 64, "eip55": 42}


def _rc_bit(t):
    r = 1
    for _ in range(t % 255):
        r <<= 1
        if r & 0x100:
            r ^= 0x171
    return r & 1


RC = [sum(_rc_bit(7 * i + j) << ((1 << j) - 1) for j in range(7)) for i in range(24)]


def _rho_offsets():
    r = [[0] * 5 for _ in range(5)]
    x, y = 1, 0
    for t in range(24):
        r[x][y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    return r


RHO = _rho_offsets()


def _rotl(v, n):
    return ((v << n) | (v >> (64 - n))) & MASK if n else v


def keccak_f(a):
    """a[x][y], 24 rounds, in place"""
    for rc in RC:
        c = [a[x][0] ^ a[x][1] ^ a[x][2] ^ a[x][3] ^ a[x][4] for x in range(5)]
        d = [c[(x - 1) % 5] ^ _rotl(c[(x + 1) % 5], 1) for x in range(5)]
        a = [[a[x][y] ^ d[x] for y in range(5)] for x in range(5)]
        b = [[0] * 5 for _ in range(5)]
        for x in range(5):
            for y in range(5):
                b[y][(2 * x + 3 * y) % 5] = _rotl(a[x][y], RHO[x][y])
        a = [[b[x][y] ^ (~b[(x + 1) % 5][y] & MASK & b[(x + 2) % 5][y]) for y in range(5)] for x in range(5)]
        a[0][0] ^= rc
    return a


def sponge256(msg, domain):
    """256-bit output, rate 136 bytes, pad = domain byte ... 0x80"""
    rate = 136
    m = bytearray(msg) + bytes([domain]) + bytes(-(len(msg) + 1) % rate)
    m[-1] |= 0x80
    a = [[0] * 5 for _ in range(5)]
    for blk in range(0, len(m), rate):
        for k in range(rate // 8):
            a[k % 5][k // 5] ^= int.from_bytes(m[blk + 8 * k:blk + 8 * k + 8], "little")
        a = keccak_f(a)
    return b"".join(a[k % 5][k // 5].to_bytes(8, "little") for k in range(4))


def keccak256(msg):
    return sponge256(msg, 0x01)


def eip55(addr20):
    """'0x' + 40 hex digits, digit i upper-cased iff nibble i of Keccak-256(the 40 lower-case digits) is at least 8"""
    low = bytes(addr20).hex()
    h = keccak256(low.encode()).hex()
    return "0x" + "".join(ch.upper() if int(h[i], 16) >= 8 else ch for i, ch in enumerate(low))


def decode_pk(rec, pk_format="affine64"):
    """the affine point of a key record, or None when the record is no Ethereum key: a coordinate >= p, off the curve, the identity, a bad SEC1 prefix, an x with no root"""
    rec = bytes(rec)
    if pk_format == "sec1":
        x = int.from_bytes(rec[1:33], "big")
        if rec[0] not in (2, 3) or x >= O.P:
            return None
        rhs = (x * x * x + 7) % O.P
        y = pow(rhs, (O.P + 1) // 4, O.P)
        if y * y % O.P != rhs:
            return None
        return (x, y if (y & 1) == (rec[0] & 1) else O.P - y)
    x, y = int.from_bytes(rec[:32], "big"), int.from_bytes(rec[32:], "big")
    if (x == 0 and y == 0) or x >= O.P or y >= O.P or (y * y - x * x * x - 7) % O.P:
        return None
    return (x, y)


def address_of(pt):
    return keccak256(pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big"))[12:]


def record_of(addr20, addr_format):
    return {"raw20": addr20, "record64": bytes(44) + addr20, "eip55": eip55(addr20).encode()}[addr_format]


def eth_address_batch(pk, expect=None, pk_format="affine64", addr_format="raw20"):
    """(address uint8[n, W], status uint8[n]) as include/plume_hip.h defines them"""
    P, W = PK_WIDTH[pk_format], ADDR_WIDTH[addr_format]
    as_bytes = lambda a: np.frombuffer(a, np.uint8) if isinstance(a, (bytes, bytearray)) else np.ascontiguousarray(a, dtype=np.uint8)  # noqa: E731
    pk = as_bytes(pk).reshape(-1, P)
    n = len(pk)
    expect = None if expect is None else as_bytes(expect).reshape(n, 20)
    address, status = np.zeros((n, W), np.uint8), np.zeros(n, np.uint8)
    for i in range(n):
        pt = decode_pk(pk[i].tobytes(), pk_format)
        if pt is None:
            status[i] = INVALID
            continue
        a = address_of(pt)
        address[i] = np.frombuffer(record_of(a, addr_format), np.uint8)
        status[i] = MATCH if expect is None or expect[i].tobytes() == a else MISMATCH
    return address, status


# ------------------------------------------------------------------------------------------------ inputs the tests share
def sample_keys(n, seed, pk_format="affine64"):
    """n valid keys (multiples of G by the C oracle), odd and even y mixed, as uint8[n, P]"""
    from tests import _oracle_c as OC
    rng = np.random.default_rng(seed)
    g = O.pt_bytes((O.GX, O.GY))
    recs = []
    for _ in range(n):
        k = (int.from_bytes(rng.bytes(32), "big") % (O.N - 1) + 1).to_bytes(32, "big")
        rec = OC.point_mul(k, g)
        recs.append(rec if pk_format == "affine64" else bytes([2 + (rec[63] & 1)]) + rec[:32])
    return np.frombuffer(b"".join(recs), np.uint8).reshape(n, PK_WIDTH[pk_format]).copy()


def _small_x(with_root):
    for x in range(1, 1000):
        rhs = (x ** 3 + 7) % O.P
        y = pow(rhs, (O.P + 1) // 4, O.P)
        if (y * y % O.P == rhs) == with_root:
            return x, y
    raise AssertionError


def invalid_keys(pk_format):
    """every kind of record that is no Ethereum key, as (name, bytes)"""
    b32 = lambda v: v.to_bytes(32, "big")  # noqa: E731
    xs, ys = _small_x(True)                        # a point with a tiny x: x + p still fits 32 bytes and is the same residue
    xn, _ = _small_x(False)
    if pk_format == "sec1":
        return [("prefix 00, zeros", bytes(33)), ("prefix 00, x of G", b"\x00" + b32(O.GX)), ("prefix 04", b"\x04" + b32(O.GX)), ("prefix 05", b"\x05" + b32(O.GX)),
                ("x >= p", bytes([2 + (ys & 1)]) + b32(xs + O.P)), ("x with no root", b"\x02" + b32(xn)), ("x with no root, 03", b"\x03" + b32(xn))]
    return [("the zero record", bytes(64)), ("off the curve", b32(O.GX) + b32(O.GY ^ 1)), ("x >= p", b32(xs + O.P) + b32(ys)), ("x = p", b32(O.P) + b32(O.GY)),
            ("y >= p", b32(O.GX) + b32(2 ** 256 - 1)), ("y = p, x = 0", bytes(32) + b32(O.P)), ("x with no root", b32(xn) + b32(O.GY))]
