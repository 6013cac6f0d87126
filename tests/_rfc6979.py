"""Test oracle: RFC 6979 §3.2 deterministic nonces with HMAC-SHA-256 (and §3.6's extra input k'), written from the RFC's text with the standard library
only, generic in the modulus q; plus the PLUME preimage of the derived-nonce signer (include/plume_hip.h, plume_sign_batch_rfc6979):

    h1  = SHA-256("PLUME-RFC6979" || u8 version || u8 mode || pk_in (64 B, mode 1 only) || msg)
    x   = sk, the 32 bytes as given
    r   = rfc6979_k(n, x, h1, aux)

The product package never imports this module."""
import hashlib
import hmac

N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141   # secp256k1 group order
DOMAIN = b"PLUME-RFC6979"
CAP = 16                                                                # candidates per item before the signer gives up (PLUME_NONCE_ROUNDS)


def _hmac(k: bytes, data: bytes) -> bytes:
    return hmac.new(k, data, hashlib.sha256).digest()


def bits2int(b: bytes, qlen: int) -> int:
    v = int.from_bytes(b, "big")
    blen = 8 * len(b)
    return v >> (blen - qlen) if blen > qlen else v


def int2octets(v: int, rlen: int) -> bytes:
    return v.to_bytes(rlen, "big")


def bits2octets(b: bytes, q: int) -> bytes:
    qlen = q.bit_length()
    z1 = bits2int(b, qlen)
    z2 = z1 - q if z1 >= q else z1
    return int2octets(z2, (qlen + 7) // 8)


def candidates(q: int, x: bytes, h1: bytes, aux: bytes = None):
    """RFC 6979 §3.2 steps b-h: every candidate k in order, in range or not.  x is int2octets(x) as given (rlen bytes)."""
    qlen = q.bit_length()
    rlen = (qlen + 7) // 8
    assert len(x) == rlen
    extra = b"" if aux is None else aux
    h = bits2octets(h1, q)
    V = b"\x01" * 32                                                    # b
    K = b"\x00" * 32                                                    # c
    K = _hmac(K, V + b"\x00" + x + h + extra)                          # d
    V = _hmac(K, V)                                                     # e
    K = _hmac(K, V + b"\x01" + x + h + extra)                          # f
    V = _hmac(K, V)                                                     # g
    while True:                                                         # h
        T = b""
        while len(T) * 8 < qlen:
            V = _hmac(K, V)
            T += V
        yield bits2int(T, qlen)
        K = _hmac(K, V + b"\x00")
        V = _hmac(K, V)


def rfc6979_k(q: int, x: bytes, h1: bytes, aux: bytes = None):
    """(k, candidates used): the first candidate in [1, q-1]"""
    for used, k in enumerate(candidates(q, x, h1, aux), start=1):
        if 1 <= k < q:
            return k, used


def rounds_needed(q: int, x: bytes, h1: bytes, aux: bytes = None, limit: int = 64) -> int:
    """candidates until one is in range, or limit + 1 when none of the first `limit` is"""
    for used, k in enumerate(candidates(q, x, h1, aux), start=1):
        if 1 <= k < q:
            return used
        if used >= limit:
            return limit + 1


def plume_h1(version: int, msg: bytes, pk_in: bytes = None) -> bytes:
    mode = 0 if pk_in is None else 1
    pre = DOMAIN + bytes([version, mode]) + (b"" if pk_in is None else bytes(pk_in))
    return hashlib.sha256(pre + bytes(msg)).digest()


def plume_nonce(version: int, sk: bytes, msg: bytes, pk_in: bytes = None, aux: bytes = None) -> bytes:
    """the 32-byte nonce plume_sign_batch_rfc6979 signs item i with; all-zero when CAP candidates ran out"""
    h1 = plume_h1(version, msg, pk_in)
    for used, k in enumerate(candidates(N, bytes(sk), h1, None if aux is None else bytes(aux)), start=1):
        if 1 <= k < N:
            return k.to_bytes(32, "big")
        if used >= CAP:
            return bytes(32)


def _flat(a) -> bytes:
    return bytes(a) if isinstance(a, (bytes, bytearray, memoryview)) else a.tobytes()


def plume_nonces(version: int, msgs, off, sk, pk_in=None, aux=None) -> bytes:
    """batch form over the C ABI's arrays (bytes or numpy): n x 32 nonces as one bytes object"""
    n = len(off) - 1
    mb, skb = _flat(msgs), _flat(sk)
    pkb = None if pk_in is None else _flat(pk_in)
    axb = None if aux is None else _flat(aux)
    out = []
    for i in range(n):
        out.append(plume_nonce(version, skb[32 * i:32 * i + 32], mb[int(off[i]):int(off[i + 1])], None if pkb is None else pkb[64 * i:64 * i + 64],
                               None if axb is None else axb[32 * i:32 * i + 32]))
    return b"".join(out)
