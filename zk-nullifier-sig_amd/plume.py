"""Host façade with the reference's API shape, computing through the MI355X engine (capi.Engine) only.

plume_rustcrypto shape (rust-k256/src/lib.rs:43-156, rust-k256/src/randomizedsigner.rs:25-112):
    DST, AffinePoint, NonZeroScalar, SecretKey, PlumeSignature{message, pk, nullifier, c, s, v1specific},
    PlumeSignatureV1Fields{r_point, hashed_to_curve_r}, PlumeSignature.verify(), PlumeSignature.sign_v1 / sign_v2,
    PlumeSigner(secret_key, v1).try_sign_with_rng(rng, msg) / sign_with_rng(rng, msg)
plume_arkworks shape (rust-arkworks/src/lib.rs:66-69,185-201,229-291):
    PlumeVersion, PlumeSignaturePublic, PlumeSignaturePrivate, sign_with_r(keypair, message, r, version), sign(rng, ...)

Everything cryptographic (hash_to_curve, the scalar multiplications, the c-hash, s = r + sk*c) runs in the HIP
kernels; this module only marshals bytes and reproduces the reference's error behaviour:
  * `expect(..)` panics of the signer (randomizedsigner.rs:61,91,95) -> PlumePanic
  * `signature::Error` (randomizedsigner.rs:59) -> SignatureError (unreachable for this DST, as in the reference)
  * the signer's self-check, when the engine has it on (Engine.set_sign_selfcheck), withholding a signature -> PlumeSelfCheckError
  * NonZeroScalar / on-curve invariants of the Rust types -> ValueError at construction
A single sign/verify is a batch of one; callers with many signatures should use Engine.verify_batch / sign_batch.
"""
from dataclasses import dataclass
from enum import Enum
from typing import Optional, Tuple

import numpy as np

from .capi import (ECDSA_INVALID, ETH_INVALID, ETH_MATCH, ETH_TX_OK, HD_HARDENED, HD_MAX_DEPTH, MERKLE_MATCH, RECOVER_INVALID, RECOVER_MATCH, STATUS_BAD_TX, STATUS_HD_HARDENED,
                   STATUS_HD_NO_KEY, Engine, bip39_bytes, default_engine, pack_messages)

DST = b"QUUX-V01-CS02-with-secp256k1_XMD:SHA-256_SSWU_RO_"  # rust-k256/src/lib.rs:61
_P = 2**256 - 2**32 - 977
_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


class PlumePanic(RuntimeError):
    """the reference signer would `panic!` here (randomizedsigner.rs:61,91,95)"""


class PlumeSelfCheckError(RuntimeError):
    """the signer's self-check (Engine.set_sign_selfcheck(1)) withheld the signature: the signer called it good but its records do not verify
    (status bit 8, PLUME_STATUS_SELFCHECK_FAILED).  Not one of the reference's panics: the reference releases such a signature."""


STATUS_SELFCHECK_FAILED = 8


class SignatureError(Exception):
    """signature::Error (randomizedsigner.rs:59)"""


@dataclass(frozen=True)
class AffinePoint:
    """k256::AffinePoint: on-curve point or the identity (x = y = None)."""
    x: Optional[int] = None
    y: Optional[int] = None

    def __post_init__(self):
        if (self.x is None) != (self.y is None):
            raise ValueError("both coordinates or none")
        if self.x is not None:
            if not (0 <= self.x < _P and 0 <= self.y < _P) or (self.y * self.y - self.x**3 - 7) % _P:
                raise ValueError("point is not on secp256k1")

    @property
    def is_identity(self):
        return self.x is None

    def to_bytes64(self) -> bytes:
        return bytes(64) if self.x is None else self.x.to_bytes(32, "big") + self.y.to_bytes(32, "big")

    @staticmethod
    def from_bytes64(b: bytes) -> "AffinePoint":
        b = bytes(b)
        if b == bytes(64):
            return AffinePoint()
        return AffinePoint(int.from_bytes(b[:32], "big"), int.from_bytes(b[32:], "big"))

    def to_encoded_point(self, compress: bool = True) -> bytes:
        """SEC1 (encode_pt, rust-k256/src/utils.rs:23-25): identity = single 00"""
        if self.x is None:
            return b"\x00"
        if compress:
            return bytes([2 + (self.y & 1)]) + self.x.to_bytes(32, "big")
        return b"\x04" + self.to_bytes64()

    @staticmethod
    def generator() -> "AffinePoint":
        return AffinePoint(0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
                           0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)


@dataclass(frozen=True)
class NonZeroScalar:
    """k256::NonZeroScalar: integer in [1, n-1]"""
    value: int

    def __post_init__(self):
        if not (1 <= self.value < _N):
            raise ValueError("scalar must be in [1, n-1]")

    def to_bytes(self) -> bytes:
        return self.value.to_bytes(32, "big")

    @staticmethod
    def from_repr(b: bytes) -> "NonZeroScalar":
        return NonZeroScalar(int.from_bytes(bytes(b), "big"))


class SecretKey(NonZeroScalar):
    """k256::SecretKey"""

    @staticmethod
    def from_bytes(b: bytes) -> "SecretKey":
        return SecretKey(int.from_bytes(bytes(b), "big"))

    @staticmethod
    def random(rng) -> "SecretKey":
        """SecretKey::random: 32 bytes from rng.fill_bytes, big-endian, rejection-sampled (pinned by the mock RNG of
        rust-k256/tests/signing.rs:23-44)."""
        while True:
            b = rng.fill_bytes(32)
            v = int.from_bytes(b, "big")
            if 1 <= v < _N:
                return SecretKey(v)


@dataclass
class PlumeSignatureV1Fields:  # rust-k256/src/lib.rs:84-89
    r_point: AffinePoint
    hashed_to_curve_r: AffinePoint


@dataclass
class PlumeSignature:  # rust-k256/src/lib.rs:67-80
    message: bytes
    pk: AffinePoint
    nullifier: AffinePoint
    c: NonZeroScalar
    s: NonZeroScalar
    v1specific: Optional[PlumeSignatureV1Fields] = None

    def verify(self, engine: Optional[Engine] = None) -> bool:
        """PlumeSignature::verify (rust-k256/src/lib.rs:93-145) on the GPU."""
        eng = engine or default_engine()
        msgs, off = pack_messages([bytes(self.message)])
        a = lambda b: np.frombuffer(b, dtype=np.uint8)  # noqa: E731
        v1 = self.v1specific
        ok = eng.verify_batch(1 if v1 else 2, msgs, off, a(self.pk.to_bytes64()), a(self.nullifier.to_bytes64()), a(self.c.to_bytes()), a(self.s.to_bytes()),
                              a(v1.r_point.to_bytes64()) if v1 else None, a(v1.hashed_to_curve_r.to_bytes64()) if v1 else None)
        return bool(ok[0])

    def _eth(self, engine, addr_format, expect=None):
        eng = engine or default_engine()
        a = lambda b: np.frombuffer(b, dtype=np.uint8)  # noqa: E731
        return eng.eth_address_batch(a(self.pk.to_bytes64()), None if expect is None else a(bytes(expect)), addr_format=addr_format)

    def eth_address(self, engine: Optional[Engine] = None) -> bytes:
        """The 20-byte Ethereum address of pk, Keccak-256(x || y)[12:], computed on the GPU (include/plume_hip.h, plume_eth_address_batch).  Raises SignatureError when pk
        is no Ethereum key: off the curve, a coordinate not below p, or the identity, which verify() accepts but which has no address."""
        address, status = self._eth(engine, "raw20")
        if int(status[0]) == ETH_INVALID:
            raise SignatureError("eth_address: pk is not a non-identity curve point")
        return address[0].tobytes()

    def eth_address_eip55(self, engine: Optional[Engine] = None) -> str:
        """eth_address() as "0x" + 40 hex digits with the EIP-55 mixed-case checksum"""
        address, status = self._eth(engine, "eip55")
        if int(status[0]) == ETH_INVALID:
            raise SignatureError("eth_address_eip55: pk is not a non-identity curve point")
        return address[0].tobytes().decode("ascii")

    def verify_for_address(self, addr20: bytes, engine: Optional[Engine] = None) -> bool:
        """verify() AND "pk is the key of the 20-byte address addr20": the gate of a consumer that holds addresses (an allow-list, ERC-7524's signing address), not
        public keys.  False for a pk that has no address."""
        if len(bytes(addr20)) != 20:
            raise ValueError("addr20: 20 raw bytes")
        _, status = self._eth(engine, "raw20", expect=addr20)
        return int(status[0]) == ETH_MATCH and self.verify(engine)

    def verify_for_root(self, root32: bytes, proof, amount: Optional[int] = None, engine: Optional[Engine] = None) -> bool:
        """verify() AND "pk's address is on the allow-list whose Merkle root is root32": pk -> address -> leaf -> proof, the sibling of verify_for_address for a consumer
        that holds one 32-byte root (OpenZeppelin's StandardMerkleTree of ["address"], or of ["address", "uint256"] when `amount` is given) and takes a proof from every
        claimant.  proof: the 32-byte siblings, leaf side first.  False for a pk that has no address."""
        eng = engine or default_engine()
        address, status = self._eth(eng, "raw20")
        if int(status[0]) == ETH_INVALID:
            return False
        return merkle_verify(address[0].tobytes(), proof, root32, amount, eng) and self.verify(eng)

    def recover_v1specific(self, engine: Optional[Engine] = None) -> PlumeSignatureV1Fields:
        """The V1-specific fields that pk, nullifier, c, s imply -- r_point = s G - c pk, hashed_to_curve_r = s H - c nullifier, recomputed on the GPU
        (include/plume_hip.h, plume_recover_batch) -- for a c that is the V1 hash of them: upgrades a compact four-field record to a V1 record.  Raises SignatureError
        when an input is no value of the reference's types, and when c is NOT that hash (a V2 signature, a forgery): never a silent pair of points that do not verify."""
        eng = engine or default_engine()
        msgs, off = pack_messages([bytes(self.message)])
        a = lambda b: np.frombuffer(b, dtype=np.uint8)  # noqa: E731
        o = eng.recover_batch(1, msgs, off, a(self.pk.to_bytes64()), a(self.nullifier.to_bytes64()), a(self.c.to_bytes()), a(self.s.to_bytes()),
                              want=("r_point", "hashed_to_curve_r", "status"))
        st = int(o["status"][0])
        if st == RECOVER_INVALID:
            raise SignatureError("recover_v1specific: an input is no value of the reference's types")
        if st != RECOVER_MATCH:
            raise SignatureError("recover_v1specific: c is not the V1 hash of the recovered points")
        return PlumeSignatureV1Fields(AffinePoint.from_bytes64(o["r_point"][0].tobytes()), AffinePoint.from_bytes64(o["hashed_to_curve_r"][0].tobytes()))

    @staticmethod
    def sign_v1(secret_key: SecretKey, msg: bytes, rng, engine: Optional[Engine] = None) -> "PlumeSignature":  # lib.rs:149-151
        return PlumeSigner(secret_key, True, engine).sign_with_rng(rng, msg)

    @staticmethod
    def sign_v2(secret_key: SecretKey, msg: bytes, rng, engine: Optional[Engine] = None) -> "PlumeSignature":  # lib.rs:154-156
        return PlumeSigner(secret_key, False, engine).sign_with_rng(rng, msg)


class PlumeSigner:  # rust-k256/src/randomizedsigner.rs:25-41
    def __init__(self, secret_key: SecretKey, v1: bool, engine: Optional[Engine] = None):
        self.secret_key = secret_key
        self.v1 = bool(v1)
        self._engine = engine

    def try_sign_with_rng(self, rng, msg: bytes) -> PlumeSignature:  # randomizedsigner.rs:43-112
        eng = self._engine or default_engine()
        r = SecretKey.random(rng)                                    # :49
        msgs, off = pack_messages([bytes(msg)])
        a = lambda b: np.frombuffer(b, dtype=np.uint8)  # noqa: E731
        o = eng.sign_batch(1 if self.v1 else 2, msgs, off, a(self.secret_key.to_bytes()), a(r.to_bytes()))
        return self._signature(o, msg)

    def _signature(self, o, msg: bytes) -> PlumeSignature:
        st = int(o["status"][0])
        if st & STATUS_SELFCHECK_FAILED:
            raise PlumeSelfCheckError("the signature does not verify and was withheld")
        if st & 4 and AffinePoint.from_bytes64(o["nullifier"][0]).is_identity:
            raise PlumePanic("something is drammatically wrong if the input hashed to the identity")               # :61
        if st & 1:
            raise PlumePanic("it should be impossible to get the hash equal to zero")                             # :91
        if st & 4:
            raise PlumePanic("something is terribly wrong if the nonce is equal to negated product of the secret and the hash")  # :95
        pt = lambda k: AffinePoint.from_bytes64(o[k][0].tobytes())  # noqa: E731
        return PlumeSignature(
            message=bytes(msg), pk=pt("pk"), nullifier=pt("nullifier"),
            c=NonZeroScalar.from_repr(o["c"][0].tobytes()), s=NonZeroScalar.from_repr(o["s"][0].tobytes()),
            v1specific=PlumeSignatureV1Fields(pt("r_point"), pt("hashed_to_curve_r")) if self.v1 else None)

    def sign_with_rng(self, rng, msg: bytes) -> PlumeSignature:
        return self.try_sign_with_rng(rng, msg)

    def sign_deterministic(self, msg: bytes, aux: Optional[bytes] = None) -> PlumeSignature:
        """sign with the nonce derived on the GPU by RFC 6979 from (secret key, version, message), hedged with the 32 bytes of aux when given
        (include/plume_hip.h, plume_sign_batch_rfc6979).  The same inputs give the same signature; no RNG is needed."""
        eng = self._engine or default_engine()
        if aux is not None and len(bytes(aux)) != 32:
            raise ValueError("aux must be 32 bytes")
        msgs, off = pack_messages([bytes(msg)])
        a = lambda b: np.frombuffer(bytes(b), dtype=np.uint8)  # noqa: E731
        o = eng.sign_batch_rfc6979(1 if self.v1 else 2, msgs, off, a(self.secret_key.to_bytes()), None if aux is None else a(aux))
        return self._signature(o, msg)


# ------------------------------------------------------------------------------------------- plume_arkworks shape
class PlumeVersion(Enum):  # rust-arkworks/src/lib.rs:66-69
    V1 = 1
    V2 = 2


@dataclass
class PlumeSignaturePublic:  # rust-arkworks/src/lib.rs:185-191
    message: bytes
    s: int
    nullifier: AffinePoint
    variant: Optional[PlumeVersion]


@dataclass
class PlumeSignaturePrivate:  # rust-arkworks/src/lib.rs:194-201
    hashed_to_curve_r: AffinePoint
    r_point: AffinePoint
    digest_private: int
    variant: PlumeVersion

    def zeroize(self):  # lib.rs:202-208
        self.digest_private = 0
        self.hashed_to_curve_r = AffinePoint()
        self.r_point = AffinePoint()


def sign_with_r(keypair: Tuple[AffinePoint, int], message: bytes, r_scalar: int, version: PlumeVersion,
                engine: Optional[Engine] = None) -> Tuple[PlumeSignaturePublic, PlumeSignaturePrivate]:
    """plume_arkworks::sign_with_r (rust-arkworks/src/lib.rs:229-278): pk supplied (not recomputed), explicit r,
    c reduced mod n (never panics), result split public / private."""
    eng = engine or default_engine()
    pk, sk = keypair
    if pk.is_identity:
        raise SignatureError("`pk` shouldn't be the identity element")      # lib.rs:99-101
    msgs, off = pack_messages([bytes(message)])
    a = lambda b: np.frombuffer(b, dtype=np.uint8)  # noqa: E731
    o = eng.sign_batch(version.value, msgs, off, a((sk % _N).to_bytes(32, "big")), a((r_scalar % _N).to_bytes(32, "big")), pk_in=a(pk.to_bytes64()))
    if int(o["status"][0]) & STATUS_SELFCHECK_FAILED:                       # Engine.set_sign_selfcheck(1): e.g. a pk that is not sk G
        raise PlumeSelfCheckError("the signature does not verify under the supplied pk and was withheld")
    pt = lambda k: AffinePoint.from_bytes64(o[k][0].tobytes())  # noqa: E731
    return (PlumeSignaturePublic(bytes(message), int.from_bytes(o["s"][0].tobytes(), "big"), pt("nullifier"), version),
            PlumeSignaturePrivate(pt("hashed_to_curve_r"), pt("r_point"), int.from_bytes(o["c"][0].tobytes(), "big"), version))


def verify_non_zk(sig: Tuple[PlumeSignaturePublic, PlumeSignaturePrivate], pk: AffinePoint, message: bytes, version: PlumeVersion,
                  engine: Optional[Engine] = None) -> bool:
    """plume_arkworks' verify_non_zk (rust-arkworks/src/tests.rs:28-78) on the GPU: c' from the GIVEN r_point / hashed_to_curve_r, both
    equations g^s pk^-c == g^r and h^s nul^-c == z for V1 and V2, then c' == digest_private.  Raises SignatureError where the reference
    returns Err(HashToCurveError) (pk = identity, rust-arkworks/src/lib.rs:99-101)."""
    eng = engine or default_engine()
    pub, prv = sig
    msgs, off = pack_messages([bytes(message)])
    a = lambda b: np.frombuffer(b, dtype=np.uint8)  # noqa: E731
    ok = eng.verify_non_zk_batch(version.value, msgs, off, a(pk.to_bytes64()), a(pub.nullifier.to_bytes64()), a((pub.s % _N).to_bytes(32, "big")),
                                 a(prv.r_point.to_bytes64()), a(prv.hashed_to_curve_r.to_bytes64()), a((prv.digest_private % _N).to_bytes(32, "big")))
    if int(ok[0]) == 2:
        raise SignatureError("`pk` shouldn't be the identity element")
    return bool(ok[0])


def _ecdsa_recover(what: str, want, hash32: bytes, r: bytes, s: bytes, v: int, engine: Optional[Engine]):
    hash32, r, s = bytes(hash32), bytes(r), bytes(s)
    if len(hash32) != 32 or len(r) != 32 or len(s) != 32:
        raise ValueError(f"{what}: hash32, r and s are 32 big-endian bytes each")
    if not 0 <= int(v) <= 255:
        raise ValueError(f"{what}: v is one byte")
    a = lambda b: np.frombuffer(b, dtype=np.uint8)  # noqa: E731
    pk, address, status = (engine or default_engine()).ecdsa_recover_batch(a(hash32), a(r), a(s), np.array([int(v)], dtype=np.uint8), want=want)
    if int(status[0]) == ECDSA_INVALID:
        raise SignatureError(f"{what}: the signature recovers no public key")
    return pk, address


def ecdsa_recover(hash32: bytes, r: bytes, s: bytes, v: int, engine: Optional[Engine] = None) -> Tuple[AffinePoint, bytes]:
    """The public key and the 20-byte Ethereum address behind one ECDSA signature over the 32-byte digest hash32, recovered on the GPU (include/plume_hip.h,
    plume_ecdsa_recover_batch: Ethereum's ecrecover).  r, s: 32 big-endian bytes; v: 0, 1, 27 or 28.  Raises SignatureError when the library rejects the item: v, r or s
    out of range, no curve point with x = r, or a key that comes out as the identity."""
    pk, address = _ecdsa_recover("ecdsa_recover", ("pk", "address", "status"), hash32, r, s, v, engine)
    return AffinePoint.from_bytes64(pk[0].tobytes()), address[0].tobytes()


def ecdsa_recover_address(hash32: bytes, r: bytes, s: bytes, v: int, engine: Optional[Engine] = None) -> bytes:
    """ecdsa_recover for callers that want the 20 address bytes only"""
    return _ecdsa_recover("ecdsa_recover_address", ("address", "status"), hash32, r, s, v, engine)[1][0].tobytes()


def _b32(what: str, name: str, b) -> bytes:
    b = bytes(b)
    if len(b) != 32:
        raise ValueError(f"{what}: {name} is 32 bytes")
    return b


def ecdsa_sign(sk, hash32: bytes, aux: Optional[bytes] = None, engine: Optional[Engine] = None, v27: bool = False) -> Tuple[bytes, bytes, int]:
    """A deterministic ECDSA signature (r, s, v) by sk over the 32-byte digest hash32, made on the GPU (include/plume_hip.h, plume_ecdsa_sign_batch): the RFC 6979 nonce over
    the digest itself -- byte-identical to geth, ethers and libsecp256k1 -- hedged with the 32 bytes of aux when given; always low s; v 0 / 1, or 27 / 28 with v27.  sk: a
    SecretKey or 32 big-endian bytes.  Raises SignatureError when sk is outside [1, n - 1] or the outcome is degenerate (status 2 / 4), PlumeSelfCheckError when the
    self-check withheld the signature."""
    sk32 = _b32("ecdsa_sign", "sk", sk.to_bytes() if isinstance(sk, SecretKey) else sk)
    a = lambda b: np.frombuffer(b, dtype=np.uint8)  # noqa: E731
    r, s, v, status = (engine or default_engine()).ecdsa_sign_batch(a(_b32("ecdsa_sign", "hash32", hash32)), a(sk32), None if aux is None else a(_b32("ecdsa_sign", "aux", aux)),
                                                                    v27=v27)
    st = int(status[0])
    if st == 8:
        raise PlumeSelfCheckError("ecdsa_sign: the signature did not recover the signer's key and was withheld")
    if st:
        raise SignatureError(f"ecdsa_sign: no signature (status {st}: {'sk outside [1, n - 1]' if st == 2 else 'a degenerate outcome'})")
    return r[0].tobytes(), s[0].tobytes(), int(v[0])


def personal_sign(sk, msg: bytes, aux: Optional[bytes] = None, engine: Optional[Engine] = None) -> bytes:
    """A wallet's personal_sign: the 65 bytes r || s || v (v = 27 / 28) of ecdsa_sign over the EIP-191 digest Keccak-256("\\x19Ethereum Signed Message:\\n" || len || msg),
    digest and signature both made on the GPU"""
    eng = engine or default_engine()
    msgs, off = pack_messages([bytes(msg)])
    r, s, v = ecdsa_sign(sk, eng.eth_message_hash_batch(msgs, off, "eip191")[0].tobytes(), aux, eng, v27=True)
    return r + s + bytes([v])


def personal_recover(msg: bytes, sig65: bytes, engine: Optional[Engine] = None) -> Tuple[AffinePoint, bytes]:
    """The public key and the 20-byte address that personal_sign'ed msg: the EIP-191 digest, then ecdsa_recover.  sig65: r || s || v with v 0, 1, 27 or 28"""
    sig65 = bytes(sig65)
    if len(sig65) != 65:
        raise ValueError("personal_recover: sig65 is the 65 bytes r || s || v")
    eng = engine or default_engine()
    msgs, off = pack_messages([bytes(msg)])
    return ecdsa_recover(eng.eth_message_hash_batch(msgs, off, "eip191")[0].tobytes(), sig65[:32], sig65[32:64], sig65[64], eng)


def tx_signing_hash(raw: bytes, engine: Optional[Engine] = None) -> bytes:
    """The 32 bytes the sender of one raw signed transaction signed, made on the GPU (include/plume_hip.h, plume_eth_tx_parse_batch): legacy (unprotected or EIP-155) and the
    typed envelopes 01 - 04.  Raises SignatureError for an item that is no such transaction (the envelope, the top-level framing or a signature field breaks the rule)."""
    msgs, off = pack_messages([bytes(raw)])
    out = (engine or default_engine()).eth_tx_parse_batch(msgs, off)
    if int(out["status"][0]) != ETH_TX_OK:
        raise SignatureError("tx_signing_hash: not a signed transaction of a known kind")
    return out["hash"][0].tobytes()


def sign_tx(sk, unsigned: bytes, aux: Optional[bytes] = None, engine: Optional[Engine] = None) -> bytes:
    """The signed raw transaction of one UNSIGNED serialization -- exactly the bytes whose Keccak-256 the sender signs --, framed, hashed, signed and assembled on the GPU
    (include/plume_hip.h, plume_eth_tx_sign_batch): legacy with 6 items (unprotected) or 9 (EIP-155: chainId, then two empty strings), or a typed envelope 01 - 04 without
    its last three fields.  The signature is ecdsa_sign's over that hash, hedged with the 32 bytes of aux when given.  sk: a SecretKey or 32 big-endian bytes.  Raises
    SignatureError for an item that is no such payload, for an sk outside [1, n - 1] and for a degenerate outcome, PlumeSelfCheckError when the self-check withheld the
    signature.  tx_sender(sign_tx(sk, u)) is the key's address."""
    sk32 = _b32("sign_tx", "sk", sk.to_bytes() if isinstance(sk, SecretKey) else sk)
    a = lambda b: np.frombuffer(b, dtype=np.uint8)  # noqa: E731
    raw, status = (engine or default_engine()).eth_tx_sign_batch([bytes(unsigned)], a(sk32), None if aux is None else a(_b32("sign_tx", "aux", aux)))
    st = int(status[0])
    if st & STATUS_BAD_TX:
        raise SignatureError("sign_tx: not an unsigned transaction of a known kind")
    if st & 8:
        raise PlumeSelfCheckError("sign_tx: the signature did not recover the signer's key and was withheld")
    if st:
        raise SignatureError(f"sign_tx: no signature (status {st}: {'sk outside [1, n - 1]' if st == 2 else 'a degenerate outcome'})")
    return raw[0]


# ------------------------------------------------------------------------------------------------ BIP-32 (library 0.17)
def parse_path(path: str):
    """The indices of a BIP-32 path: "m/44'/60'/0'/0/3" or, relative to a node, "0/3".  A component is a decimal number below 2^31; a trailing ' or h makes it
    hardened (+ 2^31).  At most 8 components (PLUME_HD_MAX_DEPTH); "m" alone, "m/" and an empty component are errors (ValueError)."""
    parts = str(path).split("/")
    if parts[0] == "m":
        parts = parts[1:]
    if not 1 <= len(parts) <= HD_MAX_DEPTH:
        raise ValueError(f"parse_path: {path!r} has {len(parts)} components; 1 .. {HD_MAX_DEPTH} are derived")
    out = []
    for c in parts:
        hard = c[-1:] in ("'", "h")
        num = c[:-1] if hard else c
        if not num.isascii() or not num.isdigit() or int(num) >= HD_HARDENED:
            raise ValueError(f"parse_path: component {c!r} of {path!r} is not an index below 2^31")
        out.append(int(num) + (HD_HARDENED if hard else 0))
    return out


def _hd_status(what: str, st: int):
    if st == STATUS_HD_HARDENED:
        raise SignatureError(f"{what}: a public key has no hardened children")
    if st == STATUS_HD_NO_KEY:
        raise SignatureError(f"{what}: the path has no key (BIP-32: IL >= n or a zero child; take the next index)")
    if st:
        raise SignatureError(f"{what}: the parent key is not valid (status {st})")


def _hd_path(path):
    return np.array([parse_path(path) if isinstance(path, str) else [int(i) for i in path]], dtype=np.uint32)


def hd_master(seed: bytes, engine: Optional[Engine] = None) -> Tuple[bytes, bytes]:
    """The BIP-32 master node (sk, chain) of a seed of 16 .. 64 bytes, made on the GPU (include/plume_hip.h, plume_hd_master_batch): HMAC-SHA512("Bitcoin seed", seed).
    The seed of a BIP-39 mnemonic is mnemonic_to_seed(mnemonic, passphrase), made on the GPU too; Engine.bip39_accounts chains both without a host copy of the seed."""
    seed = bytes(seed)
    if not 16 <= len(seed) <= 64:
        raise ValueError("hd_master: a seed is 16 .. 64 bytes")
    sk, chain, status = (engine or default_engine()).hd_master_batch(np.frombuffer(seed, dtype=np.uint8).reshape(1, -1))
    _hd_status("hd_master", int(status[0]))
    return sk[0].tobytes(), chain[0].tobytes()


def hd_derive(sk, chain: bytes, path, engine: Optional[Engine] = None) -> Tuple[bytes, bytes]:
    """The node (sk, chain) at `path` below the node (sk, chain): BIP-32's CKDpriv along "m/44'/60'/0'/0/3" (or a list of indices), on the GPU
    (plume_hd_derive_priv_batch).  sk: a SecretKey or 32 big-endian bytes.  Raises SignatureError for a parent outside [1, n - 1] and for a path that has no key."""
    sk32 = _b32("hd_derive", "sk", sk.to_bytes() if isinstance(sk, SecretKey) else sk)
    a = lambda b: np.frombuffer(b, dtype=np.uint8)  # noqa: E731
    res = (engine or default_engine()).hd_derive_priv_batch(a(sk32), a(_b32("hd_derive", "chain", chain)), _hd_path(path), want=("chain",))
    _hd_status("hd_derive", int(res["status"][0]))
    return res["sk"][0].tobytes(), res["chain"][0].tobytes()


def hd_derive_pub(pk, chain: bytes, path, engine: Optional[Engine] = None) -> Tuple[AffinePoint, bytes]:
    """The public node (pk, chain) at the non-hardened `path` ("0/3") below the public node (pk, chain): BIP-32's CKDpub on the GPU (plume_hd_derive_pub_batch) --
    what a watcher holding an xpub derives.  pk: an AffinePoint, 64 bytes x || y or 33 SEC1 bytes.  Raises SignatureError for a hardened index, an invalid key, no key."""
    pk = pk.to_bytes64() if isinstance(pk, AffinePoint) else bytes(pk)
    if len(pk) not in (33, 64):
        raise ValueError("hd_derive_pub: pk is 64 bytes x || y or 33 SEC1 bytes")
    a = lambda b: np.frombuffer(b, dtype=np.uint8)  # noqa: E731
    eng = engine or default_engine()
    if len(pk) == 33:                                                        # SEC1 in, 64 bytes out: two calls would do it; one, with the address call's decoder, is enough
        res = eng.hd_derive_pub_batch(a(pk), a(_b32("hd_derive_pub", "chain", chain)), _hd_path(path), pk_format="sec1", want=("chain",))
        _hd_status("hd_derive_pub", int(res["status"][0]))
        x = int.from_bytes(res["pk"][0, 1:].tobytes(), "big")
        y = pow((x * x * x + 7) % _P, (_P + 1) // 4, _P)
        return AffinePoint(x, y if (y & 1) == (int(res["pk"][0, 0]) & 1) else _P - y), res["chain"][0].tobytes()
    res = eng.hd_derive_pub_batch(a(pk), a(_b32("hd_derive_pub", "chain", chain)), _hd_path(path), want=("chain",))
    _hd_status("hd_derive_pub", int(res["status"][0]))
    return AffinePoint.from_bytes64(res["pk"][0].tobytes()), res["chain"][0].tobytes()


def hd_address(key, chain: bytes, path, engine: Optional[Engine] = None) -> bytes:
    """The 20-byte Ethereum address of the key at `path`: below a private node (key: a SecretKey or 32 bytes; any path) or below a public one (key: an AffinePoint, 64 or
    33 bytes; non-hardened indices only).  hd_address(*hd_master(seed), "m/44'/60'/0'/0/0") is a wallet's first account."""
    a = lambda b: np.frombuffer(b, dtype=np.uint8)  # noqa: E731
    eng = engine or default_engine()
    if isinstance(key, SecretKey) or (not isinstance(key, AffinePoint) and len(bytes(key)) == 32):
        sk32 = _b32("hd_address", "sk", key.to_bytes() if isinstance(key, SecretKey) else key)
        res = eng.hd_derive_priv_batch(a(sk32), a(_b32("hd_address", "chain", chain)), _hd_path(path), want=("address",))
    else:
        pk = key.to_bytes64() if isinstance(key, AffinePoint) else bytes(key)
        if len(pk) not in (33, 64):
            raise ValueError("hd_address: key is a 32-byte sk, or a pk of 64 bytes x || y or 33 SEC1 bytes")
        res = eng.hd_derive_pub_batch(a(pk), a(_b32("hd_address", "chain", chain)), _hd_path(path), pk_format="sec1" if len(pk) == 33 else "affine64", want=("address",))
    _hd_status("hd_address", int(res["status"][0]))
    return res["address"][0].tobytes()


# ------------------------------------------------------------------------------------------------ BIP-39 seeds (library 0.18)
def pbkdf2_sha512(password, salt, iterations: int, dklen: int = 64, engine: Optional[Engine] = None) -> bytes:
    """PBKDF2-HMAC-SHA512(password, salt, iterations)[:dklen] on the GPU (plume_pbkdf2_sha512_batch): hashlib.pbkdf2_hmac("sha512", ...) for 1 <= dklen <= 64, a salt of
    at most 256 bytes and at most 2^24 iterations.  str arguments are NFKD-normalised and UTF-8 encoded, bytes taken as given."""
    out, status = (engine or default_engine()).pbkdf2_sha512_batch([bip39_bytes(password)], bip39_bytes(salt), iterations, dklen)
    if int(status[0]):
        raise SignatureError(f"pbkdf2_sha512: not derived (status {int(status[0])})")
    return out[0].tobytes()


def mnemonic_to_seed(mnemonic, passphrase="", engine: Optional[Engine] = None) -> bytes:
    """The 64-byte BIP-39 seed of a mnemonic sentence, made on the GPU: PBKDF2-HMAC-SHA512(sentence, "mnemonic" || passphrase, 2048).  str arguments are
    NFKD-normalised and UTF-8 encoded as BIP-39 says, bytes taken as given.  The sentence is not checked against the word list (out of scope: any bytes have a seed)."""
    seed, status = (engine or default_engine()).bip39_seed_batch([bip39_bytes(mnemonic)], bip39_bytes(passphrase))
    if int(status[0]):
        raise SignatureError(f"mnemonic_to_seed: not derived (status {int(status[0])})")
    return seed[0].tobytes()


def mnemonic_to_address(mnemonic, path="m/44'/60'/0'/0/0", passphrase="", engine: Optional[Engine] = None) -> bytes:
    """The 20-byte Ethereum address of the account at `path` of a mnemonic sentence: seed, master node and the derivation chained on the GPU (Engine.bip39_accounts);
    neither the seed nor a key comes to the host.  Raises SignatureError for a path that has no key."""
    res = (engine or default_engine()).bip39_accounts([bip39_bytes(mnemonic)], bip39_bytes(passphrase), path, want=("address",))
    _hd_status("mnemonic_to_address", int(res["status"][0]))
    return res["address"][0].tobytes()


_B58 = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"


def _xkey(what: str, s: str, version: bytes) -> bytes:
    import hashlib
    v = 0
    for ch in str(s):
        d = _B58.find(ch)
        if d < 0:
            raise ValueError(f"{what}: {ch!r} is not a base58 digit")
        v = v * 58 + d
    raw = v.to_bytes(82, "big") if v < 1 << (8 * 82) else b""
    if len(raw) != 82 or hashlib.sha256(hashlib.sha256(raw[:78]).digest()).digest()[:4] != raw[78:]:
        raise ValueError(f"{what}: not 78 bytes with a valid base58check checksum")
    if raw[:4] != version:
        raise ValueError(f"{what}: version bytes {raw[:4].hex()}, expected {version.hex()}")
    return raw[:78]


def parse_xprv(s: str) -> Tuple[int, int, bytes, bytes]:
    """(depth, child_number, chain, sk) of a mainnet extended private key "xprv..." -- base58check DECODE only: hd_derive(sk, chain, path) takes it from there.
    ValueError for a bad digit, length, checksum, version or key byte."""
    b = _xkey("parse_xprv", s, bytes.fromhex("0488ade4"))
    if b[45] != 0:
        raise ValueError("parse_xprv: the key is not 00 || 32 bytes")
    return b[4], int.from_bytes(b[9:13], "big"), b[13:45], b[46:78]


def parse_xpub(s: str) -> Tuple[int, int, bytes, bytes]:
    """(depth, child_number, chain, pk33) of a mainnet extended public key "xpub...": hd_derive_pub(pk33, chain, path) takes it from there"""
    b = _xkey("parse_xpub", s, bytes.fromhex("0488b21e"))
    if b[45] not in (2, 3):
        raise ValueError("parse_xpub: the key is not a compressed point")
    return b[4], int.from_bytes(b[9:13], "big"), b[13:45], b[45:78]


def _tx_sender(what: str, want, raw: bytes, engine: Optional[Engine], low_s: bool):
    msgs, off = pack_messages([bytes(raw)])
    pk, address, status, _, _ = (engine or default_engine()).eth_tx_sender_batch(msgs, off, low_s=low_s, want=want)
    if int(status[0]) == ECDSA_INVALID:
        raise SignatureError(f"{what}: no sender (not a signed transaction of a known kind, or its signature recovers no public key)")
    return pk, address


def tx_sender(raw: bytes, engine: Optional[Engine] = None, low_s: bool = True) -> Tuple[AffinePoint, bytes]:
    """The public key and the 20-byte address of the sender of one raw signed transaction, framed, hashed and recovered on the GPU (plume_eth_tx_sender_batch).  low_s: the
    EIP-2 rule, right for everything after Homestead.  A sender recovery, not a consensus decoder: inner fields are not validated.  Raises SignatureError when there is no
    sender."""
    pk, address = _tx_sender("tx_sender", ("pk", "address", "status"), raw, engine, low_s)
    return AffinePoint.from_bytes64(pk[0].tobytes()), address[0].tobytes()


def tx_sender_address(raw: bytes, engine: Optional[Engine] = None, low_s: bool = True) -> bytes:
    """tx_sender for callers that want the 20 address bytes only"""
    return _tx_sender("tx_sender_address", ("address", "status"), raw, engine, low_s)[1][0].tobytes()


def circuit_inputs(sig: "PlumeSignature", engine: Optional[Engine] = None) -> dict:
    """All inputs of the circom verifier (circuits/circom/verify_nullifier.circom:14-31; test/v1.test.ts:68-78) for one signature, as lists of four 64-bit
    little-endian registers (circuits/circom/utils.ts:11-17): c, s, pk, nullifier from the signature, q{0,1}_x_mapped / q{0,1}_y_mapped from the GPU hash_to_curve
    (pinned), and q{0,1}_gx1_sqrt / gx2_sqrt / y_pos as include/plume_hip.h DEFINES them (UNPINNED: their generator is not vendored in the reference tree)."""
    from .capi import registers_from_be
    eng = engine or default_engine()
    msgs, off = pack_messages([bytes(sig.message)])
    a = lambda b: np.frombuffer(b, dtype=np.uint8)  # noqa: E731
    o = eng.h2c_intermediates_batch(msgs, off, a(sig.pk.to_bytes64()), registers=True)
    reg = lambda b: [int(x) for x in registers_from_be(a(b).reshape(1, 32))[0]]  # noqa: E731
    pt = lambda p: [reg(p.to_bytes64()[:32]), reg(p.to_bytes64()[32:])]  # noqa: E731
    m = o["mapped"][0]
    hints = {k: [int(x) for x in v[0]] for k, v in eng.h2c_hints_batch(msgs, off, a(sig.pk.to_bytes64()), registers=True).items()}
    return {**hints, "c": reg(sig.c.to_bytes()), "s": reg(sig.s.to_bytes()), "plume_message": list(bytes(sig.message)), "pk": pt(sig.pk), "nullifier": pt(sig.nullifier),
            "q0_x_mapped": [int(x) for x in m[0]], "q0_y_mapped": [int(x) for x in m[1]], "q1_x_mapped": [int(x) for x in m[2]], "q1_y_mapped": [int(x) for x in m[3]]}


def circuit_outputs(sig: "PlumeSignature", engine: Optional[Engine] = None) -> dict:
    """The public outputs of the plume_v2 circuit for one signature (circuits/circom/verify_nullifier.circom:140-222; test/v2.test.ts:56-59): r_point,
    hashed_to_curve_r and hashed_to_curve as [x, y] lists of four 64-bit little-endian registers, recomputed on the GPU from pk, nullifier, c, s
    (plume_recover_batch, register format).  Raises SignatureError when an input is no value of the reference's types; whether c is the hash of the points is
    the verifier's business (sig.verify), not this function's."""
    from .capi import RECOVER_FMT_REGISTERS
    eng = engine or default_engine()
    msgs, off = pack_messages([bytes(sig.message)])
    a = lambda b: np.frombuffer(b, dtype=np.uint8)  # noqa: E731
    o = eng.recover_batch(1 if sig.v1specific else 2, msgs, off, a(sig.pk.to_bytes64()), a(sig.nullifier.to_bytes64()), a(sig.c.to_bytes()), a(sig.s.to_bytes()),
                          fmt=RECOVER_FMT_REGISTERS)
    if int(o["status"][0]) == RECOVER_INVALID:
        raise SignatureError("circuit_outputs: an input is no value of the reference's types")
    return {k: [[int(x) for x in o[k][0][j]] for j in range(2)] for k in ("r_point", "hashed_to_curve_r", "hashed_to_curve")}


def sign(rng, keypair: Tuple[AffinePoint, int], message: bytes, version: PlumeVersion, engine: Optional[Engine] = None):
    """plume_arkworks::sign (rust-arkworks/src/lib.rs:281-291): r = Fr::rand(rng)"""
    r = int.from_bytes(rng.fill_bytes(48), "big") % _N
    return sign_with_r(keypair, message, r, version, engine)


def merkle_leaf(address20: bytes, amount: Optional[int] = None, engine: Optional[Engine] = None) -> bytes:
    """The leaf of one account in OpenZeppelin's StandardMerkleTree, made on the GPU (plume_merkle_leaf_batch): Keccak(Keccak(abi.encode(address))) for the tree of
    ["address"], Keccak(Keccak(abi.encode(address, amount))) for the tree of ["address", "uint256"] when amount is given."""
    if len(bytes(address20)) != 20:
        raise ValueError("merkle_leaf: address20 is 20 raw bytes")
    leaf, _ = (engine or default_engine()).merkle_leaf_batch(np.frombuffer(bytes(address20), dtype=np.uint8), None if amount is None else [int(amount)],
                                                             "address" if amount is None else "address_uint256")
    return leaf[0].tobytes()


def merkle_root(leaves, sort: bool = True, engine: Optional[Engine] = None) -> bytes:
    """The root of the tree over 32-byte leaves, built on the GPU (plume_merkle_tree_build); sort: order the leaves by hash first, as StandardMerkleTree does"""
    return (engine or default_engine()).merkle_tree(leaves, sort=sort, leaf_format="hash32").root


def merkle_proof(leaves, index: int, sort: bool = True, engine: Optional[Engine] = None):
    """The proof of leaf `index` of the tree over 32-byte leaves, as a list of 32-byte siblings (plume_merkle_tree_build, plume_merkle_proof_batch)"""
    return (engine or default_engine()).merkle_tree(leaves, sort=sort, leaf_format="hash32").proof(index)


def merkle_verify(leaf, proof, root32: bytes, amount: Optional[int] = None, engine: Optional[Engine] = None) -> bool:
    """MerkleProof.verify on the GPU (plume_merkle_verify_batch).  leaf: 32 bytes, a leaf as it is; or 20 bytes, an address whose leaf is computed first (with `amount`
    for the tree of ["address", "uint256"]).  proof: the 32-byte siblings, leaf side first."""
    leaf, proof = bytes(leaf), [bytes(p) for p in proof]
    if len(leaf) not in (20, 32) or any(len(p) != 32 for p in proof) or len(bytes(root32)) != 32:
        raise ValueError("merkle_verify: leaf is 32 bytes (or a 20-byte address), proof elements and root are 32 bytes")
    if len(proof) > 64:
        return False
    fmt = "hash32" if len(leaf) == 32 else "address" if amount is None else "address_uint256"
    a = lambda b: np.frombuffer(b, dtype=np.uint8)  # noqa: E731
    st = (engine or default_engine()).merkle_verify_batch(a(leaf), a(b"".join(proof)).reshape(1, len(proof), 32), np.array([len(proof)], dtype=np.uint8), a(bytes(root32)),
                                                          None if fmt != "address_uint256" else [int(amount)], fmt)
    return int(st[0]) == MERKLE_MATCH
