#!/usr/bin/env python3
"""Writes tests/golden/ecdsa_recover_kats.json: the vectors the ECDSA recovery tests pin (python tests/golden/make_ecdsa_recover_kats.py).
"openssl": secp256k1 keys generated and 32-byte digests signed by OpenSSL's libcrypto (through ctypes: EC_KEY_generate_key, ECDSA_do_sign), with the public key OpenSSL
reports.  OpenSSL gives (r, s) only; v is fixed here by asserting that EXACTLY ONE of the two parities makes the restatement in tests/_ecdsa.py return OpenSSL's key -- the
restatement recovers keys it did not make from signatures it did not make.  Every third signature is stored with v + 27, and its low-s twin (r, n - s, v ^ 1) is stored
where s came out high, so that both encodings and both halves of the s range appear.
"crafted": the range edges, the identity and doubling constructions, the table and digit edges of tests/_ecdsa.py::crafted_cases, as inputs only: what they give is the
restatement's to say at test time."""
import ctypes
import ctypes.util
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
from tests import _ecdsa as E  # noqa: E402

NID_SECP256K1 = 714
COUNT = 36

lib = ctypes.CDLL(ctypes.util.find_library("crypto"))
for name, res, args in [("EC_KEY_new_by_curve_name", ctypes.c_void_p, [ctypes.c_int]), ("EC_KEY_generate_key", ctypes.c_int, [ctypes.c_void_p]),
                        ("EC_KEY_free", None, [ctypes.c_void_p]), ("EC_KEY_get0_group", ctypes.c_void_p, [ctypes.c_void_p]),
                        ("EC_KEY_get0_public_key", ctypes.c_void_p, [ctypes.c_void_p]),
                        ("EC_POINT_point2oct", ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p]),
                        ("ECDSA_do_sign", ctypes.c_void_p, [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p]), ("ECDSA_SIG_free", None, [ctypes.c_void_p]),
                        ("ECDSA_do_verify", ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
                        ("ECDSA_SIG_get0_r", ctypes.c_void_p, [ctypes.c_void_p]), ("ECDSA_SIG_get0_s", ctypes.c_void_p, [ctypes.c_void_p]),
                        ("BN_bn2binpad", ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int])]:
    f = getattr(lib, name)
    f.restype, f.argtypes = res, args


def bn(ptr):
    buf = ctypes.create_string_buffer(32)
    assert lib.BN_bn2binpad(ptr, buf, 32) == 32
    return buf.raw


openssl = []
for i in range(COUNT):
    key = lib.EC_KEY_new_by_curve_name(NID_SECP256K1)
    assert key and lib.EC_KEY_generate_key(key) == 1
    pub = ctypes.create_string_buffer(65)
    assert lib.EC_POINT_point2oct(lib.EC_KEY_get0_group(key), lib.EC_KEY_get0_public_key(key), 4, pub, 65, None) == 65 and pub.raw[0] == 4
    digest = os.urandom(32)
    sig = lib.ECDSA_do_sign(digest, 32, key)
    assert sig and lib.ECDSA_do_verify(digest, 32, sig, key) == 1
    r, s = bn(lib.ECDSA_SIG_get0_r(sig)), bn(lib.ECDSA_SIG_get0_s(sig))
    lib.ECDSA_SIG_free(sig)
    lib.EC_KEY_free(key)
    want = (int.from_bytes(pub.raw[1:33], "big"), int.from_bytes(pub.raw[33:], "big"))
    ri, si = int.from_bytes(r, "big"), int.from_bytes(s, "big")
    hits = [v for v in (0, 1) if E.recover(digest, ri, si, v) == want]
    assert len(hits) == 1, (i, hits)
    v = hits[0]
    if si > E.HALF_N and i % 2:                                          # the low-s twin is the same signature as a transaction carries it
        si, v = E.N - si, v ^ 1
        assert E.recover(digest, ri, si, v) == want and E.recover(digest, ri, si, v ^ 1) != want
    openssl.append({"hash": digest.hex(), "r": r.hex(), "s": E.b32(si).hex(), "v": v + (27 if i % 3 == 0 else 0), "pk": pub.raw[1:].hex()})

crafted = [{"name": name, "hash": h.hex(), "r": E.b32(r).hex(), "s": E.b32(s).hex(), "v": v, "flags": flags} for name, h, r, s, v, flags in E.crafted_cases()]
E.KATS.write_text(json.dumps({"openssl": openssl, "crafted": crafted}, indent=1) + "\n")
print(f"wrote {E.KATS.name}: {len(openssl)} OpenSSL signatures, {len(crafted)} crafted items")
