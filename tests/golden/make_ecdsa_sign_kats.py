#!/usr/bin/env python3
"""Writes tests/golden/ecdsa_sign_kats.json: the vectors the ECDSA signing tests pin (python tests/golden/make_ecdsa_sign_kats.py).  Everything is made by the
restatement in tests/_ecdsa_sign.py from fixed and seeded inputs, so the file is reproducible; while writing it this script ASSERTS
  (a) the three widely published RFC 6979 / secp256k1 / SHA-256 vectors (sk, message -> k, r, s, v), re-derived here from sk and the message;
  (b) that OpenSSL's libcrypto (through ctypes: ECDSA_do_verify on a key and a signature set from the fixture's bytes) accepts every signature with status 0;
  (c) the Keccak-256 pins: "", "abc", and the EIP-191 digest of "hello world".
"public": the three vectors.  "sign": 36 seeded keys and digests, then the crafted items -- sk and hash on both sides of every reduction, eight items whose s is high
before the low-s rule and eight where it is low (found by search, recorded as "high"), each of them plain and hedged with a fixed aux -- with what the restatement says
of them (r, s, v in {0, 1}, status).  "hash": messages of the lengths that sit on the rate's and the decimal width's edges, in both modes, with their digests."""
import ctypes
import ctypes.util
import hashlib
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
from tests import _ecdsa as E  # noqa: E402
from tests import _ecdsa_sign as S  # noqa: E402
from tests import _keccak as K  # noqa: E402

NID_SECP256K1 = 714
COUNT = 36

lib = ctypes.CDLL(ctypes.util.find_library("crypto"))
for name, res, args in [("EC_KEY_new_by_curve_name", ctypes.c_void_p, [ctypes.c_int]), ("EC_KEY_free", None, [ctypes.c_void_p]),
                        ("EC_KEY_set_public_key_affine_coordinates", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
                        ("ECDSA_SIG_new", ctypes.c_void_p, []), ("ECDSA_SIG_free", None, [ctypes.c_void_p]),
                        ("ECDSA_SIG_set0", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
                        ("ECDSA_do_verify", ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
                        ("BN_bin2bn", ctypes.c_void_p, [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p]), ("BN_free", None, [ctypes.c_void_p])]:
    f = getattr(lib, name)
    f.restype, f.argtypes = res, args


def openssl_accepts(pk64: bytes, hash32: bytes, r32: bytes, s32: bytes) -> bool:
    key = lib.EC_KEY_new_by_curve_name(NID_SECP256K1)
    x, y = lib.BN_bin2bn(pk64[:32], 32, None), lib.BN_bin2bn(pk64[32:], 32, None)
    assert key and x and y and lib.EC_KEY_set_public_key_affine_coordinates(key, x, y) == 1
    sig = lib.ECDSA_SIG_new()
    assert sig and lib.ECDSA_SIG_set0(sig, lib.BN_bin2bn(r32, 32, None), lib.BN_bin2bn(s32, 32, None)) == 1      # (the signature owns r and s now)
    ok = lib.ECDSA_do_verify(hash32, 32, sig, key)
    lib.ECDSA_SIG_free(sig); lib.BN_free(x); lib.BN_free(y); lib.EC_KEY_free(key)
    return ok == 1


# ------------------------------------------------------------------------------------------------ (a) the published vectors
PUBLISHED = [
    (1, b"Satoshi Nakamoto", "8f8a276c19f4149656b280621e358cce24f5f52542772691ee69063b74f15d15",
     "934b1ea10a4b3c1757e2b0c017d0b6143ce3c9a7e6a4a49860d7a6ab210ee3d8", "2442ce9d2b916064108014783e923ec36b49743e2ffa1c4496f01a512aafd9e5", 1),
    (1, b"All those moments will be lost in time, like tears in rain. Time to die...", "38aa22d72376b4dbc472e06c3ba403ee0a394da63fc58d88686c611aba98d6b3",
     "8600dbd4", "547fe644", 0),
    (E.N - 1, b"Satoshi Nakamoto", "33a19b60e25fb6f4435af53a3d42d493644827367e6453928554f43e49aa6f90", "fd567d12", "6b39cd0e", 0),
]
public = []
for sk, msg, k_hex, r_hex, s_hex, v in PUBLISHED:
    sk32, h = E.b32(sk), hashlib.sha256(msg).digest()
    assert E.b32(S.nonce(sk32, h)).hex() == k_hex, msg
    r, s, got_v, st = S.sign(sk32, h)
    assert st == S.OK and E.b32(r).hex().startswith(r_hex) and E.b32(s).hex().startswith(s_hex) and got_v == v, (msg, E.b32(r).hex(), E.b32(s).hex(), got_v)
    public.append({"sk": sk32.hex(), "msg": msg.decode(), "hash": h.hex(), "k": k_hex, "r": E.b32(r).hex(), "s": E.b32(s).hex(), "v": v})

# ------------------------------------------------------------------------------------------------ (c) the hash pins
assert K.keccak256(b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
assert K.keccak256(b"abc").hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"
assert S.message_hash(b"hello world", S.EIP191).hex() == "d9eba16ed0ecae432b71fe008c98cc872bb4cc214d3220a36f365326cf807d68"
hashes = []
for mode, lengths in S.HASH_LENGTHS.items():
    for j, L in enumerate(lengths):
        msg = S.message_of(L, j + 100 * mode)
        hashes.append({"mode": mode, "msg": msg.hex(), "digest": S.message_hash(msg, mode).hex()})
hashes.append({"mode": S.EIP191, "msg": b"hello world".hex(), "digest": S.message_hash(b"hello world", S.EIP191).hex()})

# ------------------------------------------------------------------------------------------------ the sign items
items = []                                                              # (name, sk32, hash32, aux or None, high or None)
sk_s, h_s, _ = S.seeded(COUNT, 20260613)
for i in range(COUNT):
    items.append((f"seeded {i}", sk_s[i].tobytes(), h_s[i].tobytes(), None, None))
sk0, h0 = E.b32(0x519B423D715F8B581F4FA8EE59F4771A5B44C8130B4E3EACCA54A56DDA72B464), bytes(range(32))
crafted = [(f"sk = {hex(sk) if sk > 2 else sk}", E.b32(sk), h0) for sk in S.SK_EDGES] + [(f"hash = {hex(h) if h > 1 else h}", sk0, E.b32(h)) for h in S.HASH_EDGES]
for aux in (None, S.FIXED_AUX):
    for name, sk32, h in crafted:
        items.append((name + (", hedged" if aux else ""), sk32, h, aux, None))
    found = {True: 0, False: 0}                                         # eight items whose s is high before the low-s rule, eight where it is low: by search
    sk_c, h_c, _ = S.seeded(64, 777)
    for i in range(64):
        st, _, s, _, _ = S.sign_raw(sk_c[i].tobytes(), h_c[i].tobytes(), aux)
        high = s > S.HALF_N
        if st == S.OK and found[high] < 8:
            found[high] += 1
            items.append((f"{'high' if high else 'low'} s {found[high]}" + (", hedged" if aux else ""), sk_c[i].tobytes(), h_c[i].tobytes(), aux, high))
    assert found == {True: 8, False: 8}, found

sign = []
for name, sk32, h, aux, high in items:
    r, s, v, st = S.sign(sk32, h, aux)
    if st == S.OK:
        assert 1 <= r < E.N and 1 <= s <= S.HALF_N and v in (0, 1)
        Q = E.mul(int.from_bytes(sk32, "big"))
        assert openssl_accepts(E.pk_record(Q, "affine64"), h, E.b32(r), E.b32(s)), name                   # (b)
        assert not openssl_accepts(E.pk_record(Q, "affine64"), h, E.b32(r), E.b32(s ^ 1)), name           # ... and it is the signature that it accepts
        assert E.recover(h, r, s, v, E.LOW_S) == Q, name
    else:
        assert st == S.BAD_SCALAR and not 1 <= int.from_bytes(sk32, "big") < E.N, name                  # no seed here reaches a degenerate outcome
    sign.append({"name": name, "sk": sk32.hex(), "hash": h.hex(), "aux": None if aux is None else aux.hex(), "r": E.b32(r).hex(), "s": E.b32(s).hex(), "v": v, "status": st,
                 "high": high})
assert sum(1 for e in sign if e["status"] == S.BAD_SCALAR) == 2 * 4 and np.unique([e["v"] for e in sign if e["status"] == S.OK]).tolist() == [0, 1]

S.KATS.write_text(json.dumps({"public": public, "sign": sign, "hash": hashes}, indent=1) + "\n")
print(f"wrote {S.KATS.name}: {len(public)} published vectors, {len(sign)} sign items, {len(hashes)} messages")
for p in public:
    print(" ", p["r"], p["s"], p["v"])
