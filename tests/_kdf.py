"""PBKDF2-HMAC-SHA512 for a batch, restated for the tests of plume_pbkdf2_sha512_batch (include/plume_hip.h, "library 0.18"): hashlib.pbkdf2_hmac item by item plus the
call's own rules -- the status of an item whose offsets are unsound (device form), its all-zero record, the "mnemonic" prefix of PLUME_KDF_BIP39, the one record of
PLUME_KDF_SHARED_SALT.  And seeded batches whose password lengths are planted, not random: the lengths at which the lane bodies change course."""
import functools
import hashlib

import numpy as np

BIP39, SHARED_SALT = 1, 2
MAX_SALT = 256
MAX_ITERATIONS = 1 << 24
BAD_INPUT = 128
SLICE = 256                                               # PLUME_KDF_SLICE: the rounds of one k_kdf_iter dispatch
# 0 / 1: an empty and a one-byte key; 111 / 112: nothing special for a KEY (it is zero-padded, not hashed) but the lengths at which a hashed message's padding spills;
# 128 / 129: the last raw key and the first hashed one; 239 / 240: two and three blocks of key hashing; 300: well inside three
PLANTED = (0, 1, 111, 112, 128, 129, 239, 240, 300)

HARDHAT_MNEMONIC = "test test test test test test test test test test test junk"
TREZOR_MNEMONIC = "abandon abandon abandon abandon abandon abandon abandon abandon abandon abandon abandon about"
TREZOR_SEED = "c55257c360c07c72029aebc1b53c05ed0362ada38ead3e3e9efa3708e53495531f09a6987599d18264c1e1c92f2cf141630c7a3c4ab7c81b2f001698e7463b04"
RFC_STYLE = {1: "867f70cf1ade02cff3752599a3a53dc4af34c7a669815ae5d513554e1c8cf252c02d470a285a0501bad999bfe943c08f050235d7d68b1da55e63f73b60a57fce",
             2: "e1d9c16aa681708a45f5c7c4e215ceb66e011a2e9f0040713f18aefdb866d53cf76cab2868a39b9f7840edce4fef5a82be67335c77a6068e04112754f27ccf4e"}


def stage_list(iterations):
    """the stages of one device-form call with stage timing on"""
    left = iterations - 1
    return ["kdf_key"] + ["kdf_iter"] * ((left + SLICE - 1) // SLICE) + ["kdf_finish"]


def pbkdf2_batch(pw, off, pw_bytes, salt, salt_len, iterations, dklen, flags=0):
    """(out, status) as the device form gives them.  pw: the buffer; off: n + 1 offsets; salt: n records of salt_len bytes, one with SHARED_SALT, anything when salt_len
    is 0.  An item whose offsets decrease or reach past pw_bytes never reads pw"""
    n = len(off) - 1
    buf = np.asarray(pw, dtype=np.uint8).tobytes()
    rows = np.asarray(salt, dtype=np.uint8).reshape(-1, salt_len) if salt_len else None
    out, status = np.zeros((n, dklen), np.uint8), np.zeros(n, np.uint8)
    for i in range(n):
        lo, hi = int(off[i]), int(off[i + 1])
        if hi < lo or hi > pw_bytes:
            status[i] = BAD_INPUT
            continue
        s = (b"mnemonic" if flags & BIP39 else b"") + (rows[0 if flags & SHARED_SALT else i].tobytes() if salt_len else b"")
        out[i] = np.frombuffer(hashlib.pbkdf2_hmac("sha512", buf[lo:hi], s, iterations, dklen), np.uint8)
    return out, status


def planted_passwords(n, seed, lengths=PLANTED):
    """(buf, off): n seeded passwords, item i of length lengths[i % len(lengths)] -- every wavefront of 64 holds every length; buf ends with the last byte of the last item"""
    rng = np.random.default_rng(seed)
    lens = np.array([lengths[i % len(lengths)] for i in range(n)], dtype=np.uint64)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    return rng.integers(0, 256, int(off[n]), dtype=np.uint8), off


@functools.lru_cache(maxsize=None)
def planted_case(n, iterations, flags, salt_len, dklen=64):
    """one seeded batch and what the restatement says of it, computed once per process: (buf, off, salt, out, status).  The arrays are shared: leave them unchanged"""
    buf, off = planted_passwords(n, 1000 * n + iterations)
    salt = np.random.default_rng(7 * n + salt_len).integers(0, 256, (1 if flags & SHARED_SALT else n, salt_len), dtype=np.uint8)
    out, status = pbkdf2_batch(buf, off, len(buf), salt, salt_len, iterations, dklen, flags)
    return buf, off, salt, out, status
