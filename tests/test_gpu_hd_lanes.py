"""The lane bodies of the key derivation on gfx950 (tests/hd_gpu/hd_gpu.hip: one kernel that calls hd_priv_tweak, hd_pub_tweak and hmac_sha512_37 of csrc/plume_hd.h and
csrc/plume_sha512.h, one lane per element; built by __graft_entry__.build(), never from here): the tweak functions with CHOSEN IL -- n - 1 (valid), n, n + 1, 2^256 - 1,
n - k_par (child scalar zero) and, for the public form, the IL with IL G = -K_par (the identity) -- which no HMAC will ever give, so no derivation call can reach these
branches.  Every 64-lane wavefront mixes the chosen cases of both tweaks with ordinary lanes and HMAC lanes, in a seeded shuffle; status 32 comes with an all-zero record."""
import ctypes as C
import hashlib
import hmac
from pathlib import Path

import numpy as np
import pytest

from tests import _ecdsa as E
from tests import _hd as H

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SO = ROOT / "tests" / "hd_gpu" / "libplume_hd_gpu.so"
N = H.N


def _cases():
    """(kind, a, b, c, want 64 bytes, want status) -- 4 wavefronts' worth plus a partial one"""
    rng = np.random.default_rng(3217)
    rnd = lambda: int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "big")  # noqa: E731
    out = []

    def priv(il, kp):
        w = H.priv_tweak(il, kp)
        out.append((0, H.b32(il), H.b32(kp), bytes(32), (H.b32(w) if w else bytes(32)) + bytes(32), 0 if w else H.NO_KEY))

    def pub(il, kp):
        Kp = H.g_mul(kp)
        w = H.pub_tweak(il, Kp)
        out.append((1, H.b32(il), H.b32(Kp[0]), H.b32(Kp[1]), E.pk_record(w, "affine64") if w else bytes(64), 0 if w else H.NO_KEY))

    def mac():
        key, data = rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), rng.integers(0, 256, 37, dtype=np.uint8).tobytes()
        out.append((2, key, data[:32], data[32:] + bytes(27), hmac.new(key, data, hashlib.sha512).digest(), 0))

    for _ in range(8):
        kp = rnd() % (N - 1) + 1
        for il in (N - 1, N, N + 1, 2**256 - 1, N - kp, (N - kp + 1) % N, N - kp - 1):
            priv(il, kp)
        for il in (N - 1, N, N + 1, 2**256 - 1, N - kp, kp, 1):          # N - kp: IL G = -K_par; kp: the doubling
            pub(il, kp)
    while len(out) < 4 * 64 + 17:
        (priv, pub)[len(out) & 1](rnd() % N, rnd() % (N - 1) + 1) if len(out) % 3 else mac()
    order = rng.permutation(len(out))                                      # shuffled placement
    out = [out[j] for j in order]
    for b in range(0, len(out) - 63, 64):                                  # every whole wavefront holds failing lanes of both tweaks, good lanes of both, and HMAC lanes
        wave = out[b:b + 64]
        assert all(any(c[0] == kind and (c[5] != 0) == bad for c in wave) for kind in (0, 1) for bad in (False, True)) and any(c[0] == 2 for c in wave)
    return out


def test_tweaks_with_chosen_IL_on_the_gpu():
    assert SO.exists(), f"{SO} is missing: run __graft_entry__.build() (make -C tests/hd_gpu)"
    import torch  # noqa: F401  (torch ships its own HIP runtime: whichever copy loads first serves the process, and loading the system's first leaves torch without a device)
    lib = C.CDLL(str(SO))
    lib.hg_last_error.restype = C.c_char_p
    cases = _cases()
    n = len(cases)
    kind = np.array([c[0] for c in cases], np.uint8)
    a, b, c = (np.frombuffer(b"".join(x[j] for x in cases), np.uint8).copy() for j in (1, 2, 3))
    out, status = np.full(64 * n, 0xAA, np.uint8), np.full(n, 0xAAAAAAAA, np.uint32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = lib.hg_tweaks(C.c_uint32(n), p(kind), p(a), p(b), p(c), p(out), p(status))
    assert rc == 0, (lib.hg_last_error() or b"").decode()
    got = out.reshape(n, 64)
    for i, x in enumerate(cases):
        assert (got[i].tobytes(), int(status[i])) == (x[4], x[5]), (i, x[0], x[1].hex(), x[2].hex())
    assert sum(1 for x in cases if x[5] == H.NO_KEY) >= 8 * 8 and all(x[4] == bytes(64) for x in cases if x[5])
