"""The single-item forms of the key derivation in Python (zk-nullifier-sig_amd/plume.py: hd_master, hd_derive, hd_derive_pub, hd_address, parse_path, parse_xprv, parse_xpub)
and in C++ (include/plume.hpp, tests/abi_cpp/hd_test.cpp): BIP-32's test vector 1 and the Hardhat / Anvil accounts come out byte for byte, the public form agrees with the
private one, and the error each raises for a path that is none, a hardened index below a public key, a parent out of range and a string whose checksum fails."""
import subprocess
from pathlib import Path

import pytest

from tests import _ecdsa as E
from tests import _hd as H
from tests import _keccak as K

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
BAD_PATHS = ("m/", "m", "", "0//1", "/0", "2147483648", "2147483648'", "5'h", "1/2/3/4/5/6/7/8/9", "m/-1", "m/x", "m/1.0")


def _flip(s):
    """the string with one character replaced by the next base58 digit"""
    i = len(s) // 2
    return s[:i] + H._B58[(H._B58.index(s[i]) + 1) % 58] + s[i + 1:]


def test_python_facade():
    import zk_nullifier_sig_amd as plume
    eng = plume.Engine(0)
    try:
        assert plume.parse_path("m/44'/60h/0'/0/3") == [H.H + 44, H.H + 60, H.H, 0, 3] and plume.parse_path("0/3") == [0, 3] and plume.parse_path("m/0/1/2/3/4/5/6/7") == list(range(8))
        for bad in BAD_PATHS:
            with pytest.raises(ValueError):
                plume.parse_path(bad)
        # BIP-32 test vector 1: the strings decode to the values, the values derive one another
        m = plume.hd_master(H.V1_SEED, eng)
        assert (m[0].hex(), m[1].hex()) == H.V1["m"][:2]
        for depth, (path, (sk, chain, xprv)) in enumerate(H.V1.items()):
            d, child, c, k = plume.parse_xprv(xprv)
            assert (d, c.hex(), k.hex()) == (depth, chain, sk) and child == (0, H.H, 1)[depth]
            if depth:
                assert tuple(b.hex() for b in plume.hd_derive(m[0], m[1], path, eng)) == (sk, chain)
                assert tuple(b.hex() for b in plume.hd_derive(plume.SecretKey.from_bytes(m[0]), m[1], H.parse_path(path), eng)) == (sk, chain)
            with pytest.raises(ValueError):
                plume.parse_xprv(_flip(xprv))
            with pytest.raises(ValueError):
                plume.parse_xpub(xprv)
        for bad in ("", "xprv", H.V1["m"][2][:-1], H.V1["m"][2] + "1", H.V1["m"][2].replace("K", "0", 1), H.V1["m"][2].replace("K", "l", 1)):
            with pytest.raises(ValueError):
                plume.parse_xprv(bad)
        # CKDpub from (m/0') G with index 1 gives (m/0'/1) G and the same chain
        k0, c0 = bytes.fromhex(H.V1["m/0'"][0]), bytes.fromhex(H.V1["m/0'"][1])
        P0 = H.g_mul(int.from_bytes(k0, "big"))
        pk, chain = plume.hd_derive_pub(plume.AffinePoint(*P0), c0, "1", eng)
        want = H.g_mul(int(H.V1["m/0'/1"][0], 16))
        assert (pk.x, pk.y) == want and chain.hex() == H.V1["m/0'/1"][1]
        pk33, chain33 = plume.hd_derive_pub(H.ser_p(P0), c0, "1", eng)
        assert (pk33.x, pk33.y) == want and chain33 == chain and plume.hd_derive_pub(E.pk_record(P0, "affine64"), c0, [1], eng)[0] == pk
        # the Hardhat / Anvil accounts, from the seed and from the account node's public key
        seed = H.hardhat_seed()
        ms, mc = plume.hd_master(seed, eng)
        ask, ac = plume.hd_derive(ms, mc, H.HARDHAT_ACCOUNT_PATH, eng)
        assert (ask.hex(), ac.hex()) == H.HARDHAT_ACCOUNT
        A = plume.AffinePoint(*H.g_mul(int.from_bytes(ask, "big")))
        for i, (sk, addr) in enumerate(H.HARDHAT_CHILDREN):
            assert plume.hd_derive(ms, mc, f"{H.HARDHAT_ACCOUNT_PATH}/{i}", eng)[0].hex() == sk
            assert plume.hd_address(ms, mc, f"{H.HARDHAT_ACCOUNT_PATH}/{i}", eng).hex() == addr == plume.hd_address(A, ac, str(i), eng).hex() == plume.hd_address(H.ser_p((A.x, A.y)), ac, [i], eng).hex()
        # the errors
        with pytest.raises(plume.SignatureError, match="hardened"):
            plume.hd_derive_pub(A, ac, "0'", eng)
        with pytest.raises(plume.SignatureError, match="hardened"):
            plume.hd_address(A, ac, "0/1h", eng)
        for k in (0, E.N):
            with pytest.raises(plume.SignatureError, match="status 2"):
                plume.hd_derive(E.b32(k), ac, "0", eng)
        with pytest.raises(plume.SignatureError, match="status 2"):
            plume.hd_derive_pub(bytes(64), ac, "0", eng)
        for bad in (b"", bytes(15), bytes(65)):
            with pytest.raises(ValueError):
                plume.hd_master(bad, eng)
        with pytest.raises(ValueError):
            plume.hd_derive(bytes(31), ac, "0", eng)
        with pytest.raises(ValueError):
            plume.hd_derive(ask, ac, "m/", eng)

        class NoKey:                                                         # the façade's own mapping of a status no test can provoke, on a stand-in engine that reports it
            def hd_derive_priv_batch(self, *a, **k):
                import numpy as np
                return {"sk": np.zeros((1, 32), np.uint8), "chain": np.zeros((1, 32), np.uint8), "status": np.array([32], np.uint8)}
        with pytest.raises(plume.SignatureError, match="no key"):
            plume.hd_derive(ask, ac, "0", NoKey())
    finally:
        eng.close()


def test_cpp_facade(tmp_path):
    import zk_nullifier_sig_amd as plume
    rows = [("master", H.V1_SEED.hex(), *H.V1["m"][:2])]
    seed = H.hardhat_seed()
    m = H.master(seed)
    rows.append(("master", seed.hex(), H.b32(m[0]).hex(), m[1].hex()))
    m1 = H.master(H.V1_SEED)
    for path in ("m/0'", "m/0'/1", "0h/1"):
        k, c = H.derive(m1[0], m1[1], path)
        rows.append(("priv", H.V1["m"][0], H.V1["m"][1], path, H.b32(k).hex(), c.hex(), K.address_of(H.g_mul(k)).hex()))
    for i, (sk, addr) in enumerate(H.HARDHAT_CHILDREN):
        k, c = H.derive(m[0], m[1], f"{H.HARDHAT_ACCOUNT_PATH}/{i}")
        rows.append(("priv", H.b32(m[0]).hex(), m[1].hex(), f"{H.HARDHAT_ACCOUNT_PATH}/{i}", sk, c.hex(), addr))
        A = H.g_mul(int(H.HARDHAT_ACCOUNT[0], 16))
        Kc, cc = H.ckd_pub(A, bytes.fromhex(H.HARDHAT_ACCOUNT[1]), i)
        rows.append(("pub", E.pk_record(A, "affine64").hex(), H.HARDHAT_ACCOUNT[1], str(i), E.pk_record(Kc, "affine64").hex(), cc.hex(), addr))
    for depth, (sk, chain, xprv) in enumerate(H.V1.values()):
        rows.append(("xprv", xprv, str(depth), str((0, H.H, 1)[depth]), chain, sk))
        rows.append(("badx", _flip(xprv)))
    rows += [("badpath", p) for p in BAD_PATHS if p] + [("badx", "xprv"), ("badx", H.V1["m"][2] + "1")]
    vectors = tmp_path / "vectors.txt"
    vectors.write_text("".join(" ".join(r) + "\n" for r in rows))
    exe = tmp_path / "hd_test"
    libdir = plume.library_path().parent
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"), str(ROOT / "tests" / "abi_cpp" / "hd_test.cpp"), "-L", str(libdir),
                    "-lplume_hip", f"-Wl,-rpath,{libdir}", "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe), str(vectors)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "hd_test ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
