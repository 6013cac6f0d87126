"""The single-item form of the transaction signer, sign_tx, in Python (zk-nullifier-sig_amd/plume.py) and in C++ (include/plume.hpp, tests/abi_cpp/eth_tx_sign_test.cpp):
EIP-155's worked example and one item of each kind from the committed fixture come out byte for byte, tx_sender(sign_tx(sk, u)) is the key's address, and the error each
raises for an ill-framed item, a key out of range and a withheld signature."""
import subprocess
from pathlib import Path

import pytest

from tests import _ecdsa as E
from tests import _eth_tx as T
from tests import _eth_tx_sign as X

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def _picked():
    """(EIP-155's example and one signed item of each kind as (sk, unsigned, raw); a few ill-framed items of different rules)"""
    kats = T.load_kats()
    kinds = {}
    for e in kats["items"]:
        if e["status"] == T.OK and e["sk"] and not e["high_s"]:
            kinds.setdefault((e["tx_type"], e["tx_type"] != 0 or e["chain_id"] != "0"), e)       # legacy unprotected, legacy EIP-155, 01 - 04
    assert len(kinds) == 6
    ex = kats["eip155"]
    valid = [(bytes.fromhex(ex["sk"]), bytes.fromhex(ex["signing_data"]), bytes.fromhex(ex["raw"]))]
    valid += [(bytes.fromhex(e["sk"]), X.unsigned_of(bytes.fromhex(e["raw"])), bytes.fromhex(e["raw"])) for e in kinds.values()]
    invalid = [bytes.fromhex(e["unsigned"]) for e in X.load_kats()["items"] if e["status"] == X.BAD_TX][::5]
    assert len(invalid) >= 6 and b"" in [bytes.fromhex(e["unsigned"]) for e in X.load_kats()["items"]]
    return valid, invalid + [b""]


def test_python_facade():
    import zk_nullifier_sig_amd as plume
    eng = plume.Engine(0)
    try:
        valid, invalid = _picked()
        for sk, u, raw in valid:
            got = plume.sign_tx(sk, u, engine=eng)
            assert got == raw
            assert plume.tx_sender(got, eng)[1] == T.sender_of(sk)[1] and plume.tx_signing_hash(got, eng) == X.sign_tx(u, sk)[1]
            assert plume.sign_tx(plume.SecretKey.from_bytes(sk), u, engine=eng) == raw
            hedged = plume.sign_tx(sk, u, aux=bytes(range(32)), engine=eng)
            assert hedged == X.sign_tx(u, sk, bytes(range(32)))[0] != raw and plume.tx_sender_address(hedged, eng) == T.sender_of(sk)[1]
        for u in invalid:
            with pytest.raises(plume.SignatureError):
                plume.sign_tx(valid[0][0], u, engine=eng)
            with pytest.raises(plume.SignatureError):                                                # BAD_TX whatever the key is
                plume.sign_tx(bytes(32), u, engine=eng)
        for k in (0, E.N):                                                                           # a key out of range on a good item: the signer's own error
            with pytest.raises(plume.SignatureError, match="status 2"):
                plume.sign_tx(E.b32(k), valid[0][1], engine=eng)
        with pytest.raises(ValueError):
            plume.sign_tx(bytes(31), valid[0][1], engine=eng)
        eng.set_sign_selfcheck(1)                                                                     # the self-check on: the same bytes, the same errors
        try:
            assert plume.sign_tx(valid[0][0], valid[0][1], engine=eng) == valid[0][2]
            with pytest.raises(plume.SignatureError):
                plume.sign_tx(valid[0][0], invalid[0], engine=eng)
        finally:
            eng.set_sign_selfcheck(0)
        # the status of a withheld signature maps to PlumeSelfCheckError: the façade's own mapping, on a stand-in engine that reports it
        class Withheld:
            def eth_tx_sign_batch(self, unsigned, sk, aux=None, records=False):
                import numpy as np
                return [b""], np.array([8], np.uint8)
        with pytest.raises(plume.PlumeSelfCheckError):
            plume.sign_tx(valid[0][0], valid[0][1], engine=Withheld())
    finally:
        eng.close()


def test_cpp_facade(tmp_path):
    import zk_nullifier_sig_amd as plume
    valid, invalid = _picked()
    rows = [("ok", sk.hex(), u.hex(), raw.hex(), T.sender_of(sk)[1].hex()) for sk, u, raw in valid]
    rows += [("bad", valid[0][0].hex(), u.hex() or "-", "-", "-") for u in invalid]
    vectors = tmp_path / "vectors.txt"
    vectors.write_text("".join(" ".join(r) + "\n" for r in rows))
    exe = tmp_path / "eth_tx_sign_test"
    libdir = plume.library_path().parent
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"), str(ROOT / "tests" / "abi_cpp" / "eth_tx_sign_test.cpp"), "-L", str(libdir),
                    "-lplume_hip", f"-Wl,-rpath,{libdir}", "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe), str(vectors)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "eth_tx_sign_test ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
