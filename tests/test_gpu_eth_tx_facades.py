"""The single-item forms of the transaction calls, tx_signing_hash / tx_sender / tx_sender_address, in Python (zk-nullifier-sig_amd/plume.py) and in C++ (include/plume.hpp,
tests/abi_cpp/eth_tx_test.cpp): EIP-155's worked example and one item of each kind from the committed fixture, and the error each raises for an invalid transaction."""
import subprocess
from pathlib import Path

import pytest

from tests import _eth_tx as T
from tests import _keccak as K

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def _picked():
    """(valid items: one of each kind, signed; invalid items: a few of different rules; a framing-valid item whose signature recovers nothing)"""
    items = T.load_kats()["items"]
    kinds = {}
    for e in items:
        if e["status"] == T.OK and e["sk"] and not e["high_s"]:
            kinds.setdefault((e["tx_type"], e["tx_type"] != 0 or e["chain_id"] != "0"), e)       # legacy unprotected, legacy EIP-155, 01 - 04
    assert len(kinds) == 6
    invalid = [e for e in items if e["status"] == T.INVALID and e["raw"]][::9]
    rzero = next(e for e in items if e["status"] == T.OK and int(e["r"], 16) == 0)
    high = next(e for e in items if e["high_s"])
    return list(kinds.values()), invalid, rzero, high


def test_python_facades():
    import zk_nullifier_sig_amd as plume
    eng = plume.Engine(0)
    try:
        e155 = T.load_kats()["eip155"]
        raw = bytes.fromhex(e155["raw"])
        assert plume.tx_signing_hash(raw, eng).hex() == e155["hash"]
        pk, addr = plume.tx_sender(raw, eng)
        assert K.eip55(addr) in (e155["sender"], e155["sender"].encode()) and plume.tx_sender_address(raw, eng) == addr
        assert (pk.x, pk.y) == T.sender_of(bytes.fromhex(e155["sk"]))[0]
        valid, invalid, rzero, high = _picked()
        for e in valid:
            raw, (q, a) = bytes.fromhex(e["raw"]), T.sender_of(bytes.fromhex(e["sk"]))
            assert plume.tx_signing_hash(raw, eng).hex() == e["hash"], e["name"]
            pk, addr = plume.tx_sender(raw, eng)
            assert (pk.x, pk.y) == q and addr == a and plume.tx_sender_address(raw, eng) == a, e["name"]
        for e in invalid + [{"raw": "", "name": "empty"}]:
            for f in (plume.tx_signing_hash, plume.tx_sender, plume.tx_sender_address):
                with pytest.raises(plume.SignatureError):
                    f(bytes.fromhex(e["raw"]), eng)
        assert plume.tx_signing_hash(bytes.fromhex(rzero["raw"]), eng).hex() == rzero["hash"]       # the framing is fine; nothing recovers
        with pytest.raises(plume.SignatureError):
            plume.tx_sender(bytes.fromhex(rzero["raw"]), eng)
        with pytest.raises(plume.SignatureError):                                                    # a high s is no sender under the EIP-2 rule, and one without it
            plume.tx_sender_address(bytes.fromhex(high["raw"]), eng)
        assert plume.tx_sender_address(bytes.fromhex(high["raw"]), eng, low_s=False) == T.sender_of(bytes.fromhex(high["sk"]))[1]
    finally:
        eng.close()


def test_cpp_facade(tmp_path):
    import zk_nullifier_sig_amd as plume
    valid, invalid, rzero, high = _picked()
    e155 = T.load_kats()["eip155"]
    rows = [("ok", e155["raw"], e155["hash"], e155["sender"][2:].lower())]
    rows += [("ok", e["raw"], e["hash"], T.sender_of(bytes.fromhex(e["sk"]))[1].hex()) for e in valid]
    rows += [("bad", e["raw"], "-", "-") for e in invalid]
    rows += [("nosender", rzero["raw"], rzero["hash"], "-"), ("highs", high["raw"], high["hash"], T.sender_of(bytes.fromhex(high["sk"]))[1].hex())]
    vectors = tmp_path / "vectors.txt"
    vectors.write_text("".join(" ".join(r) + "\n" for r in rows))
    exe = tmp_path / "eth_tx_test"
    libdir = plume.library_path().parent
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"), str(ROOT / "tests" / "abi_cpp" / "eth_tx_test.cpp"), "-L", str(libdir),
                    "-lplume_hip", f"-Wl,-rpath,{libdir}", "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe), str(vectors)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "eth_tx_test ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
