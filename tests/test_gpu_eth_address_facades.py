"""The façades of the Ethereum-address call on the MI355X: PlumeSignature.eth_address, eth_address_eip55 and verify_for_address (zk-nullifier-sig_amd/plume.py) on the
reference's fixed vector and on golden V1 and V2 records, the allow-list gate end to end (64-byte address records in Engine.nullifier_set(), then contains), and the same
three methods of include/plume.hpp through tests/abi_cpp/eth_address_test.cpp.  Expected addresses come from the restatement of tests/_keccak.py."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import _keccak as K

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLD = json.loads((ROOT / "tests" / "golden" / "golden_batches.json").read_text())


@pytest.fixture(scope="module")
def eng():
    import zk_nullifier_sig_amd as plume
    e = plume.Engine(0)
    yield e
    e.close()


def _vector_signature(plume, k, ver):
    pt = lambda name: plume.AffinePoint.from_bytes64(bytes.fromhex(k[name + "_x"]) + bytes.fromhex(k[name + "_y"]))  # noqa: E731
    sc = lambda name: plume.NonZeroScalar.from_repr(bytes.fromhex(k[name]))  # noqa: E731
    v1 = plume.PlumeSignatureV1Fields(pt("g_r"), pt("h_r")) if ver == 1 else None
    return plume.PlumeSignature(k["msg_utf8"].encode(), pt("pk"), pt("nullifier"), sc(f"c_v{ver}"), sc(f"s_v{ver}"), v1)


def _golden_signature(plume, it, ver):
    pt = lambda name: plume.AffinePoint.from_bytes64(bytes.fromhex(it[name]))  # noqa: E731
    sc = lambda name: plume.NonZeroScalar.from_repr(bytes.fromhex(it[name]))  # noqa: E731
    v1 = plume.PlumeSignatureV1Fields(pt("r_point"), pt("hashed_to_curve_r")) if ver == 1 else None
    return plume.PlumeSignature(bytes.fromhex(it["msg"]), pt("pk"), pt("nullifier"), sc("c"), sc("s"), v1)


def _check(plume, eng, sig, other_s):
    want = K.address_of(K.decode_pk(sig.pk.to_bytes64()))
    assert sig.eth_address(eng) == want and sig.eth_address_eip55(eng) == K.eip55(want)
    assert sig.verify(eng) and sig.verify_for_address(want, eng)
    for bit in (0, 77, 159):                                          # one flipped bit of the address
        other = bytearray(want)
        other[bit // 8] ^= 1 << (bit % 8)
        assert not sig.verify_for_address(bytes(other), eng)
    bad = plume.PlumeSignature(sig.message, sig.pk, sig.nullifier, sig.c, other_s, sig.v1specific)
    assert not bad.verify(eng) and not bad.verify_for_address(want, eng)                  # the right address, a corrupted s
    assert bad.eth_address(eng) == want
    with pytest.raises(ValueError):
        sig.verify_for_address(want + b"\0", eng)


@pytest.mark.parametrize("ver", [1, 2])
def test_reference_vector(eng, kats, ver):
    import zk_nullifier_sig_amd as plume
    k = kats["plume_vector"]
    _check(plume, eng, _vector_signature(plume, k, ver), plume.NonZeroScalar.from_repr(bytes.fromhex(k[f"s_v{3 - ver}"])))


@pytest.mark.parametrize("ver", [1, 2])
def test_golden_record(eng, ver):
    import zk_nullifier_sig_amd as plume
    items = GOLD[f"sign_v{ver}"]
    _check(plume, eng, _golden_signature(plume, items[3], ver), plume.NonZeroScalar.from_repr(bytes.fromhex(items[4]["s"])))


def test_a_pk_that_is_no_ethereum_key(eng, kats):
    import zk_nullifier_sig_amd as plume
    sig = _vector_signature(plume, kats["plume_vector"], 2)
    want = sig.eth_address(eng)
    object.__setattr__(sig.pk, "y", sig.pk.y ^ 1)                       # off the curve: the constructor would refuse it, the library must
    with pytest.raises(plume.SignatureError, match="non-identity curve point"):
        sig.eth_address(eng)
    with pytest.raises(plume.SignatureError, match="non-identity curve point"):
        sig.eth_address_eip55(eng)
    assert not sig.verify_for_address(want, eng)


def test_allow_list_gate_end_to_end(eng):
    """the example of DESIGN.md: the list is a nullifier set of 64-byte address records; a claim passes when its signature verifies and its key's record is in the set"""
    import zk_nullifier_sig_amd as plume
    items = GOLD["sign_v2"]
    pk = np.frombuffer(b"".join(bytes.fromhex(it["pk"]) for it in items), np.uint8).reshape(-1, 64)
    assert len(np.unique(pk, axis=0)) == len(pk) >= 32
    listed = np.arange(len(pk)) % 3 != 0
    records, status = eng.eth_address_batch(pk, addr_format="record64")
    assert (status == plume.ETH_MATCH).all()
    for i in (0, 1, len(pk) - 1):
        assert records[i].tobytes() == bytes(44) + K.address_of(K.decode_pk(pk[i].tobytes()))
    with eng.nullifier_set() as allow:
        fresh, n_fresh = allow.insert(records[listed])
        assert n_fresh == int(listed.sum()) and fresh.all() and len(allow) == n_fresh
        # the gate, for a batch of claims: every public key's record, then one lookup; an invalid key writes the zero record, which is not on the list
        claims = pk.copy()
        claims[5] = 0
        recs, st = eng.eth_address_batch(claims, addr_format="record64")
        found = allow.contains(recs)
        want = listed.copy()
        want[5] = False
        assert st[5] == plume.ETH_INVALID and np.array_equal(found.astype(bool), want)
        sig = _golden_signature(plume, items[1], 2)
        assert listed[1] and sig.verify(eng) and allow.contains(np.frombuffer(bytes(44) + sig.eth_address(eng), np.uint8))[0] == 1


def test_cpp_facade(tmp_path):
    import zk_nullifier_sig_amd as plume
    exe = tmp_path / "eth_address_test"
    libdir = plume.library_path().parent
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"), str(ROOT / "tests" / "abi_cpp" / "eth_address_test.cpp"), "-L", str(libdir),
                    "-lplume_hip", f"-Wl,-rpath,{libdir}", "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "eth_address_test ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
