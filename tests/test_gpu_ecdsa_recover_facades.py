"""The façades of the ECDSA recovery on the MI355X: ecdsa_recover and ecdsa_recover_address of zk-nullifier-sig_amd/plume.py on OpenSSL's vectors
(tests/golden/ecdsa_recover_kats.json) and on the three invalid kinds (a field out of range, an r with no curve point, a key that comes out as the identity), the
anonymity-set flow of DESIGN.md end to end (signatures -> 64-byte address records -> Engine.nullifier_set(); the recovered pk -> the verifier), and the same two
functions of include/plume.hpp through tests/abi_cpp/ecdsa_recover_test.cpp.  Expected keys and addresses come from OpenSSL and the restatement of tests/_ecdsa.py."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import _ecdsa as E
from tests import _keccak as K

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
KATS = E.load_kats()
CRAFTED = {c["name"]: c for c in KATS["crafted"]}
INVALID_KINDS = ("r = 0, v = 0", "s = n, flags = 0", "v = 29", "r = n - 1, v = 1", "identity: R = k G, hash = s k")     # out of range x 3, no root, identity


@pytest.fixture(scope="module")
def eng():
    import zk_nullifier_sig_amd as plume
    e = plume.Engine(0)
    yield e
    e.close()


def _fields(e):
    return bytes.fromhex(e["hash"]), bytes.fromhex(e["r"]), bytes.fromhex(e["s"]), e["v"]


def test_genuine_signatures(eng):
    import zk_nullifier_sig_amd as plume
    for e in KATS["openssl"][:6]:
        pk, address = plume.ecdsa_recover(*_fields(e), eng)
        assert isinstance(pk, plume.AffinePoint) and pk.to_bytes64().hex() == e["pk"]
        assert address == K.address_of((pk.x, pk.y)) and plume.ecdsa_recover_address(*_fields(e), eng) == address
    c = CRAFTED["doubling: R = k G, hash = -s k"]
    pk, address = plume.ecdsa_recover(*_fields(c), eng)
    assert (pk.x, pk.y) == E.recover(bytes.fromhex(c["hash"]), int(c["r"], 16), int(c["s"], 16), c["v"])


@pytest.mark.parametrize("name", INVALID_KINDS)
def test_the_invalid_kinds_raise(eng, name):
    import zk_nullifier_sig_amd as plume
    c = CRAFTED[name]
    assert E.recover(bytes.fromhex(c["hash"]), int(c["r"], 16), int(c["s"], 16), c["v"]) is None
    with pytest.raises(plume.SignatureError, match="recovers no public key"):
        plume.ecdsa_recover(*_fields(c), eng)
    with pytest.raises(plume.SignatureError, match="recovers no public key"):
        plume.ecdsa_recover_address(*_fields(c), eng)


def test_malformed_arguments(eng):
    import zk_nullifier_sig_amd as plume
    h, r, s, v = _fields(KATS["openssl"][0])
    with pytest.raises(ValueError):
        plume.ecdsa_recover(h + b"\0", r, s, v, eng)
    with pytest.raises(ValueError):
        plume.ecdsa_recover_address(h, r, s, 256, eng)


def test_anonymity_set_flow_end_to_end(eng):
    """the listed accounts' signatures give the set's records; a claim's recovered key goes to the verifier and its record is looked up in the set"""
    import zk_nullifier_sig_amd as plume
    n = len(KATS["openssl"])
    a = lambda k: np.frombuffer(b"".join(bytes.fromhex(e[k]) for e in KATS["openssl"]), np.uint8).reshape(n, 32)  # noqa: E731
    v = np.array([e["v"] for e in KATS["openssl"]], np.uint8)
    pk, records, status = eng.ecdsa_recover_batch(a("hash"), a("r"), a("s"), v, addr_format="record64")
    assert (status == plume.ECDSA_MATCH).all() and pk.tobytes().hex() == "".join(e["pk"] for e in KATS["openssl"])
    listed = np.arange(n) % 3 != 0
    with eng.nullifier_set() as members:
        fresh, n_fresh = members.insert(records[listed])
        assert n_fresh == int(listed.sum()) and fresh.all()
        assert np.array_equal(members.contains(records).astype(bool), listed)
        # binding a claimed pk to an account: the claim's ECDSA signature must recover the claimed address
        claimed = records[:, 44:].copy()
        claimed[7, 0] ^= 0x80
        _, _, st = eng.ecdsa_recover_batch(a("hash"), a("r"), a("s"), v, expect=claimed, want=("status",))
        assert st[7] == plume.ECDSA_MISMATCH and (np.delete(st, 7) == plume.ECDSA_MATCH).all()
    addr2, st2 = eng.eth_address_batch(pk)                                                   # the recovered keys are keys every other call takes
    assert (st2 == plume.ETH_MATCH).all() and np.array_equal(addr2, records[:, 44:])


def test_cpp_facade(tmp_path):
    import zk_nullifier_sig_amd as plume
    lines = []
    for e in KATS["openssl"][:5]:
        pt = (int(e["pk"][:64], 16), int(e["pk"][64:], 16))
        lines.append(f'{e["hash"]} {e["r"]} {e["s"]} {e["v"]} {e["pk"]} {K.address_of(pt).hex()}')
    for name in INVALID_KINDS:
        c = CRAFTED[name]
        lines.append(f'{c["hash"]} {c["r"]} {c["s"]} {c["v"]} - -')
    vectors = tmp_path / "vectors.txt"
    vectors.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "ecdsa_recover_test"
    libdir = plume.library_path().parent
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"), str(ROOT / "tests" / "abi_cpp" / "ecdsa_recover_test.cpp"), "-L", str(libdir),
                    "-lplume_hip", f"-Wl,-rpath,{libdir}", "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe), str(vectors)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ecdsa_recover_test ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
