"""The façades of the point recovery on the MI355X: PlumeSignature.recover_v1specific and circuit_outputs (zk-nullifier-sig_amd/plume.py) against the reference's fixed
vector, and PlumeSignature::recover_v1specific of include/plume.hpp through tests/abi_cpp/recover_test.cpp."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def eng():
    import zk_nullifier_sig_amd as plume
    e = plume.Engine(0)
    yield e
    e.close()


def _vector_signature(plume, k, ver, with_v1=False):
    pt = lambda name: plume.AffinePoint.from_bytes64(bytes.fromhex(k[name + "_x"]) + bytes.fromhex(k[name + "_y"]))  # noqa: E731
    sc = lambda name: plume.NonZeroScalar.from_repr(bytes.fromhex(k[name]))  # noqa: E731
    v1 = plume.PlumeSignatureV1Fields(pt("g_r"), pt("h_r")) if with_v1 else None
    return plume.PlumeSignature(k["msg_utf8"].encode(), pt("pk"), pt("nullifier"), sc(f"c_v{ver}"), sc(f"s_v{ver}"), v1)


def test_recover_v1specific_upgrades_the_compact_record(eng, kats):
    import zk_nullifier_sig_amd as plume
    k = kats["plume_vector"]
    sig = _vector_signature(plume, k, 1)
    assert not sig.verify(eng)                                           # four fields only: read as a V2 record, whose hash c is not
    f = sig.recover_v1specific(eng)
    assert f.r_point.to_bytes64() == bytes.fromhex(k["g_r_x"] + k["g_r_y"]) and f.hashed_to_curve_r.to_bytes64() == bytes.fromhex(k["h_r_x"] + k["h_r_y"])
    sig.v1specific = f
    assert sig.verify(eng)
    with pytest.raises(plume.SignatureError, match="not the V1 hash"):    # status 0 is never silent: a V2 signature has no V1 fields to recover
        _vector_signature(plume, k, 2).recover_v1specific(eng)
    bad = _vector_signature(plume, k, 1)
    object.__setattr__(bad.nullifier, "y", bad.nullifier.y ^ 1)           # off the curve: the constructor would refuse it, the library must
    with pytest.raises(plume.SignatureError, match="no value"):
        bad.recover_v1specific(eng)


@pytest.mark.parametrize("ver", [1, 2])
def test_circuit_outputs_are_the_vector_in_registers(eng, kats, ver):
    import zk_nullifier_sig_amd as plume
    k = kats["plume_vector"]
    out = plume.circuit_outputs(_vector_signature(plume, k, ver, with_v1=ver == 1), eng)
    reg = lambda h: [int(h[48 - 16 * j:64 - 16 * j], 16) for j in range(4)]  # noqa: E731  (circuits/circom/utils.ts:11-17: four 64-bit registers, least significant first)
    assert out == {"r_point": [reg(k["g_r_x"]), reg(k["g_r_y"])], "hashed_to_curve_r": [reg(k["h_r_x"]), reg(k["h_r_y"])], "hashed_to_curve": [reg(k["h_x"]), reg(k["h_y"])]}
    inputs = plume.circuit_inputs(_vector_signature(plume, k, ver, with_v1=ver == 1), eng)
    assert inputs["pk"] == [reg(k["pk_x"]), reg(k["pk_y"])]               # the same register convention as the inputs


def test_cpp_facade(tmp_path):
    import zk_nullifier_sig_amd as plume
    exe = tmp_path / "recover_test"
    libdir = plume.library_path().parent
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"), str(ROOT / "tests" / "abi_cpp" / "recover_test.cpp"), "-L", str(libdir),
                    "-lplume_hip", f"-Wl,-rpath,{libdir}", "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "recover_test ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
