"""plume_ecdsa_recover_batch* on the host side (csrc/plume_ecdsa_capi.hip) under the sanitizers, on the CPU (tests/_hostsim.py): the ABI's
translation unit, the three kernels as host loops (tests/hostsim/ecdsa_launch.cpp) and a driver (tests/hostsim/ecdsa_driver.cpp) that
pins every output to vectors this test writes from the Python restatement (tests/_ecdsa.py) over the OpenSSL and crafted items of
tests/golden/ecdsa_recover_kats.json: the host form with chunks of 1, 64 and n, a plume_init_multi context over eight mock devices, the device form on caller streams
(nothing runs before the caller synchronises), sub-batches, argument errors, every allocation of a call failing in turn.  ASan + UBSan and TSan, lazy, random and eager
schedulers.  One mutant of a launcher, which drops its stream argument, must fail the driver."""
import struct

import pytest

from tests import _ecdsa as E
from tests import _hostsim as H

UNITS = dict(driver="ecdsa_driver", capi=["plume_ecdsa_capi.hip"], launch=["ecdsa_launch.cpp"])


@pytest.fixture(scope="module")
def vectors(tmp_path_factory):
    """the OpenSSL items with the crafted ones planted among them (first, last and in between), and what the restatement says about them, once"""
    kats = E.load_kats()
    rows = [(bytes.fromhex(e["hash"]), bytes.fromhex(e["r"]), bytes.fromhex(e["s"]), e["v"]) for e in kats["openssl"]]
    for j, c in enumerate(kats["crafted"]):
        rows.insert(0 if j == 0 else len(rows) if j == 1 else (3 * j) % len(rows), (bytes.fromhex(c["hash"]), bytes.fromhex(c["r"]), bytes.fromhex(c["s"]), c["v"]))
    H, R, S = (b"".join(row[k] for row in rows) for k in range(3))
    V = bytes(row[3] for row in rows)
    pk, raw, st = E.recover_batch(H, R, S, V)
    _, eip, st2 = E.recover_batch(H, R, S, V, None, "affine64", "eip55")
    assert list(st) == list(st2) and st[0] == E.INVALID and 20 < int((st == E.INVALID).sum()) < len(rows) - 40
    path = tmp_path_factory.mktemp("ecdsa_vectors") / "vectors.bin"
    path.write_bytes(struct.pack("<I", len(rows)) + H + R + S + V + st.tobytes() + pk.tobytes() + raw.tobytes() + eip.tobytes())
    return path


@pytest.mark.parametrize("san,runs", H.RUNS)
def test_ecdsa_recover_host_side_under_sanitizers(tmp_path, vectors, san, runs):
    exe = H.build(tmp_path / "b", san, **UNITS)
    for seed, sched in runs:
        H.ok(H.run(exe, vectors, seed, sched=sched), "ecdsa_driver", seed)


def test_the_driver_fails_when_a_launcher_drops_its_stream(tmp_path, vectors):
    r = H.run(H.build(tmp_path / "b", "", **UNITS, defs={"ecdsa_launch.cpp": ["-DECDSA_MUTANT_DROPS_STREAM"]}), vectors, 1)
    assert r.returncode != 0 and "ecdsa_driver:" in r.stderr and "one device, host form" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])
