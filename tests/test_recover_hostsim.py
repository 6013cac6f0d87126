"""plume_recover_batch* on the host side (capi_recover / capi_recover_device in csrc/plume_capi.hip, csrc/plume_recover_capi.hip) under the sanitizers, on the CPU
(tests/_hostsim.py): the ABI's translation unit, k_recover_finalize as a host loop (tests/hostsim/recover_launch.cpp) and a driver (tests/hostsim/recover_driver.cpp) that pins
every output to the C oracle (oracle_point_mul, oracle_hash_to_curve_batch, oracle_verify_batch) on fuzzed batches with the r = 0 signature planted: host form, device
form, a multi-device context over eight mock devices, two lanes in flight, sub_batches = 2, the three formats, every subset of NULL outputs.  ASan + UBSan and TSan,
lazy, random and eager schedulers.  Two mutants of the launcher must each fail the driver: one that writes points for rejected items, one that hashes the wrong version."""
import pytest

from tests import _hostsim as H

UNITS = dict(driver="recover_driver", capi=["plume_recover_capi.hip"], launch=["recover_launch.cpp"])


@pytest.mark.parametrize("san,runs", H.RUNS)
def test_recover_host_side_under_sanitizers(tmp_path, san, runs):
    exe = H.build(tmp_path / "b", san, **UNITS)
    for seed, sched in runs:
        H.ok(H.run(exe, seed, sched=sched), "recover_driver", seed)


def test_the_driver_fails_when_points_are_written_for_rejected_items(tmp_path):
    r = H.run(H.build(tmp_path / "b", "", **UNITS, defs={"recover_launch.cpp": ["-DRECOVER_MUTANT_WRITES_REJECTED"]}), 1)
    assert r.returncode != 0 and "recover_driver:" in r.stderr and "PLUME_RECOVER_INVALID" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])


def test_the_driver_fails_when_the_wrong_version_is_hashed(tmp_path):
    r = H.run(H.build(tmp_path / "b", "", **UNITS, defs={"recover_launch.cpp": ["-DRECOVER_MUTANT_WRONG_VERSION"]}), 1)
    assert r.returncode != 0 and "recover_driver:" in r.stderr and "PLUME_RECOVER_MATCH" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])
