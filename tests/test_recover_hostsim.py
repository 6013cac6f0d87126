"""plume_recover_batch* on the host side (capi_recover / capi_recover_device in csrc/plume_capi.hip, csrc/plume_recover_capi.hip) under the sanitizers, on the CPU: the
unchanged objects of the existing host-side harness (tests/hostsim/Makefile: plume_capi.hip against the mock HIP runtime, the other kernels as host loops, the C oracle)
linked with the ABI's translation unit, k_recover_finalize as a host loop (tests/hostsim/recover_launch.cpp) and a driver (tests/hostsim/recover_driver.cpp) that pins
every output to the C oracle (oracle_point_mul, oracle_hash_to_curve_batch, oracle_verify_batch) on fuzzed batches with the r = 0 signature planted: host form, device
form, a multi-device context over eight mock devices, two lanes in flight, sub_batches = 2, the three formats, every subset of NULL outputs.  ASan + UBSan and TSan,
lazy, random and eager schedulers.  Two mutants of the launcher must each fail the driver: one that writes points for rejected items, one that hashes the wrong version."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "zk-nullifier-sig_amd" / "csrc"
HOSTSIM = ROOT / "tests" / "hostsim"
FLAGS = ["-std=c++17", "-g", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off", "-DPLUME_GW=16", "-DPLUME_COMB_W=10", f"-I{HOSTSIM / 'mockhip'}", f"-I{CSRC}"]


def _san_flags(san):
    return [f"-fsanitize={san}", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if san else []


def _build(out, san, launch_defs=()):
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("no g++ / make")
    out.mkdir(parents=True, exist_ok=True)
    subprocess.run(["make", "-C", str(HOSTSIM), f"OUT={out}", f"SAN={san}", "-j2", str(out / "capi.o"), str(out / "launch.o"), str(out / "oracle.o")],
                   check=True, capture_output=True, text=True, timeout=1200)
    flags = FLAGS + _san_flags(san)
    units = [(["-x", "c++", "-O1", "-Werror"], CSRC / "plume_recover_capi.hip", "rcapi.o"), (["-O2", "-Werror", *launch_defs], HOSTSIM / "recover_launch.cpp", "rlaunch.o"),
             (["-O1", "-Werror"], HOSTSIM / "recover_driver.cpp", "rdriver.o")]
    for extra, src, obj in units:
        subprocess.run(["g++", *extra, *flags, "-c", str(src), "-o", str(out / obj)], check=True, capture_output=True, text=True, timeout=600)
    exe = out / "recover_driver"
    subprocess.run(["g++", *_san_flags(san), "-o", str(exe), *[str(out / o) for o in ("capi.o", "launch.o", "oracle.o", "rcapi.o", "rlaunch.o", "rdriver.o")], "-lpthread"],
                   check=True, capture_output=True, text=True, timeout=600)
    return exe


def _run(exe, seed, sched):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")
    for k in ("PLUME_MOCK_SCHED", "PLUME_SUB_BATCHES", "PLUME_SERIAL", "PLUME_STAGE_TIMES", "PLUME_MSM_PAIR_MAX", "PLUME_INGEST_SPLIT_MAX"):
        env.pop(k, None)
    if sched:
        env["PLUME_MOCK_SCHED"] = sched
    return subprocess.run([str(exe), str(seed)], capture_output=True, text=True, timeout=900, env=env)


def _ok(r, seed):
    assert r.returncode == 0, (seed, r.stdout[-2000:], r.stderr[-4000:])
    assert f"recover_driver seed {seed}: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "WARNING: ThreadSanitizer" not in r.stderr


@pytest.mark.parametrize("san,runs", [("address,undefined", [(1, None), (2, "random:2"), (3, "eager")]), ("thread", [(4, "random:4")])])
def test_recover_host_side_under_sanitizers(tmp_path, san, runs):
    exe = _build(tmp_path / "b", san)
    for seed, sched in runs:
        _ok(_run(exe, seed, sched), seed)


def test_the_driver_fails_when_points_are_written_for_rejected_items(tmp_path):
    r = _run(_build(tmp_path / "b", "", launch_defs=["-DRECOVER_MUTANT_WRITES_REJECTED"]), 1, None)
    assert r.returncode != 0 and "recover_driver:" in r.stderr and "PLUME_RECOVER_INVALID" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])


def test_the_driver_fails_when_the_wrong_version_is_hashed(tmp_path):
    r = _run(_build(tmp_path / "b", "", launch_defs=["-DRECOVER_MUTANT_WRONG_VERSION"]), 1, None)
    assert r.returncode != 0 and "recover_driver:" in r.stderr and "PLUME_RECOVER_MATCH" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])
