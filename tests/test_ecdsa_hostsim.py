"""plume_ecdsa_recover_batch* on the host side (csrc/plume_ecdsa_capi.hip) under the sanitizers, on
the CPU: the unchanged objects of the existing host-side harness (tests/hostsim/Makefile: plume_capi.hip against the mock HIP runtime, the other kernels as host loops, the
C oracle) linked with the ABI's translation unit, the three kernels as host loops (tests/hostsim/ecdsa_launch.cpp) and a driver (tests/hostsim/ecdsa_driver.cpp) that
pins every output to vectors this test writes from the Python restatement (tests/_ecdsa.py) over the OpenSSL and crafted items of
tests/golden/ecdsa_recover_kats.json: the host form with chunks of 1, 64 and n, a plume_init_multi context over eight mock devices, the device form on caller streams
(nothing runs before the caller synchronises), sub-batches, argument errors, every allocation of a call failing in turn.  ASan + UBSan and TSan, lazy, random and eager
schedulers.  One mutant of a launcher, which drops its stream argument, must fail the driver."""
import os
import shutil
import struct
import subprocess
from pathlib import Path

import pytest

from tests import _ecdsa as E

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
    units = [(["-x", "c++", "-O1", "-Werror"], CSRC / "plume_ecdsa_capi.hip", "kcapi.o"), (["-O2", "-Werror", *launch_defs], HOSTSIM / "ecdsa_launch.cpp", "klaunch.o"),
             (["-O1", "-Werror"], HOSTSIM / "ecdsa_driver.cpp", "kdriver.o")]
    for extra, src, obj in units:
        subprocess.run(["g++", *extra, *flags, "-c", str(src), "-o", str(out / obj)], check=True, capture_output=True, text=True, timeout=600)
    exe = out / "ecdsa_driver"
    subprocess.run(["g++", *_san_flags(san), "-o", str(exe), *[str(out / o) for o in ("capi.o", "launch.o", "oracle.o", "kcapi.o", "klaunch.o", "kdriver.o")], "-lpthread"],
                   check=True, capture_output=True, text=True, timeout=600)
    return exe


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


def _run(exe, vectors, seed, sched):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")
    for k in ("PLUME_MOCK_SCHED", "PLUME_SUB_BATCHES", "PLUME_SERIAL", "PLUME_STAGE_TIMES", "PLUME_MSM_PAIR_MAX", "PLUME_INGEST_SPLIT_MAX", "PLUME_OVERLAP_MIN"):
        env.pop(k, None)
    if sched:
        env["PLUME_MOCK_SCHED"] = sched
    return subprocess.run([str(exe), str(vectors), str(seed)], capture_output=True, text=True, timeout=1500, env=env)


def _ok(r, seed):
    assert r.returncode == 0, (seed, r.stdout[-2000:], r.stderr[-4000:])
    assert f"ecdsa_driver seed {seed}: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "WARNING: ThreadSanitizer" not in r.stderr


@pytest.mark.parametrize("san,runs", [("address,undefined", [(1, None), (2, "random:2"), (3, "eager")]), ("thread", [(4, "random:4")])])
def test_ecdsa_recover_host_side_under_sanitizers(tmp_path, vectors, san, runs):
    exe = _build(tmp_path / "b", san)
    for seed, sched in runs:
        _ok(_run(exe, vectors, seed, sched), seed)


def test_the_driver_fails_when_a_launcher_drops_its_stream(tmp_path, vectors):
    r = _run(_build(tmp_path / "b", "", launch_defs=["-DECDSA_MUTANT_DROPS_STREAM"]), vectors, 1, None)
    assert r.returncode != 0 and "ecdsa_driver:" in r.stderr and "one device, host form" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])
