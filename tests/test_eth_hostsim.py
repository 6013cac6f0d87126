"""plume_eth_address_batch* on the host side (csrc/plume_eth_capi.hip) under the sanitizers, on the
CPU: the unchanged objects of the existing host-side harness (tests/hostsim/Makefile: plume_capi.hip against the mock HIP runtime, the other kernels as host loops, the C
oracle) linked with the ABI's translation unit, k_eth_address as a host loop (tests/hostsim/eth_launch.cpp) and a driver (tests/hostsim/eth_driver.cpp) that pins every
output to vectors this test writes from the Python restatement (tests/_keccak.py): the host form with chunks smaller than n, plume_init_multi contexts over three and
eight mock devices, the device form on a caller stream (nothing runs before the caller synchronises), two calls back to back on one stream, every allocation of a call
failing in turn, no table built.  ASan + UBSan and TSan, lazy, random and eager schedulers.  One mutant of the launcher, which drops its stream argument, must fail the
driver."""
import os
import shutil
import struct
import subprocess
from pathlib import Path

import pytest

from tests import _keccak as K

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
    units = [(["-x", "c++", "-O1", "-Werror"], CSRC / "plume_eth_capi.hip", "ecapi.o"), (["-O2", "-Werror", *launch_defs], HOSTSIM / "eth_launch.cpp", "elaunch.o"),
             (["-O1", "-Werror"], HOSTSIM / "eth_driver.cpp", "edriver.o")]
    for extra, src, obj in units:
        subprocess.run(["g++", *extra, *flags, "-c", str(src), "-o", str(out / obj)], check=True, capture_output=True, text=True, timeout=600)
    exe = out / "eth_driver"
    subprocess.run(["g++", *_san_flags(san), "-o", str(exe), *[str(out / o) for o in ("capi.o", "launch.o", "oracle.o", "ecapi.o", "elaunch.o", "edriver.o")], "-lpthread"],
                   check=True, capture_output=True, text=True, timeout=600)
    return exe


@pytest.fixture(scope="module")
def vectors(tmp_path_factory):
    """per key format: 64 keys with every invalid kind planted (first, last and in between), status, raw address, EIP-55 record -- from the restatement, once"""
    blob = b""
    for fmt in ("affine64", "sec1"):
        bad = [rec for _, rec in K.invalid_keys(fmt)]
        keys = [k.tobytes() for k in K.sample_keys(64 - len(bad), 21 if fmt == "sec1" else 20, fmt)]
        for j, rec in enumerate(bad):
            keys.insert(0 if j == 0 else len(keys) if j == 1 else 9 * j, rec)
        raw, st = K.eth_address_batch(b"".join(keys), None, fmt, "raw20")
        eip, st2 = K.eth_address_batch(b"".join(keys), None, fmt, "eip55")
        assert list(st) == list(st2) and int((st == K.INVALID).sum()) == len(bad) and st[0] == st[-1] == K.INVALID
        blob += struct.pack("<I", len(keys)) + b"".join(keys) + st.tobytes() + raw.tobytes() + eip.tobytes()
    path = tmp_path_factory.mktemp("eth_vectors") / "vectors.bin"
    path.write_bytes(blob)
    return path


def _run(exe, vectors, seed, sched):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")
    for k in ("PLUME_MOCK_SCHED", "PLUME_SUB_BATCHES", "PLUME_SERIAL", "PLUME_STAGE_TIMES", "PLUME_MSM_PAIR_MAX", "PLUME_INGEST_SPLIT_MAX"):
        env.pop(k, None)
    if sched:
        env["PLUME_MOCK_SCHED"] = sched
    return subprocess.run([str(exe), str(vectors), str(seed)], capture_output=True, text=True, timeout=900, env=env)


def _ok(r, seed):
    assert r.returncode == 0, (seed, r.stdout[-2000:], r.stderr[-4000:])
    assert f"eth_driver seed {seed}: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "WARNING: ThreadSanitizer" not in r.stderr


@pytest.mark.parametrize("san,runs", [("address,undefined", [(1, None), (2, "random:2"), (3, "eager")]), ("thread", [(4, "random:4")])])
def test_eth_address_host_side_under_sanitizers(tmp_path, vectors, san, runs):
    exe = _build(tmp_path / "b", san)
    for seed, sched in runs:
        _ok(_run(exe, vectors, seed, sched), seed)


def test_the_driver_fails_when_the_launcher_drops_its_stream(tmp_path, vectors):
    r = _run(_build(tmp_path / "b", "", launch_defs=["-DETH_MUTANT_DROPS_STREAM"]), vectors, 1, None)
    assert r.returncode != 0 and "eth_driver:" in r.stderr and "one device, host form" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])
