"""plume_ecdsa_sign_batch* and plume_eth_message_hash_batch* on the host side (csrc/plume_ecdsa_sign_capi.hip, csrc/plume_eth_hash_capi.hip) under the sanitizers, on the CPU: the unchanged objects of the existing host-side harness
(tests/hostsim/Makefile: plume_capi.hip against the mock HIP runtime, the other kernels as host loops, the C oracle) linked with the two ABI translation units, the self-check's switch
(csrc/plume_selfcheck_capi.hip, tests/hostsim/selfcheck_launch.cpp), the recover stages' launchers (tests/hostsim/ecdsa_launch.cpp: the self-check runs them), the new kernels as host loops (tests/hostsim/ecdsa_sign_launch.cpp) and a driver
(tests/hostsim/ecdsa_sign_driver.cpp) that pins every output to vectors this test writes from the restatement (tests/_ecdsa_sign.py) over the whole fixture: the host form
with chunks of 1, 7 and n, pageable and page-locked arrays, the device form on a caller stream (nothing runs before the caller synchronises), the three uniform levels,
sub-batches, the self-check on (same bytes, the stage list of the header), plume_init_multi contexts over three and eight mock devices, argument errors, every allocation
of a call failing in turn.  ASan + UBSan and TSan, lazy, random and eager schedulers.  One mutant of a launcher, which drops its stream argument, must fail the driver."""
import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import _ecdsa_sign as S

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
    units = [(["-x", "c++", "-O1", "-Werror"], CSRC / "plume_ecdsa_sign_capi.hip", "scapi.o"), (["-x", "c++", "-O1", "-Werror"], CSRC / "plume_ecdsa_capi.hip", "kcapi.o"), (["-x", "c++", "-O1", "-Werror"], CSRC / "plume_eth_hash_capi.hip", "hcapi.o"),
             (["-x", "c++", "-O1", "-Werror"], CSRC / "plume_selfcheck_capi.hip", "ccapi.o"), (["-O2", "-Werror"], HOSTSIM / "selfcheck_launch.cpp", "claunch.o"),
             (["-O2", "-Werror"], HOSTSIM / "ecdsa_launch.cpp", "rlaunch.o"), (["-O2", "-Werror", *launch_defs], HOSTSIM / "ecdsa_sign_launch.cpp", "slaunch.o"),
             (["-O1", "-Werror"], HOSTSIM / "ecdsa_sign_driver.cpp", "sdriver.o")]
    procs = [subprocess.Popen(["g++", *extra, *flags, "-c", str(src), "-o", str(out / obj)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for extra, src, obj in units]
    for p, (_, src, _) in zip(procs, units):
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, (src.name, err[-4000:])
    exe = out / "ecdsa_sign_driver"
    subprocess.run(["g++", *_san_flags(san), "-o", str(exe), *[str(out / o) for o in ("capi.o", "launch.o", "oracle.o", "scapi.o", "kcapi.o", "hcapi.o", "ccapi.o", "claunch.o", "rlaunch.o", "slaunch.o", "sdriver.o")],
                    "-lpthread"], check=True, capture_output=True, text=True, timeout=600)
    return exe


@pytest.fixture(scope="module")
def vectors(tmp_path_factory):
    """every item of the fixture (its own aux dropped: a call hedges all of its items or none) and what the restatement says of it without and with aux, once; the
    fixture's messages of both modes and their digests in both modes"""
    kats = S.load_kats()
    H = b"".join(bytes.fromhex(e["hash"]) for e in kats["sign"])
    SK = b"".join(bytes.fromhex(e["sk"]) for e in kats["sign"])
    n = len(kats["sign"])
    AUX = np.random.default_rng(5).bytes(32 * n)
    blob = struct.pack("<I", n) + H + SK + AUX
    for aux in (None, AUX):
        r, s, v, st = S.sign_batch(H, SK, aux, 0)
        assert S.BAD_SCALAR in st and int((st == S.OK).sum()) > n - 12
        blob += r.tobytes() + s.tobytes() + v.tobytes() + st.tobytes()
    msgs = [bytes.fromhex(e["msg"]) for e in kats["hash"]]
    off = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint64)
    buf = b"".join(msgs)
    blob += struct.pack("<I", len(msgs)) + off.tobytes() + buf + S.message_hash_batch(buf, off, S.KECCAK256).tobytes() + S.message_hash_batch(buf, off, S.EIP191).tobytes()
    path = tmp_path_factory.mktemp("ecdsa_sign_vectors") / "vectors.bin"
    path.write_bytes(blob)
    return path


def _run(exe, vectors, seed, sched):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")
    for k in ("PLUME_MOCK_SCHED", "PLUME_SUB_BATCHES", "PLUME_SERIAL", "PLUME_STAGE_TIMES", "PLUME_OVERLAP_MIN", "PLUME_SIGN_SELFCHECK", "PLUME_SIGN_UNIFORM"):
        env.pop(k, None)
    if sched:
        env["PLUME_MOCK_SCHED"] = sched
    return subprocess.run([str(exe), str(vectors), str(seed)], capture_output=True, text=True, timeout=1500, env=env)


def _ok(r, seed):
    assert r.returncode == 0, (seed, r.stdout[-2000:], r.stderr[-4000:])
    assert f"ecdsa_sign_driver seed {seed}: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "WARNING: ThreadSanitizer" not in r.stderr


@pytest.mark.parametrize("san,runs", [("address,undefined", [(1, None), (2, "random:2"), (3, "eager")]), ("thread", [(4, "random:4")])])
def test_ecdsa_sign_host_side_under_sanitizers(tmp_path, vectors, san, runs):
    exe = _build(tmp_path / "b", san)
    for seed, sched in runs:
        _ok(_run(exe, vectors, seed, sched), seed)


def test_the_driver_fails_when_a_launcher_drops_its_stream(tmp_path, vectors):
    r = _run(_build(tmp_path / "b", "", launch_defs=["-DECDSA_SIGN_MUTANT_DROPS_STREAM"]), vectors, 1, None)
    assert r.returncode != 0 and "ecdsa_sign_driver:" in r.stderr and "one device, host form" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])
