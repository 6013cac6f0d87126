"""The derived-nonce signer's host side (csrc/plume_nonce_capi.hip and the nonce hook of plume_capi.hip) under the sanitizers, on the CPU: the unchanged objects of the
existing host-side harness (tests/hostsim/Makefile: plume_capi.hip against the mock HIP runtime, the other kernels as host loops) linked with the ABI's translation unit,
k_sign_nonce as a host loop (tests/hostsim/nonce_launch.cpp) and a driver (tests/hostsim/nonce_driver.cpp) that checks every output against the C oracle's sign given the
lane body's nonces and, after every call, that no device allocation still holds a derived nonce or a staged secret: host and device forms, one device and eight, pieces of
5-64 items, pageable and page-locked arrays, an allocation failure at every allocation of a call, argument errors.  ASan + UBSan and TSan, random and eager schedulers; a
mutant that drops the nonce buffer's wipe must fail."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "zk-nullifier-sig_amd" / "csrc"
HOSTSIM = ROOT / "tests" / "hostsim"
FLAGS = ["-std=c++17", "-g", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off", "-DPLUME_GW=16", "-DPLUME_COMB_W=10", f"-I{HOSTSIM / 'mockhip'}"]
WIPE = "    if (nonce_fn) HIPCHK(hipMemsetAsync(ctx->nonce.p, 0, 32 * n, st));"


def _san_flags(san):
    return [f"-fsanitize={san}", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if san else []


def _build(out, san, csrc=CSRC):
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("no g++ / make")
    out.mkdir(parents=True, exist_ok=True)
    mk = ["make", "-C", str(HOSTSIM), f"OUT={out}", f"SAN={san}", "-j2"]
    if csrc != CSRC:
        mk.append(f"CSRC={csrc}")
    subprocess.run(mk + [str(out / "capi.o"), str(out / "launch.o"), str(out / "oracle.o")], check=True, capture_output=True, text=True, timeout=1200)
    flags = FLAGS + [f"-I{csrc}"] + _san_flags(san)
    units = [(["-x", "c++", "-O1", "-Werror"], csrc / "plume_nonce_capi.hip", "ncapi.o"), (["-O2", "-Werror"], HOSTSIM / "nonce_launch.cpp", "nlaunch.o"),
             (["-O1", "-Werror"], HOSTSIM / "nonce_driver.cpp", "ndriver.o")]
    for extra, src, obj in units:
        subprocess.run(["g++", *extra, *flags, "-c", str(src), "-o", str(out / obj)], check=True, capture_output=True, text=True, timeout=600)
    exe = out / "nonce_driver"
    subprocess.run(["g++", *_san_flags(san), "-o", str(exe), *[str(out / o) for o in ("capi.o", "launch.o", "oracle.o", "ncapi.o", "nlaunch.o", "ndriver.o")], "-lpthread"],
                   check=True, capture_output=True, text=True, timeout=600)
    return exe


def _run(exe, seed, sched):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")
    if sched:
        env["PLUME_MOCK_SCHED"] = sched
    return subprocess.run([str(exe), str(seed)], capture_output=True, text=True, timeout=900, env=env)


@pytest.mark.parametrize("san,runs", [("address,undefined", [(1, None), (2, "random:2"), (3, "eager")]), ("thread", [(4, "random:4")])])
def test_nonce_host_side_under_sanitizers(tmp_path, san, runs):
    exe = _build(tmp_path / "b", san)
    for seed, sched in runs:
        r = _run(exe, seed, sched)
        assert r.returncode == 0, (seed, sched, r.stdout[-2000:], r.stderr[-4000:])
        assert f"nonce_driver seed {seed}: ok" in r.stdout
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "WARNING: ThreadSanitizer" not in r.stderr


def test_the_driver_fails_when_the_nonce_buffer_is_not_wiped(tmp_path):
    """mutant: sign_device no longer wipes the workspace nonce buffer -- the driver's scan of device memory must find a nonce"""
    src = (CSRC / "plume_capi.hip").read_text()
    assert src.count(WIPE) == 1
    csrc = tmp_path / "pkg" / "csrc"                              # ../../include from csrc, as in the tree
    shutil.copytree(CSRC, csrc, ignore=shutil.ignore_patterns("*.o", "*.so"))
    (tmp_path / "include").mkdir()
    shutil.copy(ROOT / "include" / "plume_hip.h", tmp_path / "include" / "plume_hip.h")
    (csrc / "plume_capi.hip").write_text(src.replace(WIPE, ""))
    exe = _build(tmp_path / "b", "", csrc=csrc)
    r = _run(exe, 1, None)
    assert r.returncode != 0 and "!sec.count(r)" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])
