"""The signer's self-check on the host side (the gate in csrc/plume_capi.hip's sign_device, csrc/plume_selfcheck_capi.hip) under the sanitizers, on the CPU: the unchanged
objects of the existing host-side harness (tests/hostsim/Makefile: plume_capi.hip against the mock HIP runtime, the other kernels as host loops) linked with the ABI's
translation unit, k_sign_release as a host loop (tests/hostsim/selfcheck_launch.cpp) and a driver (tests/hostsim/selfcheck_driver.cpp) that checks every output against the
C oracle's sign + verify_non_zk on batches with planted wrong keys and, after every call, that no device allocation holds the c or s of a withheld item.  ASan + UBSan and
TSan, lazy, random and eager schedulers.  Three mutants must each fail the driver: a release launcher that ignores the verdict, the staging wipe removed, and the sign
kernels pointed at the caller's arrays instead of the staging (caught with a release launcher that writes nothing: the caller's arrays must still hold their pre-fill)."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "zk-nullifier-sig_amd" / "csrc"
HOSTSIM = ROOT / "tests" / "hostsim"
FLAGS = ["-std=c++17", "-g", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off", "-DPLUME_GW=16", "-DPLUME_COMB_W=10", f"-I{HOSTSIM / 'mockhip'}"]
WIPE = "        HIPCHK(hipMemsetAsync(ctx->scstage.p, 0, kStageBytes * n, st));"
REDIRECT = "    if (selfcheck) { pk = g_pk; nul = g_nul; c = g_c; s = g_s; rpt = g_rpt; hr = g_hr; status = g_status; out33 = false; }"


def _san_flags(san):
    return [f"-fsanitize={san}", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if san else []


def _build(out, san, csrc=CSRC, launch_defs=()):
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("no g++ / make")
    out.mkdir(parents=True, exist_ok=True)
    mk = ["make", "-C", str(HOSTSIM), f"OUT={out}", f"SAN={san}", "-j2"]
    if csrc != CSRC:
        mk.append(f"CSRC={csrc}")
    subprocess.run(mk + [str(out / "capi.o"), str(out / "launch.o"), str(out / "oracle.o")], check=True, capture_output=True, text=True, timeout=1200)
    flags = FLAGS + [f"-I{csrc}"] + _san_flags(san)
    units = [(["-x", "c++", "-O1", "-Werror"], csrc / "plume_selfcheck_capi.hip", "sccapi.o"), (["-O2", "-Werror", *launch_defs], HOSTSIM / "selfcheck_launch.cpp", "sclaunch.o"),
             (["-x", "c++", "-O1", "-Werror"], csrc / "plume_nonce_capi.hip", "ncapi.o"), (["-O2", "-Werror"], HOSTSIM / "nonce_launch.cpp", "nlaunch.o"),
             (["-O1", "-Werror"], HOSTSIM / "selfcheck_driver.cpp", "scdriver.o")]
    for extra, src, obj in units:
        subprocess.run(["g++", *extra, *flags, "-c", str(src), "-o", str(out / obj)], check=True, capture_output=True, text=True, timeout=600)
    exe = out / "selfcheck_driver"
    subprocess.run(["g++", *_san_flags(san), "-o", str(exe), *[str(out / o) for o in ("capi.o", "launch.o", "oracle.o", "sccapi.o", "sclaunch.o", "ncapi.o", "nlaunch.o", "scdriver.o")],
                    "-lpthread"], check=True, capture_output=True, text=True, timeout=600)
    return exe


def _run(exe, seed, sched, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")
    env.pop("PLUME_MOCK_SCHED", None)
    env.pop("PLUME_SIGN_SELFCHECK", None)
    if sched:
        env["PLUME_MOCK_SCHED"] = sched
    return subprocess.run([str(exe), str(seed), *args], capture_output=True, text=True, timeout=900, env=env)


def _ok(r, seed):
    assert r.returncode == 0, (seed, r.stdout[-2000:], r.stderr[-4000:])
    assert f"selfcheck_driver seed {seed}: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "WARNING: ThreadSanitizer" not in r.stderr


@pytest.mark.parametrize("san,runs", [("address,undefined", [(1, None), (2, "random:2"), (3, "eager")]), ("thread", [(4, "random:4")])])
def test_selfcheck_host_side_under_sanitizers(tmp_path, san, runs):
    exe = _build(tmp_path / "b", san)
    for seed, sched in runs:
        _ok(_run(exe, seed, sched), seed)


def _mutated_csrc(tmp_path, old, new):
    src = (CSRC / "plume_capi.hip").read_text()
    assert src.count(old) == 1, "the mutant's text is no longer in plume_capi.hip -- update the mutant"
    csrc = tmp_path / "pkg" / "csrc"                              # ../../include from csrc, as in the tree
    shutil.copytree(CSRC, csrc, ignore=shutil.ignore_patterns("*.o", "*.so"))
    (tmp_path / "include").mkdir()
    shutil.copy(ROOT / "include" / "plume_hip.h", tmp_path / "include" / "plume_hip.h")
    (csrc / "plume_capi.hip").write_text(src.replace(old, new))
    return csrc


def test_the_driver_fails_when_the_release_ignores_the_verdict(tmp_path):
    exe = _build(tmp_path / "b", "", launch_defs=["-DSELFCHECK_MUTANT_IGNORES_VERDICT"])
    r = _run(exe, 1, None)
    assert r.returncode != 0 and "selfcheck_driver:" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])


def test_the_driver_fails_when_the_staging_is_not_wiped(tmp_path):
    exe = _build(tmp_path / "b", "", csrc=_mutated_csrc(tmp_path, WIPE, ""))
    r = _run(exe, 1, None)
    assert r.returncode != 0 and "!sec.count(r)" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])


def test_the_driver_fails_when_the_sign_kernels_write_the_callers_arrays(tmp_path):
    """with a release launcher that writes nothing the caller's arrays keep their pre-fill -- unless the sign kernels were pointed at them"""
    nothing = ["-DSELFCHECK_RELEASE_NOTHING"]
    _ok(_run(_build(tmp_path / "good", "", launch_defs=nothing), 1, None, "prefill"), 1)
    exe = _build(tmp_path / "b", "", csrc=_mutated_csrc(tmp_path, REDIRECT, ""), launch_defs=nothing)
    r = _run(exe, 1, None, "prefill")
    assert r.returncode != 0 and "all_fill" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])
