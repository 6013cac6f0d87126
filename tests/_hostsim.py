"""How a call family's host-side driver is built and run (tests/test_*_hostsim.py).  A family's program is the unchanged objects of the existing host-side harness
(tests/hostsim/Makefile: csrc/plume_capi.hip against the mock HIP runtime -> capi.o, the pipeline's kernels as host loops -> launch.o, the C oracle -> oracle.o) linked with
the family's translation units of csrc compiled as C++, its kernels as host loops (tests/hostsim/*_launch.cpp) and its driver (tests/hostsim/*_driver.cpp, which open with
driver_prelude.h).  Every program is stand-alone, with its own main, built with -fsanitize=... and run directly: nothing is loaded into Python.

The three base objects depend only on the sanitizer and on csrc, so for the tree's csrc they are built once per process -- or taken from the background builds of a
whole-suite run (tests/_prebuild.py), which are the same make command.  A build from a mutated copy of csrc is never cached and never shared."""
import atexit
import os
import shutil
import subprocess
import tempfile
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "zk-nullifier-sig_amd" / "csrc"
HOSTSIM = ROOT / "tests" / "hostsim"
FLAGS = ["-std=c++17", "-g", "-Wall", "-Wextra", "-Wno-unused-parameter", "-ffp-contract=off", "-DPLUME_GW=16", "-DPLUME_COMB_W=10", f"-I{HOSTSIM / 'mockhip'}"]
BASE = ("capi.o", "launch.o", "oracle.o")
# (sanitizers, [(seed, mock stream scheduler)]) of a family's test under the sanitizers: lazy, random and eager under ASan + UBSan, random under TSan
RUNS = [("address,undefined", [(1, None), (2, "random:2"), (3, "eager")]), ("thread", [(4, "random:4")])]

_PREBUILT = {"address,undefined": "hostsim_asan", "thread": "hostsim_tsan", "": "hostsim_plain"}
_bases = {}                                                # sanitizers -> the directory that holds the tree's own base objects


def san_flags(san):
    return [f"-fsanitize={san}", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if san else []


def _make_base(out, san, csrc, objects=BASE):
    mk = ["make", "-C", str(HOSTSIM), f"OUT={out}", f"SAN={san}", "-j2"]
    if csrc != CSRC:
        mk.append(f"CSRC={csrc}")
    subprocess.run(mk + [str(Path(out) / o) for o in objects], check=True, capture_output=True, text=True, timeout=1200)
    return Path(out)


def _tree_base(san):
    if san not in _bases:
        from tests import _prebuild
        pre = _prebuild.get(_PREBUILT[san]) if san in _PREBUILT else None
        if pre is not None and all((pre / o).exists() for o in BASE):
            _bases[san] = pre
        else:
            d = tempfile.mkdtemp(prefix="plume_hostsim_base_")
            atexit.register(shutil.rmtree, d, ignore_errors=True)
            _bases[san] = _make_base(d, san, CSRC)
    return _bases[san]


def build(out, san, driver, capi=(), launch=(), csrc=CSRC, defs=None, sources=None, oracle=True):
    """tests/hostsim/<driver>.cpp with the `capi` units of csrc (file names) and the `launch` files of tests/hostsim, under -fsanitize=<san>, into `out`; the executable.
    defs: source name -> extra flags (a launcher's mutant); sources: source name -> the file compiled in its place (a patched unit); csrc: a patched copy of the tree's"""
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("no g++ / make")
    out.mkdir(parents=True, exist_ok=True)
    defs, sources = defs or {}, sources or {}
    objects = [o for o in BASE if oracle or o != "oracle.o"]
    base = _tree_base(san) if csrc == CSRC else _make_base(out, san, csrc, objects)
    flags = FLAGS + [f"-I{csrc}"] + san_flags(san)
    units = [(["-x", "c++", "-O1", "-Werror"], name, csrc / name) for name in capi] + [(["-O2", "-Werror"], name, HOSTSIM / name) for name in launch]
    units.append((["-O1", "-Werror"], f"{driver}.cpp", HOSTSIM / f"{driver}.cpp"))
    objs = [out / (Path(name).stem + ".o") for _, name, _ in units]
    procs = [subprocess.Popen(["g++", *extra, *defs.get(name, ()), *flags, "-c", str(sources.get(name, src)), "-o", str(obj)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for (extra, name, src), obj in zip(units, objs)]
    for p, (_, name, _) in zip(procs, units):
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, (name, err[-4000:])
    exe = out / driver
    subprocess.run(["g++", *san_flags(san), "-o", str(exe), *[str(base / o) for o in objects], *map(str, objs), "-lpthread"], check=True, capture_output=True, text=True, timeout=600)
    return exe


def run(exe, *args, sched=None, extra_env=None, timeout=1500):
    """the program on `args`, with none of the caller's PLUME_* settings, under the mock's stream scheduler `sched` (None: lazy)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("PLUME_")}
    env.update(ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")
    if sched:
        env["PLUME_MOCK_SCHED"] = sched
    env.update(extra_env or {})
    return subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=timeout, env=env)


def ok(r, driver, seed):
    assert r.returncode == 0, (seed, r.stdout[-2000:], r.stderr[-4000:])
    assert f"{driver} seed {seed}: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "WARNING: ThreadSanitizer" not in r.stderr
