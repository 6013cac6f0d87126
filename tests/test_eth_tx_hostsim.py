"""plume_eth_tx_parse_batch* and plume_eth_tx_sender_batch* on the host side (csrc/plume_eth_tx_capi.hip) under the sanitizers, on
the CPU: the unchanged objects of the existing host-side harness (tests/hostsim/Makefile: plume_capi.hip against the mock HIP runtime, the other kernels as host loops, the C
oracle) linked with the ABI's translation unit, the recover stages' launchers (tests/hostsim/ecdsa_launch.cpp), k_eth_tx_parse as a host loop
(tests/hostsim/eth_tx_launch.cpp) and a driver (tests/hostsim/eth_tx_driver.cpp) that pins every output to vectors this test writes from the restatements
(tests/_eth_tx.py, tests/_ecdsa.py) over the committed fixture: the host form with chunks of 1, 7 and n, the device form on a caller stream (nothing runs before the caller
synchronises), sub-batches, the stage lists, plume_init_multi contexts over three and eight mock devices, argument errors, every allocation of a call failing in turn, no
table built by a context that only parses.  ASan + UBSan and TSan, lazy, random and eager schedulers: stand-alone programs, nothing is loaded into Python.  One mutant of
the launcher, which drops its stream argument, must fail the driver."""
import os
import shutil
import struct
import subprocess
from pathlib import Path

import pytest

from tests import _ecdsa as E
from tests import _eth_tx as T

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
    units = [(["-x", "c++", "-O1", "-Werror"], CSRC / "plume_eth_tx_capi.hip", "tcapi.o"), (["-x", "c++", "-O1", "-Werror"], CSRC / "plume_ecdsa_capi.hip", "kcapi.o"), (["-O2", "-Werror"], HOSTSIM / "ecdsa_launch.cpp", "rlaunch.o"),
             (["-O2", "-Werror", *launch_defs], HOSTSIM / "eth_tx_launch.cpp", "tlaunch.o"), (["-O1", "-Werror"], HOSTSIM / "eth_tx_driver.cpp", "tdriver.o")]
    procs = [subprocess.Popen(["g++", *extra, *flags, "-c", str(src), "-o", str(out / obj)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for extra, src, obj in units]
    for p, (_, src, _) in zip(procs, units):
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, (src.name, err[-4000:])
    exe = out / "eth_tx_driver"
    subprocess.run(["g++", *_san_flags(san), "-o", str(exe), *[str(out / o) for o in ("capi.o", "launch.o", "oracle.o", "tcapi.o", "kcapi.o", "rlaunch.o", "tlaunch.o", "tdriver.o")], "-lpthread"],
                   check=True, capture_output=True, text=True, timeout=600)
    return exe


@pytest.fixture(scope="module")
def vectors(tmp_path_factory):
    """the fixture's items (the two long ones left out: the recover stages of a CPU are slow enough) and what the restatements say of them, once"""
    raws = [bytes.fromhex(e["raw"]) for e in T.load_kats()["items"] if len(e["raw"]) < 4000]
    txs, off = T.pack(raws)
    p = T.parse_batch(txs, off)
    pk, addr, st = E.recover_batch(p["hash"], p["r"], p["s"], p["v"], None, "affine64", "raw20", E.LOW_S)
    assert (st[p["status"] == T.INVALID] == 3).all() and int((st == 1).sum()) > 100 and int(((st == 3) & (p["status"] == T.OK)).sum()) >= 5
    blob = struct.pack("<I", len(raws)) + off.tobytes() + txs.tobytes() + b"".join(p[k].tobytes() for k in ("hash", "r", "s", "v", "tx_type", "status", "chain_id"))
    blob += pk.tobytes() + addr.tobytes() + st.tobytes()
    path = tmp_path_factory.mktemp("eth_tx_vectors") / "vectors.bin"
    path.write_bytes(blob)
    return path


def _run(exe, vectors, seed, sched):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")
    for k in ("PLUME_MOCK_SCHED", "PLUME_SUB_BATCHES", "PLUME_SERIAL", "PLUME_STAGE_TIMES", "PLUME_OVERLAP_MIN", "PLUME_MSM_PAIR_MAX", "PLUME_INGEST_SPLIT_MAX"):
        env.pop(k, None)
    if sched:
        env["PLUME_MOCK_SCHED"] = sched
    return subprocess.run([str(exe), str(vectors), str(seed)], capture_output=True, text=True, timeout=1500, env=env)


def _ok(r, seed):
    assert r.returncode == 0, (seed, r.stdout[-2000:], r.stderr[-4000:])
    assert f"eth_tx_driver seed {seed}: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "WARNING: ThreadSanitizer" not in r.stderr


@pytest.mark.parametrize("san,runs", [("address,undefined", [(1, None), (2, "random:2"), (3, "eager")]), ("thread", [(4, "random:4")])])
def test_eth_tx_host_side_under_sanitizers(tmp_path, vectors, san, runs):
    exe = _build(tmp_path / "b", san)
    for seed, sched in runs:
        _ok(_run(exe, vectors, seed, sched), seed)


def test_the_driver_fails_when_the_launcher_drops_its_stream(tmp_path, vectors):
    r = _run(_build(tmp_path / "b", "", launch_defs=["-DETH_TX_MUTANT_DROPS_STREAM"]), vectors, 1, None)
    assert r.returncode != 0 and "eth_tx_driver:" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])
