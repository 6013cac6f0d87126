"""plume_eth_tx_sign_batch* on the host side (csrc/plume_eth_tx_sign_capi.hip) under the sanitizers, on the CPU: the unchanged
objects of the existing host-side harness (tests/hostsim/Makefile: plume_capi.hip against the mock HIP runtime, the other kernels as host loops, the C oracle) linked with
the ABI's translation unit, the self-check's switch (csrc/plume_selfcheck_capi.hip, tests/hostsim/selfcheck_launch.cpp), the launchers of the sign and recover stages (tests/hostsim/ecdsa_sign_launch.cpp,
ecdsa_launch.cpp), the two new kernels as host loops
(tests/hostsim/eth_tx_sign_launch.cpp) and a driver (tests/hostsim/eth_tx_sign_driver.cpp) that pins every output to vectors this test writes from the restatement
(tests/_eth_tx_sign.py): the host form with chunks that cut the batch into 1, 2 and many pieces and on sub-ranges, the assembled out compared whole; the device form on a
caller stream; sub-batches; the self-check and the stage lists; plume_init_multi contexts over two and eight mock devices; argument errors; every allocation of a call
failing in turn; the staged sk and aux wiped on success and on failure.  ASan + UBSan and TSan, lazy, random and eager schedulers: stand-alone programs, nothing is
loaded into Python.  One mutant of the launcher, an assemble that writes one byte past out_len, must fail the driver."""
import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import _eth_tx as T
from tests import _eth_tx_sign as X
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
    units = [(["-x", "c++", "-O1", "-Werror"], CSRC / "plume_eth_tx_sign_capi.hip", "xcapi.o"), (["-x", "c++", "-O1", "-Werror"], CSRC / "plume_ecdsa_sign_capi.hip", "scapi.o"), (["-x", "c++", "-O1", "-Werror"], CSRC / "plume_ecdsa_capi.hip", "kcapi.o"), (["-O2", "-Werror"], HOSTSIM / "ecdsa_launch.cpp", "rlaunch.o"),
             (["-O2", "-Werror"], HOSTSIM / "ecdsa_sign_launch.cpp", "slaunch.o"), (["-O2", "-Werror", *launch_defs], HOSTSIM / "eth_tx_sign_launch.cpp", "xlaunch.o"),
             (["-x", "c++", "-O1", "-Werror"], CSRC / "plume_selfcheck_capi.hip", "ccapi.o"), (["-O2", "-Werror"], HOSTSIM / "selfcheck_launch.cpp", "claunch.o"),
             (["-O1", "-Werror"], HOSTSIM / "eth_tx_sign_driver.cpp", "xdriver.o")]
    procs = [subprocess.Popen(["g++", *extra, *flags, "-c", str(src), "-o", str(out / obj)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for extra, src, obj in units]
    for p, (_, src, _) in zip(procs, units):
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, (src.name, err[-4000:])
    exe = out / "eth_tx_sign_driver"
    subprocess.run(["g++", *_san_flags(san), "-o", str(exe), *[str(out / o) for o in ("capi.o", "launch.o", "oracle.o", "xcapi.o", "scapi.o", "kcapi.o", "ccapi.o", "claunch.o", "rlaunch.o", "slaunch.o", "xlaunch.o", "xdriver.o")],
                    "-lpthread"], check=True, capture_output=True, text=True, timeout=600)
    return exe


@pytest.fixture(scope="module")
def vectors(tmp_path_factory):
    """the first 72 short items of both fixtures as one batch (framed and unframed items alternate; keys out of range and the refused v among the new vectors are added) and what
    the restatement says of them without and with aux, once"""
    items, keys = X.fixture_batch()
    short = [(it, sk) for it, sk in zip(items, keys) if len(it) < 1000]
    extra = [(bytes.fromhex(e["unsigned"]), bytes.fromhex(e["sk"])) for e in X.load_kats()["items"] if e["status"] in (X.BAD_SCALAR, X.IDENTITY)]
    picked = short[:72] + extra
    items, keys = [p[0] for p in picked], [p[1] for p in picked]
    n = len(items)
    txs, off = T.pack(items)
    sk = b"".join(keys)
    aux = b"".join(K.keccak256(b"hostsim aux %d" % j) for j in range(n))
    blob = struct.pack("<I", n) + off.tobytes() + txs.tobytes() + sk + aux
    for a in (None, aux):
        w = X.sign_batch(txs, off, sk, a)
        assert (w["status"] == 0).sum() >= 20 and (w["status"] == X.BAD_TX).sum() >= 20 and (w["status"] == X.BAD_SCALAR).sum() == 3
        blob += b"".join(np.ascontiguousarray(w[k]).tobytes() for k in ("out", "out_len", "status", "hash", "r", "s", "v", "chain_id", "tx_type"))
    path = tmp_path_factory.mktemp("eth_tx_sign_vectors") / "vectors.bin"
    path.write_bytes(blob)
    return path


def _run(exe, vectors, seed, sched):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")
    for k in ("PLUME_MOCK_SCHED", "PLUME_SUB_BATCHES", "PLUME_SERIAL", "PLUME_STAGE_TIMES", "PLUME_OVERLAP_MIN", "PLUME_MSM_PAIR_MAX", "PLUME_INGEST_SPLIT_MAX", "PLUME_SIGN_SELFCHECK"):
        env.pop(k, None)
    if sched:
        env["PLUME_MOCK_SCHED"] = sched
    return subprocess.run([str(exe), str(vectors), str(seed)], capture_output=True, text=True, timeout=1500, env=env)


def _ok(r, seed):
    assert r.returncode == 0, (seed, r.stdout[-2000:], r.stderr[-4000:])
    assert f"eth_tx_sign_driver seed {seed}: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "WARNING: ThreadSanitizer" not in r.stderr


@pytest.mark.parametrize("san,runs", [("address,undefined", [(1, None), (2, "random:2"), (3, "eager")]), ("thread", [(4, "random:4")])])
def test_eth_tx_sign_host_side_under_sanitizers(tmp_path, vectors, san, runs):
    exe = _build(tmp_path / "b", san)
    for seed, sched in runs:
        _ok(_run(exe, vectors, seed, sched), seed)


def test_the_driver_fails_when_the_assemble_writes_past_out_len(tmp_path, vectors):
    r = _run(_build(tmp_path / "b", "", launch_defs=["-DETH_TX_SIGN_MUTANT_WRITES_PAST"]), vectors, 1, None)
    assert r.returncode != 0 and "eth_tx_sign_driver:" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])
