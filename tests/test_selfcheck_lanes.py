"""k_sign_release's lane body (zk-nullifier-sig_amd/csrc/plume_selfcheck.h) on the host: tests/selfcheck/release_lanes.cpp compiled with g++ under AddressSanitizer +
UBSan and -Werror, against the restatement below.  Every combination of staged status (0, 1, 2, 4, 6) x verdict (0, 1, 2) x 64- / 33-byte form x pk array present / NULL x
destination alignment (all sixteen offsets from a 16-byte boundary, so the aligned 16-byte path, the gathered 16-byte path and the byte path at both ends all run), batch
sizes that end inside a quad, identity records (the 00 tag), odd and even y; the bytes around every array stay untouched."""
import itertools
import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "zk-nullifier-sig_amd" / "csrc"
WIDTHS = [64, 64, 32, 32, 64, 64]
POINTS = (0, 1, 4, 5)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("release_lanes") / "release_lanes"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}",
                    str(ROOT / "tests" / "selfcheck" / "release_lanes.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True, timeout=600)
    return exe


def release(stage, status, verdict, out33):
    """the definition (include/plume_hip.h, plume_set_sign_selfcheck): the seven caller arrays as lists of per-item bytes"""
    out = [[] for _ in range(7)]
    for i in range(len(status)):
        withheld = status[i] == 0 and verdict[i] != 1
        for k in range(6):
            rec = bytes(stage[k][i])
            if out33 and k in POINTS:
                rec = bytes(33) if rec == bytes(64) else bytes([2 + (rec[63] & 1)]) + rec[:32]
            out[k].append(bytes(len(rec)) if withheld else rec)
        out[6].append(bytes([status[i] if status[i] else (0 if verdict[i] == 1 else 8)]))
    return [b"".join(o) for o in out]


def _run(harness, tmp_path, stage, status, verdict, out33, has_pk, mis):
    n = len(status)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<4I", n, out33, has_pk, mis) + b"".join(np.ascontiguousarray(s).tobytes() for s in stage) + bytes(status) + bytes(verdict))
    r = subprocess.run([str(harness), str(fin), str(fout)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "release_lanes ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    got, want = fout.read_bytes(), release(stage, status, verdict, out33)
    pos = 0
    for k in range(7):
        if k == 0 and not has_pk:
            continue                                               # (the harness itself checked that nothing was written anywhere)
        seg = got[pos:pos + 64 + len(want[k])]
        pos += len(seg)
        assert seg[:32] == b"\xAA" * 32 and seg[-32:] == b"\xAA" * 32, f"record {k}: bytes outside the array were written"
        assert seg[32:-32] == want[k], f"record {k} (n={n}, out33={out33}, misalign={mis})"
    assert pos == len(got)


def _staging(rng, n):
    stage = [rng.integers(0, 256, size=(n, w), dtype=np.uint8) for w in WIDTHS]
    for k in POINTS:                                                # identities, and both parities of y
        stage[k][rng.random(n) < 0.2] = 0
        stage[k][:, 63] = (stage[k][:, 63] & 0xFE) | (rng.integers(0, 2, size=n, dtype=np.uint8) & stage[k].any(axis=1))
    return stage


def test_every_combination_of_status_verdict_form_and_alignment(harness, tmp_path):
    rng = np.random.default_rng(5)
    combos = list(itertools.product((0, 1, 2, 4, 6), (0, 1, 2)))
    status = [s for s, _ in combos] * 3
    verdict = [v for _, v in combos] * 3
    n = len(status)
    for out33, has_pk, mis in itertools.product((0, 1), (0, 1), range(16)):
        _run(harness, tmp_path, _staging(rng, n), status, verdict, out33, has_pk, mis)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 7, 16, 17, 255, 1000])
def test_batch_sizes_that_end_inside_a_quad(harness, tmp_path, n):
    rng = np.random.default_rng(n)
    for out33, mis in itertools.product((0, 1), (0, 4, 9)):
        status = list(rng.choice([0, 0, 0, 2, 5], size=n))
        verdict = list(rng.choice([1, 1, 0, 2], size=n))
        _run(harness, tmp_path, _staging(rng, n), [int(x) for x in status], [int(x) for x in verdict], out33, 1, mis)
