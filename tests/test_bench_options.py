"""bench.py's plain run and its two options: --full (everything besides the headline) and --dump-outputs DIR (what the last timed step computed, as .npy files)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "hbm_view", "valu_roofline", "stage_roofline", "cpu_baseline", "other_workloads", "e2e_host_pinned", "in_flight")


@pytest.fixture
def bench():
    """bench.py as a module, without the defaults it sets for its own process (PLUME_STAGE_TIMES=1, ...) staying in this one: contexts the later tests create must
    start from the library's defaults"""
    saved = dict(os.environ)
    import bench as mod
    os.environ.clear()
    os.environ.update(saved)
    return mod


def test_full_is_off_by_default_and_the_environment_can_ask_for_it(bench, monkeypatch):
    monkeypatch.delenv("PLUME_BENCH_FULL", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 3)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"
    monkeypatch.setenv("PLUME_BENCH_FULL", "1")
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    assert bench.parse().full


def test_dump_outputs_writes_float32_and_a_fixed_sample_above_the_budget(bench, tmp_path, monkeypatch):
    rng = np.random.default_rng(5)
    n = 4096
    arrs = {"pk": rng.integers(0, 256, (n, 64), dtype=np.uint8), "c": rng.integers(0, 256, (n, 32), dtype=np.uint8), "status": rng.integers(0, 2, n, dtype=np.uint8)}
    # everything fits: every row, no index file
    bench.dump_outputs(tmp_path / "all", arrs)
    assert not (tmp_path / "all" / "sample_index.npy").exists()
    for k, x in arrs.items():
        got = np.load(tmp_path / "all" / f"{k}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, x)
    # over the budget: the same seeded rows of every array, twice the same, within the budget
    monkeypatch.setattr(bench, "DUMP_BUDGET", 100_000)
    for d in ("s1", "s2"):
        bench.dump_outputs(tmp_path / d, arrs)
    idx = np.load(tmp_path / "s1" / "sample_index.npy")
    assert idx.dtype == np.float64 and np.array_equal(idx, np.load(tmp_path / "s2" / "sample_index.npy"))
    ii = idx.astype(np.int64)
    assert 0 < len(ii) < n and np.all(np.diff(ii) > 0) and ii[-1] < n
    data = 0
    for k, x in arrs.items():
        got = np.load(tmp_path / "s1" / f"{k}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, x[ii]) and np.array_equal(got, np.load(tmp_path / "s2" / f"{k}.npy"))
        data += got.nbytes
    assert data + idx.nbytes <= 100_000
    # ranks of a distributed run write their own files and share the budget
    bench.dump_outputs(tmp_path / "r", arrs, rank=1, world=2)
    assert (tmp_path / "r" / "rank1_pk.npy").exists() and not (tmp_path / "r" / "pk.npy").exists()
    assert sum(np.load(tmp_path / "r" / f"rank1_{k}.npy").nbytes for k in arrs) <= 50_000


def _bench(args, timeout=600):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py")] + args, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-1500:], r.stderr[-3000:])
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    """a plain run prints the contract's keys and none of the sections --full adds; --dump-outputs writes the last timed step's verdicts (V1 verify, 2^16) and the
    signer's seven arrays (2^14), the same in a second run, the verdicts equal to the corruption pattern and a sample of the signatures equal to the C oracle's"""
    from tests import _oracle_c as OC
    from tests import synth
    n = 1 << 16
    for k in ("v1", "v2"):
        d = _bench(["--gpus", "1", "--config", "2", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / k)])
        assert all(x in d for x in CONTRACT) and not any(x in d for x in FULL_ONLY), sorted(d)
        assert d["steps"] == 3 and d["unit"] == "verifies/s" and d["value"] > 0
        ok = np.load(tmp_path / k / "ok.npy")
        assert ok.dtype == np.float32 and np.array_equal(ok, synth.expected_ok(n))
    m = 1 << 14
    for k in ("s1", "s2"):
        d = _bench(["--gpus", "1", "--config", "3", "--log2-batch", "14", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / k)])
        assert d["unit"] == "signs/s" and not any(x in d for x in FULL_ONLY)
    outs = ("pk", "nullifier", "c", "s", "r_point", "hashed_to_curve_r", "status")
    got = {x: np.load(tmp_path / "s1" / f"{x}.npy") for x in outs}
    for x in outs:
        assert got[x].dtype == np.float32 and got[x].shape[0] == m and np.array_equal(got[x], np.load(tmp_path / "s2" / f"{x}.npy")), x
    assert not got["status"].any()
    b = synth.sign_inputs(64)
    want = OC.sign_batch(1, b["msgs"], b["off"], b["sk"], b["r"], nthreads=4)
    for x in outs[:-1]:
        assert np.array_equal(got[x][:64], want[x].astype(np.float32)), x
