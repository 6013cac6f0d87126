"""plume_pbkdf2_sha512_batch_device beside its yardstick, hashlib.pbkdf2_hmac over the same sentences on 16 worker processes; one GPU, one process on it, HIP events
through torch on the call's stream, median of --reps after warm-up, in --rounds interleaved rounds, for every n of --sizes:
  * seeds     BIP-39 seeds of n twelve-word sentences (2048 iterations, 64 bytes, "mnemonic" in front of one shared passphrase) at the library's slice, PLUME_KDF_SLICE
  * slices    the same call with the remaining 2047 iterations enqueued in slices of 128 / 256 / 512 / one dispatch (env PLUME_KDF_SLICE, read per call), interleaved
  * one call with stage timing on: the time per stage, the slices of "kdf_iter" summed
  * cpu       hashlib.pbkdf2_hmac("sha512", sentence, b"mnemonic" + passphrase, 2048) over --cpu-items of the sentences, 16 worker processes (started before the GPU
              is opened; they never touch it)
Prints one JSON line and writes it to --out (default profiles/kdf_timing.json).  Every run checks the outputs of a seeded sample of the items against hashlib.  The
sentences are twelve words drawn from a short made-up list: the word list is out of scope and any bytes have a seed.  Not run by the suite.
    python tests/gpu_debug/kdf_timing.py [--sizes 1024,65536,1048576] [--reps 7] [--rounds 3] [--out FILE]"""
import argparse
import hashlib
import json
import multiprocessing
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

WORDS = "abandon ability able about above absent absorb abstract absurd abuse access accident zone zoo wrong year".split()
PASSPHRASE = b"timing"
SLICES = (128, 256, 512, 0)                                     # 0: one dispatch for all the remaining iterations


def sentences(n, seed):
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, len(WORDS), (n, 12))
    return [" ".join(WORDS[j] for j in row).encode() for row in idx]


def _cpu_seed(s):
    return hashlib.pbkdf2_hmac("sha512", s, b"mnemonic" + PASSPHRASE, 2048)


def cpu_yardstick(items, workers=16):
    with multiprocessing.get_context("fork").Pool(workers) as pool:
        pool.map(_cpu_seed, items[:workers])                       # the workers are up
        t0 = time.perf_counter()
        pool.map(_cpu_seed, items, chunksize=max(1, len(items) // (4 * workers)))
        dt = time.perf_counter() - t0
    return {"items": len(items), "workers": workers, "seconds": dt, "seeds_per_s": len(items) / dt}


def measure(eng, torch, plume, dev, n, reps, rounds):
    items = sentences(n, n)
    buf, off = plume.capi.pack_messages(items)
    d_pw, d_off = torch.from_numpy(buf).to(dev), torch.from_numpy(off.view(np.int64)).to(dev)
    d_salt = torch.from_numpy(np.frombuffer(PASSPHRASE, np.uint8).copy()).to(dev)
    out, st = torch.zeros((n, 64), dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)                                  # a stream of its own: the events below are recorded on the stream the library runs on
    stream.wait_stream(torch.cuda.current_stream(dev))
    sample = np.random.default_rng(n + 1).choice(n, min(n, 24), replace=False)

    def call():
        eng.pbkdf2_sha512_batch_device(n, d_pw, d_off, int(off[n]), d_salt, len(PASSPHRASE), 2048, 64, out, st, flags=plume.KDF_BIP39 | plume.KDF_SHARED_SALT, stream=stream)

    def check():
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert int(st.count_nonzero()) == 0
        for i in sample:
            assert got[i].tobytes() == _cpu_seed(items[i]), (n, int(i))
        out.zero_()

    def timed(slice_):
        if slice_ is None:
            os.environ.pop("PLUME_KDF_SLICE", None)
        else:
            os.environ["PLUME_KDF_SLICE"] = str(slice_)
        try:
            ms = []
            call()
            check()
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call()
                e1.record(stream)
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            check()
            return statistics.median(ms)
        finally:
            os.environ.pop("PLUME_KDF_SLICE", None)

    arms = [("seeds", None)] + [(f"slice_{s or 'all'}", s) for s in SLICES]
    runs = {k: [] for k, _ in arms}
    for _ in range(rounds):                                          # interleaved
        for k, s in arms:
            runs[k].append(timed(s))
    eng.set_stage_timing(True)
    try:
        stages = {}
        for _ in range(reps):
            call()
            torch.cuda.synchronize()
            per_call = {}
            for name, ms in eng.last_stage_times():
                per_call[name] = per_call.get(name, 0.0) + ms         # the slices of kdf_iter: their total
            for name, ms in per_call.items():
                stages.setdefault(name, []).append(ms)
        stage_ms = {name: statistics.median(x) for name, x in stages.items()}
    finally:
        eng.set_stage_timing(False)
    med = {k: statistics.median(x) for k, x in runs.items()}
    return {"n": n, "ms": med, "all_ms": runs, "stage_ms": stage_ms, "seeds_per_s": n / (med["seeds"] * 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,65536,1048576")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cpu-items", type=int, default=8192)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "kdf_timing.json"))
    a = ap.parse_args()
    cpu = cpu_yardstick(sentences(a.cpu_items, 1))                    # before the GPU is opened: the workers are forked from a process that holds no device
    import torch
    import zk_nullifier_sig_amd as plume
    eng = plume.Engine(0)
    dev = torch.device("cuda:0")
    runs = [measure(eng, torch, plume, dev, int(x), a.reps, a.rounds) for x in a.sizes.split(",")]
    res = {"version": eng.version(), "reps": a.reps, "rounds": a.rounds, "cpu": cpu, "runs": runs,
           "gpu_over_cpu": {str(r["n"]): r["seeds_per_s"] / cpu["seeds_per_s"] for r in runs}}
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
