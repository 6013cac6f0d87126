"""plume_eth_tx_sign_batch_device beside its yardstick, the bare signer on the same digests; one GPU, one process, HIP events through torch on the call's stream, median of
--reps after warm-up, in --rounds interleaved rounds, for every n of --sizes: seeded type-02 transfers of about 120 bytes (built from --distinct unsigned items repeated,
a seeded key per item), and one more run at the largest n in which 1 % of the items carry 4 KiB of data.
  * plume_eth_tx_sign_batch_device, every output
  * plume_ecdsa_sign_batch_device over the digests the first call reported: the yardstick
  * one call of the first with stage timing on: what k_eth_tx_sign_frame and k_eth_tx_sign_assemble add, stage by stage
Prints one JSON line and writes it to --out (default profiles/eth_tx_sign_timing.json).  Every run checks that all items were signed and that the bare signer gives the r
the transaction signer reported.  Not run by the suite.
    python tests/gpu_debug/eth_tx_sign_timing.py [--sizes 1024,65536,1048576] [--distinct 4096] [--reps 7] [--rounds 3] [--out FILE]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import zk_nullifier_sig_amd as plume  # noqa: E402
from tests import _eth_tx as T  # noqa: E402

GROWTH = 68


def workload(n, distinct, seed, big_share=0.0):
    rng = np.random.default_rng(seed)
    base = []
    for j in range(distinct):
        data = rng.bytes(4096) if rng.random() < big_share else rng.bytes(int(rng.integers(60, 80)))
        base.append(T.signing_data(2, T.default_fields(2, 1, data, 2 * int(rng.integers(60)))))       # (an even salt: no access list)
    pick = rng.integers(distinct, size=n)
    items = [base[k] for k in pick]
    sk = np.frombuffer(rng.bytes(32 * n), np.uint8).reshape(n, 32).copy()
    sk[:, 0] &= 0x7F                                                     # below n; zero has probability 2^-255
    lens = [len(u) for u in items]
    return items, sk, min(lens), max(lens), sum(lens) / n


def measure(eng, dev, n, distinct, reps, rounds, big_share):
    items, sk, lmin, lmax, lmean = workload(n, distinct, 1, big_share)
    txs, off = T.pack(items)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    z = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
    dm, doff, dsk = t(txs), t(off.view(np.int64)), t(sk)
    nbytes = int(off[-1])
    out_bytes = nbytes + GROWTH * n
    out, out_len, st = z(out_bytes), torch.zeros(n, dtype=torch.int32, device=dev), z(n)
    h, r, s, v, typ = z(n, 32), z(n, 32), z(n, 32), z(n), z(n)
    chain = torch.zeros(n, dtype=torch.int64, device=dev)
    r2, s2, v2, st2 = z(n, 32), z(n, 32), z(n), z(n)
    stream = torch.cuda.Stream(dev)                                  # a stream of its own: the events below are recorded on the stream the library runs on
    stream.wait_stream(torch.cuda.current_stream(dev))

    def sign_tx():
        eng.eth_tx_sign_batch_device(n, dm, doff, nbytes, dsk, None, out, out_bytes, out_len, st, hash32=h, r=r, s=s, v=v, chain_id=chain, tx_type=typ, stream=stream)

    def sign():
        eng.ecdsa_sign_batch_device(n, h, dsk, None, r2, s2, v2, st2, stream=stream)

    def timed(fn):
        ms = []
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    runs = {"sign_tx": [], "sign": []}
    for _ in range(rounds):                                          # interleaved
        for k, fn in (("sign_tx", sign_tx), ("sign", sign)):
            runs[k].append(timed(fn))
    assert int((st == 0).sum()) == n and int((st2 == 0).sum()) == n and torch.equal(r, r2) and torch.equal(s, s2) and torch.equal(v, v2)
    assert int(out_len.sum()) > nbytes and int((typ == 2).sum()) == n
    eng.set_stage_timing(True)
    stages = {}
    try:
        for _ in range(reps):
            sign_tx()
            torch.cuda.synchronize()
            for name, ms in eng.last_stage_times():
                stages.setdefault(name, []).append(ms)
    finally:
        eng.set_stage_timing(False)
    stage_ms = {k: statistics.median(x) for k, x in stages.items()}
    med = {k: statistics.median(x) for k, x in runs.items()}
    added = med["sign_tx"] - med["sign"]
    return {"n": n, "big_share": big_share, "bytes_min": lmin, "bytes_max": lmax, "bytes_mean": lmean, "sign_tx_ms": med["sign_tx"], "ecdsa_sign_ms": med["sign"], "all_ms": runs,
            "added_ms": added, "sign_tx_over_sign": med["sign_tx"] / med["sign"], "stage_ms": stage_ms,
            "frame_share_of_sign": stage_ms.get("eth_tx_sign_frame", 0.0) / med["sign"], "assemble_share_of_sign": stage_ms.get("eth_tx_sign_assemble", 0.0) / med["sign"],
            "transactions_per_s": n / (med["sign_tx"] * 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,65536,1048576")
    ap.add_argument("--distinct", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "eth_tx_sign_timing.json"))
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",")]
    eng = plume.Engine(0)
    dev = torch.device("cuda:0")
    runs = [measure(eng, dev, n, a.distinct, a.reps, a.rounds, 0.0) for n in sizes]
    runs.append(measure(eng, dev, max(sizes), a.distinct, a.reps, a.rounds, 0.01))
    res = {"version": eng.version(), "reps": a.reps, "rounds": a.rounds, "distinct": a.distinct, "runs": runs}
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
