"""The key-derivation calls beside their yardstick, plume_ecdsa_sign_batch_device at the same n (one comb multiplication per item); one GPU, one process, HIP events through
torch on the call's stream, median of --reps after warm-up, in --rounds interleaved rounds, for every n of --sizes:
  * priv1    plume_hd_derive_priv_batch_device, depth 1, ONE shared parent, item i takes index i: the .../0/i case, every output
  * priv5    the same call at depth 5 (m/44'/60'/0'/0/i from per-item master nodes)
  * pub1     plume_hd_derive_pub_batch_device, depth 1, one shared parent, pk and address out
  * sign     plume_ecdsa_sign_batch_device over seeded digests with the keys priv1 derived: the yardstick
  * one call of each derive form with stage timing on: the time per stage
Prints one JSON line and writes it to --out (default profiles/hd_timing.json).  Every run checks that all items were derived and that the public form gives the
addresses the private form gave.  Not run by the suite.
    python tests/gpu_debug/hd_timing.py [--sizes 1024,65536,1048576] [--reps 7] [--rounds 3] [--out FILE]"""
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

HARD = 2**31


def measure(eng, dev, n, reps, rounds):
    rng = np.random.default_rng(n)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    z = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
    node = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    node[:, 0] &= 0x7F
    d_sk, d_chain = t(node), t(rng.integers(0, 256, (n, 32), dtype=np.uint8))
    idx = np.arange(n, dtype=np.uint32)
    path1 = t(idx.reshape(n, 1).view(np.int32))
    p5 = np.empty((n, 5), np.uint32)
    p5[:, 0], p5[:, 1], p5[:, 2], p5[:, 3], p5[:, 4] = HARD + 44, HARD + 60, HARD, 0, idx
    path5 = t(p5.view(np.int32))
    sk, chain, pk, addr, st = z(n, 32), z(n, 32), z(n, 64), z(n, 20), z(n)
    sk5, st5 = z(n, 32), z(n)
    ppk, paddr, pst = z(n, 64), z(n, 20), z(n)
    h, r, s, v, sst = t(rng.integers(0, 256, (n, 32), dtype=np.uint8)), z(n, 32), z(n, 32), z(n), z(n)
    stream = torch.cuda.Stream(dev)                                  # a stream of its own: the events below are recorded on the stream the library runs on
    stream.wait_stream(torch.cuda.current_stream(dev))
    # the shared parent: a node one hardened level down, with its public key
    up = eng.hd_derive_priv_batch(node[:1], d_chain[:1].cpu().numpy(), np.array([[HARD]], np.uint32), want=("chain", "pk"))     # a node and its public key: the watcher's xpub
    d_usk, d_uchain, d_upk = t(up["sk"]), t(up["chain"]), t(up["pk"])

    def priv1():
        eng.hd_derive_batch_device(False, plume.HD_SHARED_PARENT, n, d_usk, d_uchain, path1, 1, sk, chain, pk, addr, st, stream=stream)

    def priv5():
        eng.hd_derive_batch_device(False, 0, n, d_sk, d_chain, path5, 5, sk5, None, None, None, st5, stream=stream)

    def pub1():
        eng.hd_derive_batch_device(True, plume.HD_SHARED_PARENT, n, d_upk, d_uchain, path1, 1, None, None, ppk, paddr, pst, stream=stream)

    def sign():
        eng.ecdsa_sign_batch_device(n, h, sk, None, r, s, v, sst, stream=stream)

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

    calls = (("priv1", priv1), ("priv5", priv5), ("pub1", pub1), ("sign", sign))
    runs = {k: [] for k, _ in calls}
    for _ in range(rounds):                                          # interleaved
        for k, fn in calls:
            runs[k].append(timed(fn))
    assert int(st.count_nonzero()) == 0 and int(st5.count_nonzero()) == 0 and int(pst.count_nonzero()) == 0 and int(sst.count_nonzero()) == 0
    assert torch.equal(ppk, pk) and torch.equal(paddr, addr)
    eng.set_stage_timing(True)
    stage_ms = {}
    try:
        for k, fn in calls[:3]:
            stages = {}
            for _ in range(reps):
                fn()
                torch.cuda.synchronize()
                for name, ms in eng.last_stage_times():
                    stages.setdefault(name, []).append(ms)
            stage_ms[k] = {name: statistics.median(x) * (len(x) // reps) for name, x in stages.items()}      # a stage that runs once per level: its total
    finally:
        eng.set_stage_timing(False)
    med = {k: statistics.median(x) for k, x in runs.items()}
    return {"n": n, "ms": med, "all_ms": runs, "over_sign": {k: med[k] / med["sign"] for k in ("priv1", "priv5", "pub1")}, "stage_ms": stage_ms,
            "keys_per_s": {k: n / (med[k] * 1e-3) for k in ("priv1", "priv5", "pub1")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,65536,1048576")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "hd_timing.json"))
    a = ap.parse_args()
    eng = plume.Engine(0)
    dev = torch.device("cuda:0")
    runs = [measure(eng, dev, int(x), a.reps, a.rounds) for x in a.sizes.split(",")]
    res = {"version": eng.version(), "reps": a.reps, "rounds": a.rounds, "runs": runs}
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
