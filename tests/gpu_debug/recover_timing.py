"""plume_recover_batch_device beside the verify it is built from, one GPU, same process, HIP events through torch, median of --reps after warm-up, alternating:
  * plume_recover_batch_device (version 2, 64-byte records, every output) of --n device-resident items
  * plume_verify_batch_device version 2 on the same inputs
  * a plain device-to-device copy of 192 B x n (what writing three 64-byte records per item costs at the least)
Recover should cost the verify plus about that copy.  The bound it is held to is the baseline's own run-to-run spread in this process: recover <= (verify + copy) x
(1 + spread), spread = (max - min) / median over the verify rounds.  Also the stage times of one call of each kind: recover_finalize beside verify_finalize.
Prints one JSON line and writes it to --out (default profiles/recover_timing.json); exits 1 when the bound is missed.
    python tests/gpu_debug/recover_timing.py [--n 1048576] [--reps 5] [--rounds 4] [--out FILE]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--msg-len", type=int, default=32)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "recover_timing.json"))
    a = ap.parse_args()
    n, L = a.n, a.msg_len
    eng = plume.Engine(0)
    rng = np.random.default_rng(1)
    msgs = rng.integers(0, 256, size=n * L + 16, dtype=np.uint8)
    off = (np.arange(n + 1, dtype=np.uint64) * L)
    sk = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    r = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    for x in (sk, r):
        x[:, 0] &= 0x7F
        x[:, 31] |= 1
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    dm, doff, dsk, dr = t(msgs), t(off.view(np.int64)), t(sk), t(r)
    pk, nul, c, s, rp, hr = (torch.zeros((n, w), dtype=torch.uint8, device=dev) for w in (64, 64, 32, 32, 64, 64))
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)                                  # a stream of its own: the events below are recorded on the stream the library runs on
    stream.wait_stream(torch.cuda.current_stream(dev))
    eng.sign_batch_device(2, n, dm, doff, len(msgs), dsk, dr, None, pk, nul, c, s, rp, hr, status, stream=stream)
    stream.synchronize()
    assert not bool(status.any())
    out = [torch.zeros((n, 64), dtype=torch.uint8, device=dev) for _ in range(3)]
    st = torch.zeros(n, dtype=torch.uint8, device=dev)
    ok = torch.zeros(n, dtype=torch.uint8, device=dev)
    src, dst = torch.zeros(192 * n, dtype=torch.uint8, device=dev), torch.zeros(192 * n, dtype=torch.uint8, device=dev)

    def recover():
        eng.recover_batch_device(2, n, dm, doff, len(msgs), pk, nul, c, s, out[0], out[1], out[2], st, stream=stream)

    def verify():
        eng.verify_batch_device(2, n, dm, doff, len(msgs), pk, nul, c, s, None, None, ok, stream=stream)

    def copy():
        with torch.cuda.stream(stream):
            dst.copy_(src, non_blocking=True)

    def timed(fn):
        ms = []
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    rec, ver, cp = [], [], []
    for _ in range(a.rounds):                                        # alternating
        rec.append(timed(recover))
        ver.append(timed(verify))
        cp.append(timed(copy))
    assert int(ok.sum()) == n and int((st == 1).sum()) == n and torch.equal(out[0], rp) and torch.equal(out[1], hr)
    res = {"n": n, "msg_len": L, "version": eng.version(), "recover_ms": statistics.median(rec), "verify_ms": statistics.median(ver), "copy_192B_ms": statistics.median(cp),
           "all_recover_ms": rec, "all_verify_ms": ver, "all_copy_ms": cp}
    res["ratio_to_verify"] = res["recover_ms"] / res["verify_ms"]
    res["ratio_to_verify_plus_copy"] = res["recover_ms"] / (res["verify_ms"] + res["copy_192B_ms"])
    res["verify_spread"] = (max(ver) - min(ver)) / res["verify_ms"]
    res["bound"] = 1.0 + res["verify_spread"]
    res["within_bound"] = res["ratio_to_verify_plus_copy"] <= res["bound"]
    eng.set_stage_timing(1)
    stages = {}
    for name, fn in (("recover", recover), ("verify", verify)):
        runs = []
        for _ in range(a.reps):
            fn()
            torch.cuda.synchronize()
            runs.append(eng.last_stage_times())
        stages[name] = [[k, statistics.median(x[j][1] for x in runs)] for j, (k, _) in enumerate(runs[0])]
    eng.set_stage_timing(0)
    res["recover_stages_ms"], res["verify_stages_ms"] = stages["recover"], stages["verify"]
    res["recover_finalize_ms"], res["verify_finalize_ms"] = dict(stages["recover"]).get("recover_finalize"), dict(stages["verify"]).get("verify_finalize")
    res["msm_kernel"] = eng.last_msm_kernel()
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    eng.close()
    return 0 if res["within_bound"] else 1


if __name__ == "__main__":
    sys.exit(main())
