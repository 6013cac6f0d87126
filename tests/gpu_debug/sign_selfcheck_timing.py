"""The signer's self-check on one GPU (include/plume_hip.h, plume_set_sign_selfcheck), same process, HIP events through torch, median of --reps after warm-up:
  * device-resident V1 sign of --n items with the check on (mode 1)
  * what a caller can do without it: the mode-0 sign followed by plume_verify_non_zk_batch_device of its outputs on the same stream (the sum the issue compares against)
  * the stage times of a mode-1 call (plume_last_stage_times): the sign stages, the check's stages, then sign_release -- beside the 0.13 ms a pure copy of 0.8 GB would take
Prints one JSON line; exits 1 when mode 1 takes more than 1.03 x the sign-then-verify sum.
    python tests/gpu_debug/sign_selfcheck_timing.py [--n 1048576] [--reps 5] [--msg-len 32] [--uniform 1]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import zk_nullifier_sig_amd as plume  # noqa: E402


BOUND = 1.03   # mode 1 may take at most this multiple of sign + verify_non_zk (same-box repeats differ by under 1 %, the staging pass adds about 0.4 %)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--msg-len", type=int, default=32)
    ap.add_argument("--uniform", type=int, default=1)
    a = ap.parse_args()
    n, L = a.n, a.msg_len
    eng = plume.Engine(0)
    eng.set_sign_uniform(a.uniform)
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
    o = [torch.zeros((n, w), dtype=torch.uint8, device=dev) for w in (64, 64, 32, 32, 64, 64)] + [torch.zeros(n, dtype=torch.uint8, device=dev)]
    pk, nul, c, s, rp, hr, status = o
    ok = torch.zeros(n, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)                                  # a stream of its own: the events below are recorded on the stream the library runs on
    stream.wait_stream(torch.cuda.current_stream(dev))

    def sign():
        eng.sign_batch_device(1, n, dm, doff, len(msgs), dsk, dr, None, *o, stream=stream)

    def sign_then_verify():
        sign()
        eng.verify_non_zk_batch_device(1, n, dm, doff, len(msgs), pk, nul, s, rp, hr, c, ok, stream=stream)

    def timed(fn, mode):
        eng.set_sign_selfcheck(mode)
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

    res = {"n": n, "msg_len": L, "uniform": a.uniform, "version": eng.version()}
    on, two, plain = [], [], []
    for _ in range(3):                                               # interleaved
        on.append(timed(sign, 1))
        two.append(timed(sign_then_verify, 0))
        plain.append(timed(sign, 0))
    assert int(ok.sum()) == n and not bool(status.any())
    res["selfcheck_ms"], res["sign_then_verify_ms"], res["sign_ms"] = statistics.median(on), statistics.median(two), statistics.median(plain)
    res["all_selfcheck_ms"], res["all_sign_then_verify_ms"] = on, two
    res["ratio"] = res["selfcheck_ms"] / res["sign_then_verify_ms"]
    eng.set_sign_selfcheck(1)
    eng.set_stage_timing(1)
    st = []
    for _ in range(a.reps):
        sign()
        torch.cuda.synchronize()
        st.append(eng.last_stage_times())
    eng.set_stage_timing(0)
    eng.set_sign_selfcheck(0)
    res["stages_ms"] = [[k, statistics.median(x[j][1] for x in st)] for j, (k, _) in enumerate(st[0])]      # in order: "tables" occurs twice (the signer's, the check's)
    res["sign_release_ms"] = res["stages_ms"][-1][1] if res["stages_ms"][-1][0] == "sign_release" else None
    res["sign_release_copy_estimate_ms"] = 0.13
    res["msm_kernel"] = eng.last_msm_kernel()
    res["bound"] = BOUND
    res["within_bound"] = res["ratio"] <= BOUND
    print(json.dumps(res))
    eng.close()
    return 0 if res["within_bound"] else 1


if __name__ == "__main__":
    sys.exit(main())
