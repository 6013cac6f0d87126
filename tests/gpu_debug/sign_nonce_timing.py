"""Derived-nonce signer timing on one GPU (include/plume_hip.h, plume_sign_batch_rfc6979*), same process, HIP events through torch, median of --reps:
  * k_sign_nonce alone: the `sign_nonce` stage of a serial device-resident call (plume_last_stage_times)
  * device-resident sign of --n V1 items, derived nonces against caller nonces (the ratio)
  * host-pointer sign from page-locked arrays, derived against caller nonces (items per second)
    python tests/gpu_debug/sign_nonce_timing.py [--n 1048576] [--reps 5] [--msg-len 32] [--uniform 1]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import zk_nullifier_sig_amd as plume  # noqa: E402
from zk_nullifier_sig_amd import capi  # noqa: E402


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
    sk[:, 0] &= 0x7F
    sk[:, 31] |= 1
    r = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    r[:, 0] &= 0x7F
    r[:, 31] |= 1
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    dm, doff, dsk, dr = t(msgs), t(off.view(np.int64)), t(sk), t(r)
    o = [torch.zeros((n, w), dtype=torch.uint8, device=dev) for w in (64, 64, 32, 32, 64, 64)] + [torch.zeros(n, dtype=torch.uint8, device=dev)]

    stream = torch.cuda.Stream(dev)                                  # a stream of its own: the events below are recorded on the stream the library runs on
    stream.wait_stream(torch.cuda.current_stream(dev))

    def caller():
        eng.sign_batch_device(1, n, dm, doff, len(msgs), dsk, dr, None, *o, stream=stream)

    def derived():
        eng.sign_batch_rfc6979_device(1, n, dm, doff, len(msgs), dsk, None, None, *o, stream=stream)

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

    res = {"n": n, "msg_len": L, "uniform": a.uniform, "version": plume.library_path().name}
    # interleaved A/B of the device-resident calls
    ca, de = [], []
    for _ in range(3):
        ca.append(timed(caller))
        de.append(timed(derived))
    res["device_caller_ms"], res["device_derived_ms"] = statistics.median(ca), statistics.median(de)
    res["device_ratio"] = res["device_derived_ms"] / res["device_caller_ms"]
    eng.set_stage_timing(1)
    st = []
    for _ in range(a.reps):
        derived()
        torch.cuda.synchronize()
        st.append(dict(eng.last_stage_times()))
    eng.set_stage_timing(0)
    res["stages_ms"] = {k: statistics.median(s[k] for s in st) for k in st[0]}
    res["sign_nonce_ms"] = res["stages_ms"].get("sign_nonce")
    # host-pointer calls from page-locked arrays
    pm, poff, psk, pr = capi.pinned_copy(msgs), capi.pinned_copy(off), capi.pinned_copy(sk), capi.pinned_copy(r)
    out = {k: capi.pinned_empty((n, w)) for k, w in [("pk", 64), ("nullifier", 64), ("c", 32), ("s", 32), ("r_point", 64), ("hashed_to_curve_r", 64)]}
    out["status"] = capi.pinned_empty(n)

    def wall(fn):
        fn()
        xs = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            xs.append(time.perf_counter() - t0)
        return statistics.median(xs)
    hc = wall(lambda: eng.sign_batch(1, pm, poff, psk, pr, out=out))
    hd = wall(lambda: eng.sign_batch_rfc6979(1, pm, poff, psk, out=out))
    res["host_caller_Mps"], res["host_derived_Mps"] = n / hc / 1e6, n / hd / 1e6
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
