"""plume_eth_address_batch_device beside the verify it stands in front of, one GPU, same process, HIP events through torch, median of --reps after warm-up, in --rounds
interleaved rounds, all on the same device-resident pk array of --n items:
  * plume_eth_address_batch_device, 64-byte keys, every output, in the three address formats (raw20, record64, eip55)
  * plume_verify_batch_device version 1
  * a plain device-to-device copy of 84 B x n (what reading a 64-byte key and writing a 20-byte address costs at the least)
The bound: raw20 at or below 5 % of this run's verify step (an instruction count puts it near 2 %; the margin is for the on-curve check and clock differences between
boxes).  Prints one JSON line and writes it to --out (default profiles/eth_address_timing.json); exits 1 when the bound is missed.
    python tests/gpu_debug/eth_address_timing.py [--n 1048576] [--reps 5] [--rounds 3] [--out FILE]"""
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

BOUND = 0.05


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--msg-len", type=int, default=32)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "eth_address_timing.json"))
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
    eng.sign_batch_device(1, n, dm, doff, len(msgs), dsk, dr, None, pk, nul, c, s, rp, hr, status, stream=stream)
    stream.synchronize()
    assert not bool(status.any())
    widths = {"raw20": 20, "record64": 64, "eip55": 42}
    addr = {k: torch.zeros((n, w), dtype=torch.uint8, device=dev) for k, w in widths.items()}
    st = torch.zeros(n, dtype=torch.uint8, device=dev)
    ok = torch.zeros(n, dtype=torch.uint8, device=dev)
    src, dst = torch.zeros(84 * n, dtype=torch.uint8, device=dev), torch.zeros(84 * n, dtype=torch.uint8, device=dev)

    def eth(fmt):
        return lambda: eng.eth_address_batch_device(n, pk, None, addr[fmt], st, addr_format=fmt, stream=stream)

    def verify():
        eng.verify_batch_device(1, n, dm, doff, len(msgs), pk, nul, c, s, rp, hr, ok, stream=stream)

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

    runs = {k: [] for k in ("raw20", "record64", "eip55", "verify", "copy")}
    for _ in range(a.rounds):                                        # interleaved
        for fmt in widths:
            runs[fmt].append(timed(eth(fmt)))
        runs["verify"].append(timed(verify))
        runs["copy"].append(timed(copy))
    assert int(ok.sum()) == n and int((st == 1).sum()) == n
    # the three formats agree with each other and, on a sample, with the definition: the public address of sk = 1 is appended by hand below
    assert torch.equal(addr["record64"][:, 44:], addr["raw20"]) and not bool(addr["record64"][:, :44].any())
    low = bytes(addr["eip55"][7].cpu().numpy()).decode().lower()
    assert low == "0x" + bytes(addr["raw20"][7].cpu().numpy()).hex()
    g = bytes.fromhex("79be667ef9dcbbac55a06295ce870b07029bfcdb2dce28d959f2815b16f81798483ada7726a3c4655da4fbfc0e1108a8fd17b448a68554199c47d08ffb10d4b8")
    a1, s1 = eng.eth_address_batch(np.frombuffer(g, np.uint8), addr_format="eip55")
    assert a1[0].tobytes() == b"0x7E5F4552091A69125d5DfCb7b8C2659029395Bdf" and int(s1[0]) == 1
    med = {k: statistics.median(v) for k, v in runs.items()}
    res = {"n": n, "msg_len": L, "version": eng.version(), "eth_raw20_ms": med["raw20"], "eth_record64_ms": med["record64"], "eth_eip55_ms": med["eip55"],
           "verify_v1_ms": med["verify"], "copy_84B_ms": med["copy"], "all_ms": runs}
    res["raw20_over_verify"] = med["raw20"] / med["verify"]
    res["raw20_over_copy"] = med["raw20"] / med["copy"]
    res["addresses_per_s"] = n / (med["raw20"] * 1e-3)
    res["bound"] = BOUND
    res["within_bound"] = res["raw20_over_verify"] <= BOUND
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    eng.close()
    return 0 if res["within_bound"] else 1


if __name__ == "__main__":
    sys.exit(main())
