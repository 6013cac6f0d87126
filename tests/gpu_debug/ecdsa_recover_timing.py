"""plume_ecdsa_recover_batch_device beside a V1 verify of as many items, one GPU, same process, HIP events through torch, median of --reps after warm-up, in --rounds
interleaved rounds, on --n device-resident genuine signatures:
  * plume_ecdsa_recover_batch_device, every output, 20-byte addresses + 64-byte keys
  * plume_verify_batch_device version 1
and the recovery's per-stage split from plume_last_stage_times (one more call with stage timing on, outside the timed ones).
The signatures are genuine: the signer's own kernels give pk = sk G and R = k G for n seeded keys and nonces (plume_sign_batch_device: its pk and r_point outputs), the
host finishes them -- r = R.x, v = parity of R.y, s = k^-1 (z + r sk) mod n over a random 32-byte digest -- and the recovered keys must equal pk, all n of them.
The yardstick is the verify step of the SAME run: a verify does two double multiplications per item plus hash-to-curve and the challenge hash, a recovery one double
multiplication plus a square root, an inversion mod n and one Keccak, so a recovery slower than the verify beside it means the multiplication path or the table stage is
wrong, not merely untuned.  Prints one JSON line and writes it to --out (default profiles/ecdsa_recover_timing.json); exits 1 when the bound is missed.
    python tests/gpu_debug/ecdsa_recover_timing.py [--n 1048576] [--reps 5] [--rounds 3] [--out FILE]"""
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

BOUND = 1.0
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--msg-len", type=int, default=32)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ecdsa_recover_timing.json"))
    a = ap.parse_args()
    n, L = a.n, a.msg_len
    eng = plume.Engine(0)
    rng = np.random.default_rng(1)
    msgs = rng.integers(0, 256, size=n * L + 16, dtype=np.uint8)
    off = (np.arange(n + 1, dtype=np.uint64) * L)
    sk = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    k = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    for x in (sk, k):
        x[:, 0] &= 0x7F
        x[:, 31] |= 1
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    dm, doff, dsk, dk = t(msgs), t(off.view(np.int64)), t(sk), t(k)
    pk, nul, c, s, rp, hr = (torch.zeros((n, w), dtype=torch.uint8, device=dev) for w in (64, 64, 32, 32, 64, 64))
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)                                  # a stream of its own: the events below are recorded on the stream the library runs on
    stream.wait_stream(torch.cuda.current_stream(dev))
    eng.sign_batch_device(1, n, dm, doff, len(msgs), dsk, dk, None, pk, nul, c, s, rp, hr, status, stream=stream)
    stream.synchronize()
    assert not bool(status.any())
    # the ECDSA signatures over random digests with the same keys and nonces, finished on the host
    R = rp.cpu().numpy()
    digest = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    es = np.zeros((n, 32), dtype=np.uint8)
    for i in range(n):
        r_i = int.from_bytes(R[i, :32].tobytes(), "big")
        assert 0 < r_i < N
        s_i = pow(int.from_bytes(k[i].tobytes(), "big"), -1, N) * (int.from_bytes(digest[i].tobytes(), "big") + r_i * int.from_bytes(sk[i].tobytes(), "big")) % N
        assert s_i
        es[i] = np.frombuffer(s_i.to_bytes(32, "big"), np.uint8)
    ev = (R[:, 63] & 1).astype(np.uint8)
    ev[::3] += 27
    dh, dr, ds, dv = t(digest), t(R[:, :32]), t(es), t(ev)
    qpk = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
    addr = torch.zeros((n, 20), dtype=torch.uint8, device=dev)
    st = torch.zeros(n, dtype=torch.uint8, device=dev)
    ok = torch.zeros(n, dtype=torch.uint8, device=dev)

    def recover():
        eng.ecdsa_recover_batch_device(n, dh, dr, ds, dv, None, qpk, addr, st, stream=stream)

    def verify():
        eng.verify_batch_device(1, n, dm, doff, len(msgs), pk, nul, c, s, rp, hr, ok, stream=stream)

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

    runs = {"recover": [], "verify": []}
    for _ in range(a.rounds):                                        # interleaved
        runs["recover"].append(timed(recover))
        runs["verify"].append(timed(verify))
    assert int(ok.sum()) == n and int((st == 1).sum()) == n
    assert torch.equal(qpk, pk)                                      # every recovered key is the signer's
    a1, s1 = eng.eth_address_batch(qpk[:4096].cpu().numpy())
    assert np.array_equal(a1, addr[:4096].cpu().numpy()) and (s1 == 1).all()
    eng.set_stage_timing(True)
    recover()
    stream.synchronize()
    stages = [(name, float(ms)) for name, ms in eng.last_stage_times()]
    eng.set_stage_timing(False)
    med = {key: statistics.median(v) for key, v in runs.items()}
    res = {"n": n, "msg_len": L, "version": eng.version(), "recover_ms": med["recover"], "verify_v1_ms": med["verify"], "all_ms": runs, "stages_ms": stages,
           "recover_over_verify": med["recover"] / med["verify"], "recoveries_per_s": n / (med["recover"] * 1e-3), "bound": BOUND}
    res["within_bound"] = res["recover_over_verify"] <= BOUND
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    eng.close()
    return 0 if res["within_bound"] else 1


if __name__ == "__main__":
    sys.exit(main())
