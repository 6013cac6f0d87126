"""k_eth_tx_parse beside its yardstick, and the sender call beside the recovery it ends in; one GPU, same process, HIP events through torch, median of --reps after
warm-up, in --rounds interleaved rounds, all on the same device-resident buffer of --n seeded signed transactions of a realistic mix (110 - 250 bytes; 60 % type 02,
30 % legacy EIP-155, the rest types 01, 03, 04 and unprotected legacy), built from --distinct signed items repeated:
  * plume_eth_tx_parse_batch_device, every output
  * plume_eth_message_hash_batch_device mode 0 over the same bytes: the yardstick -- it reads the same input and runs the same number of permutations to within one per
    item (it is also what gives the transaction ids)
  * plume_eth_tx_sender_batch_device
  * plume_ecdsa_recover_batch_device on the arrays the parse wrote
Prints one JSON line and writes it to --out (default profiles/eth_tx_timing.json).  parse_over_hash above about 2 means the kernel serialises on the byte walk over the
top-level items; sender_over_recover is what framing and hashing add to a recovery.  Not run by the suite.
    python tests/gpu_debug/eth_tx_timing.py [--n 1048576] [--distinct 512] [--reps 5] [--rounds 3] [--out FILE]"""
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
from tests import _ecdsa as E  # noqa: E402
from tests import _eth_tx as T  # noqa: E402


def workload(n, distinct, seed):
    rng = np.random.default_rng(seed)
    base = []
    for j in range(distinct):
        u = rng.random()
        typ, chain = (2, 1) if u < 0.6 else (0, 1) if u < 0.9 else ((1, 1), (3, 1), (4, 1), (0, 0))[int(rng.integers(4))]
        sk = E.b32(int.from_bytes(rng.bytes(32), "big") % (E.N - 1) + 1)
        raw = T.build(typ, sk, chain, rng.bytes(int(rng.integers(0, 100))), salt=2 * int(rng.integers(60)))[0]       # (an even salt: no access list)
        base.append((raw, T.sender_of(sk)[1]))
    pick = rng.integers(distinct, size=n)
    raws = [base[k][0] for k in pick]
    addr = np.frombuffer(b"".join(base[k][1] for k in pick), np.uint8).reshape(n, 20)
    lens = [len(r) for r in raws]
    return raws, addr, min(lens), max(lens), sum(lens) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--distinct", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "eth_tx_timing.json"))
    a = ap.parse_args()
    n = a.n
    raws, want_addr, lmin, lmax, lmean = workload(n, a.distinct, 1)
    txs, off = T.pack(raws)
    eng = plume.Engine(0)
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    dm, doff = t(txs), t(off.view(np.int64))
    nbytes = int(off[-1])
    z = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731
    h, r, s, v, typ, pst = z(n, 32), z(n, 32), z(n, 32), z(n), z(n), z(n)
    chain = torch.zeros(n, dtype=torch.int64, device=dev)
    txid = z(n, 32)
    pk, addr, st = z(n, 64), z(n, 20), z(n)
    pk2, addr2, st2 = z(n, 64), z(n, 20), z(n)
    stream = torch.cuda.Stream(dev)                                  # a stream of its own: the events below are recorded on the stream the library runs on
    stream.wait_stream(torch.cuda.current_stream(dev))

    def parse():
        eng.eth_tx_parse_batch_device(n, dm, doff, nbytes, h, r, s, v, chain, typ, pst, stream=stream)

    def hash0():
        eng.eth_message_hash_batch_device(n, dm, doff, nbytes, txid, mode="keccak256", stream=stream)

    def sender():
        eng.eth_tx_sender_batch_device(n, dm, doff, nbytes, None, pk, addr, chain, typ, st, low_s=True, stream=stream)

    def recover():
        eng.ecdsa_recover_batch_device(n, h, r, s, v, None, pk2, addr2, st2, low_s=True, stream=stream)

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

    runs = {k: [] for k in ("parse", "hash", "sender", "recover")}
    for _ in range(a.rounds):                                        # interleaved
        for k, fn in (("parse", parse), ("hash", hash0), ("sender", sender), ("recover", recover)):
            runs[k].append(timed(fn))
    assert int((pst == 1).sum()) == n and int((st == 1).sum()) == n and int((st2 == 1).sum()) == n
    assert torch.equal(addr, addr2) and torch.equal(pk, pk2) and np.array_equal(addr.cpu().numpy(), want_addr)      # every sender is the signer
    med = {k: statistics.median(x) for k, x in runs.items()}
    res = {"n": n, "distinct": a.distinct, "bytes_min": lmin, "bytes_max": lmax, "bytes_mean": lmean, "version": eng.version(), "parse_ms": med["parse"],
           "hash_keccak256_ms": med["hash"], "sender_ms": med["sender"], "recover_ms": med["recover"], "all_ms": runs,
           "parse_over_hash": med["parse"] / med["hash"], "sender_over_recover": med["sender"] / med["recover"], "senders_per_s": n / (med["sender"] * 1e-3),
           "parse_GB_per_s": nbytes / (med["parse"] * 1e-3) / 1e9}
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
