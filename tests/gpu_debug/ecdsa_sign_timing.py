"""plume_ecdsa_sign_batch_device and plume_eth_message_hash_batch_device on one GPU, same process, HIP events through torch, median of --reps after warm-up, in --rounds
interleaved rounds, on device-resident seeded keys and digests, at 2^14, 2^16 and 2^20 items (--sizes):
  * plume_ecdsa_sign_batch_device with the self-check off at uniform levels 1 and 2, and with the self-check on (level 1)
  * the yardsticks of the SAME run and the same n: plume_ecdsa_recover_batch_device (low s, every output) over the signatures the sign call just made -- every recovered
    key must be the pk the PLUME signer reports for the same sk -- and plume_sign_batch_rfc6979_device version 2 over 32-byte messages
  * per-stage splits from plume_last_stage_times (one more call each with stage timing on, outside the timed ones)
  * k_eth_message_hash at 2^20 messages of 32 bytes and at 2^20 ragged messages of 0 .. 300 bytes, both modes
A sign call does one comb multiplication and one inversion mod n per item where a recovery does a table build and a 65-position chain: sign_over_recover says how the two
compare on this run.  Prints one JSON line and writes it to --out (default profiles/ecdsa_sign_timing.json).
    python tests/gpu_debug/ecdsa_sign_timing.py [--sizes 16384,65536,1048576] [--reps 5] [--rounds 3] [--out FILE]"""
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
    ap.add_argument("--sizes", default="16384,65536,1048576")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ecdsa_sign_timing.json"))
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",")]
    eng = plume.Engine(0)
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    stream = torch.cuda.Stream(dev)                                  # a stream of its own: the events below are recorded on the stream the library runs on
    stream.wait_stream(torch.cuda.current_stream(dev))

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

    def stages_of(fn):
        eng.set_stage_timing(True)
        fn()
        stream.synchronize()
        out = [(name, float(ms)) for name, ms in eng.last_stage_times()]
        eng.set_stage_timing(False)
        return out

    def configured(level, selfcheck, fn):
        def run():
            eng.set_sign_uniform(level)
            eng.set_sign_selfcheck(selfcheck)
            fn()
        return run

    res = {"version": eng.version(), "reps": a.reps, "rounds": a.rounds, "sizes": {}}
    for n in sizes:
        rng = np.random.default_rng(n)
        sk = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        sk[:, 0] &= 0x7F
        sk[:, 31] |= 1
        digest = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        msgs = np.concatenate([digest.reshape(-1), np.zeros(16, np.uint8)])
        off = np.arange(n + 1, dtype=np.uint64) * 32
        dh, dsk, dm, doff = t(digest), t(sk), t(msgs), t(off.view(np.int64))
        r, s = (torch.zeros((n, 32), dtype=torch.uint8, device=dev) for _ in range(2))
        v, st = (torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(2))
        qpk, addr, rst = torch.zeros((n, 64), dtype=torch.uint8, device=dev), torch.zeros((n, 20), dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
        pk, nul, rp, hr = (torch.zeros((n, 64), dtype=torch.uint8, device=dev) for _ in range(4))
        pc, ps = (torch.zeros((n, 32), dtype=torch.uint8, device=dev) for _ in range(2))
        pst = torch.zeros(n, dtype=torch.uint8, device=dev)

        def sign():
            eng.ecdsa_sign_batch_device(n, dh, dsk, None, r, s, v, st, v27=True, stream=stream)

        def recover():
            eng.ecdsa_recover_batch_device(n, dh, r, s, v, None, qpk, addr, rst, low_s=True, stream=stream)

        def plume_sign():
            eng.sign_batch_rfc6979_device(2, n, dm, doff, len(msgs), dsk, None, None, pk, nul, pc, ps, rp, hr, pst, stream=stream)

        cases = {"sign_level1": configured(1, 0, sign), "sign_level2": configured(2, 0, sign), "sign_selfcheck_level1": configured(1, 1, sign),
                 "ecdsa_recover": recover, "plume_sign_rfc6979_v2": configured(1, 0, plume_sign)}
        runs = {k: [] for k in cases}
        for _ in range(a.rounds):                                    # interleaved
            for k, fn in cases.items():
                runs[k].append(timed(fn))
        eng.set_sign_selfcheck(0)
        eng.set_sign_uniform(1)
        # what was timed is right: every item signed, every signature recovers to the pk the PLUME signer reports for the same sk
        sign(); recover(); plume_sign()
        stream.synchronize()
        assert not bool(st.any()) and int((rst == 1).sum()) == n and not bool(pst.any()) and torch.equal(qpk, pk)
        med = {k: statistics.median(x) for k, x in runs.items()}
        res["sizes"][str(n)] = {"ms": med, "all_ms": runs, "sign_over_recover": med["sign_level1"] / med["ecdsa_recover"], "signatures_per_s": n / (med["sign_level1"] * 1e-3),
                                "stages_ms": {k: stages_of(cases[k]) for k in ("sign_level1", "sign_level2", "sign_selfcheck_level1", "ecdsa_recover")}}
        eng.set_sign_selfcheck(0)
        eng.set_sign_uniform(1)
        del dh, dsk, dm, doff, r, s, v, st, qpk, addr, rst, pk, nul, rp, hr, pc, ps, pst
        torch.cuda.empty_cache()

    # the message hash: 2^20 messages of 32 bytes, and 2^20 ragged messages of 0 .. 300 bytes
    n = 1 << 20
    rng = np.random.default_rng(7)
    hashes = {}
    for name, lens in (("32_bytes", np.full(n, 32, dtype=np.int64)), ("ragged_0_300", rng.integers(0, 301, size=n, dtype=np.int64))):
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        nbytes = int(off[-1])
        dm, doff = t(rng.integers(0, 256, size=nbytes + 16, dtype=np.uint8)), t(off.view(np.int64))
        out = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        for mode in ("keccak256", "eip191"):
            fn = lambda: eng.eth_message_hash_batch_device(n, dm, doff, nbytes, out, mode=mode, stream=stream)  # noqa: E731
            ms = statistics.median(timed(fn) for _ in range(a.rounds))
            hashes[f"{name}_{mode}"] = {"ms": ms, "bytes": nbytes, "messages_per_s": n / (ms * 1e-3), "GB_per_s": nbytes / (ms * 1e-3) / 1e9}
    res["message_hash_2^20"] = hashes
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
