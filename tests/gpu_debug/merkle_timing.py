"""The Merkle calls stage by stage; one GPU, one process, HIP events through torch on the stream the library runs on, median of --reps after warm-up, in --rounds
interleaved rounds, for n = 2^10, 2^16, 2^20 seeded addresses (device-resident, 20 raw bytes each):
  * leaf:    plume_merkle_leaf_batch_device, ADDRESS leaves (two permutations per item)
  * build:   plume_merkle_tree_build_device sorted and in input order, whole calls; and with stage timing on, the stages of the sorted call one by one -- merkle_sort,
             merkle_place, merkle_levels (one launch per depth of more than 256 parents), merkle_top (the depths above in one launch).  An event between two stages costs a
             few microseconds of idle GPU, so the stages add up to more than the call
  * top:     at every n, the input-order build with the fused top and with PLUME_MERKLE_FUSED_TOP=0 (one k_merkle_level launch per depth all the way up), interleaved: at
             n = 2^10 that is 1 + 1 launches against 10
  * proof:   plume_merkle_proof_batch_device for all n leaves;  verify: plume_merkle_verify_batch_device of those n proofs from the addresses
  * yardstick: plume_eth_message_hash_batch_device mode 0 over n - 1 messages of 64 bytes -- the level stage's n - 1 one-block Keccaks through the keccak_stream kernel --
             in the same process; the figure of profiles/eth_address_timing.json (2^20 one-block Keccaks behind a curve check, another run) is copied beside it
Checks while it runs: every verify status is 1, and both top forms give the same root.  Prints one JSON line and writes it to --out (default
profiles/merkle_timing.json).  Not run by the suite.
    python tests/gpu_debug/merkle_timing.py [--sizes 1024,65536,1048576] [--reps 7] [--rounds 3] [--out FILE]"""
import argparse
import json
import os
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
    ap.add_argument("--sizes", default="1024,65536,1048576")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "merkle_timing.json"))
    a = ap.parse_args()
    eng = plume.Engine(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    z = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)  # noqa: E731

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

    sizes = []
    for n in (int(x) for x in a.sizes.split(",")):
        rng = np.random.default_rng(n)
        addr = torch.from_numpy(rng.integers(0, 256, (n, 20), dtype=np.uint8)).to(dev)
        depth = eng.merkle_max_proof_len(n)
        leaf, lst, tree, tree2, proof, ln, vst = z(n, 32), z(n), z(2 * n - 1, 32), z(2 * n - 1, 32), z(n, depth, 32), z(n), z(n)
        pos = torch.zeros(n, dtype=torch.int32, device=dev)
        pairs, poff, digest = z(64 * (n - 1) + 16), torch.arange(n, dtype=torch.int64, device=dev) * 64, z(n - 1, 32)

        def build(sort, out=tree):
            eng.merkle_tree_build_device(n, leaf, out, pos, sort, stream=stream)

        def top(fused):
            os.environ["PLUME_MERKLE_FUSED_TOP"] = "1" if fused else "0"
            try:
                eng.merkle_tree_build_device(n, leaf, tree2, None, False, stream=stream)
            finally:
                os.environ.pop("PLUME_MERKLE_FUSED_TOP", None)

        calls = {"leaf": lambda: eng.merkle_leaf_batch_device(n, addr, None, leaf, lst, "address", "raw20", stream=stream),
                 "build_sorted": lambda: build(True), "build_input_order": lambda: build(False), "input_order_fused_top": lambda: top(True),
                 "input_order_level_per_depth": lambda: top(False),
                 "proof_all_leaves": lambda: eng.merkle_proof_batch_device(n, tree, n, pos, depth, proof, ln, stream=stream),
                 "verify_n_proofs": lambda: eng.merkle_verify_batch_device(n, addr, None, depth, proof, ln, tree, vst, "address", "raw20", stream=stream),
                 "keccak_stream_n_minus_1_blocks": lambda: eng.eth_message_hash_batch_device(n - 1, pairs, poff, 64 * (n - 1), digest, mode="keccak256", stream=stream)}
        runs = {k: [] for k in calls}
        stages = {}
        for _ in range(a.rounds):                                      # interleaved; build_sorted before proof and verify, which read its tree and leaf_pos
            for k, fn in calls.items():
                if k == "input_order_level_per_depth":
                    top(False)
                    torch.cuda.synchronize()
                    unfused_root = tree2[0].clone()
                if k == "proof_all_leaves":
                    build(True)
                runs[k].append(timed(fn))
            eng.set_stage_timing(True)
            try:
                for _ in range(a.reps):
                    build(True, tree2)
                    torch.cuda.synchronize()
                    for name, ms in eng.last_stage_times():
                        stages.setdefault(name, []).append(ms)
            finally:
                eng.set_stage_timing(False)
        assert int((vst == 1).sum()) == n and int((lst == 1).sum()) == n
        top(True)
        torch.cuda.synchronize()
        assert torch.equal(tree2[0], unfused_root)
        med = {k: statistics.median(v) for k, v in runs.items()}
        sizes.append({"n": n, "depth": depth, "ms": med, "sorted_build_stage_ms": {k: statistics.median(v) for k, v in stages.items()}, "all_ms": runs,
                      "fused_top_over_level_per_depth": med["input_order_fused_top"] / med["input_order_level_per_depth"],
                      "level_hashes": n - 1, "input_order_build_over_keccak_stream": med["build_input_order"] / med["keccak_stream_n_minus_1_blocks"],
                      "leaves_per_s_sorted_build": n / (med["build_sorted"] * 1e-3), "proofs_verified_per_s": n / (med["verify_n_proofs"] * 1e-3)})
    ref = json.loads((ROOT / "profiles" / "eth_address_timing.json").read_text())
    res = {"version": eng.version(), "reps": a.reps, "rounds": a.rounds, "sizes": sizes,
           "eth_address_timing_json": {"n": ref["n"], "eth_raw20_ms": ref["eth_raw20_ms"], "version": ref["version"]}}
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
