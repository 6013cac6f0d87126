"""DistributedNullifierSet (zk-nullifier-sig_amd/nullifier_set.py) over gloo on the CPU: several rounds of inserts from every rank, with repeats within a rank, across
ranks and across rounds, must give each rank exactly the flags one global set would give its items (ids: rank offset + position), and the global count.  The local sets
are a test double with NullifierSet's device-form signature that answers from a Python set."""
import os
import random

import numpy as np
import pytest


class SetDouble:
    """stand-in for zk_nullifier_sig_amd.NullifierSet on CPU tensors (test infrastructure): a Python set of records and the definition of `fresh`"""
    def __init__(self):
        self.S = set()

    def insert_device(self, n, nullifier, live, ids, fresh, n_fresh=None, stream=None):
        import torch
        recs = [bytes(r) for r in nullifier.numpy().reshape(n, 64)]
        lv = [1] * n if live is None else live.numpy().tolist()
        idv = list(range(n)) if ids is None else ids.numpy().tolist()
        best = {}
        for i in range(n):
            if lv[i] and (recs[i] not in best or idv[i] < best[recs[i]]):
                best[recs[i]] = idv[i]
        f = [1 if lv[i] and recs[i] not in self.S and best[recs[i]] == idv[i] else 0 for i in range(n)]
        self.S |= set(best)
        fresh.copy_(torch.tensor(f, dtype=torch.uint8))
        if n_fresh is not None:
            n_fresh.fill_(sum(f))

    def contains_device(self, n, nullifier, found, stream=None):
        import torch
        found.copy_(torch.tensor([1 if bytes(r) in self.S else 0 for r in nullifier.numpy().reshape(n, 64)], dtype=torch.uint8))

    def __len__(self):
        return len(self.S)


def _rounds(seed, rounds=4, per_rank=(0, 1, 37, 400)):
    """per round: the global batch (records drawn from a shared pool) and live flags; rank r takes a contiguous slice"""
    rng = random.Random(seed)
    pool = [bytes(rng.randrange(256) for _ in range(64)) for _ in range(600)] + [bytes(64)]
    out = []
    for k in range(rounds):
        total = per_rank[k % len(per_rank)] * 3 + 11 * k
        recs = [pool[rng.randrange(len(pool))] for _ in range(total)]
        live = [0 if rng.random() < 0.2 else 1 for _ in range(total)]
        out.append((recs, live))
    return out


def _global(rounds):
    S, res = set(), []
    for recs, live in rounds:
        seen, f = set(), []
        for r, lv in zip(recs, live):
            fr = bool(lv) and r not in S and r not in seen
            if lv:
                seen.add(r)
            f.append(1 if fr else 0)
        S |= seen
        res.append((f, sum(f)))
    return res, len(S)


def _worker(rank, world, port, seed, out):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import zk_nullifier_sig_amd.nullifier_set as NS
        ds = NS.DistributedNullifierSet(SetDouble())
        got = []
        for recs, live in _rounds(seed):
            lo, hi = (len(recs) * rank) // world, (len(recs) * (rank + 1)) // world
            nul = torch.from_numpy(np.frombuffer(b"".join(recs[lo:hi]), dtype=np.uint8).reshape(hi - lo, 64).copy())
            lv = torch.tensor(live[lo:hi], dtype=torch.uint8)
            fresh, cnt = ds.insert(nul, lv)
            got.append((fresh.tolist(), cnt, ds.contains(nul).tolist()))
        out[rank] = (got, len(ds))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3, 8])
def test_distributed_set_equals_one_global_set(world):
    import torch.multiprocessing as mp
    seed = 77 + world
    rounds = _rounds(seed)
    want, want_size = _global(rounds)
    with mp.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_worker, args=(world, 29750 + world, seed, out), nprocs=world, join=True)
        res = {r: out[r] for r in range(world)}
    for k, ((f_want, c_want), (recs, live)) in enumerate(zip(want, rounds)):
        flags, found = [], []
        for r in range(world):
            f, c, fd = res[r][0][k]
            assert c == c_want, (k, r)
            flags += f
            found += fd
        assert flags == f_want, k
        members = {x for rr, ll in rounds[:k + 1] for x, l in zip(rr, ll) if l}          # the set after round k
        assert found == [int(rec in members) for rec in recs], k
    for r in range(world):
        assert res[r][1] == want_size

