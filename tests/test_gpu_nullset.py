"""The persistent nullifier set on the MI355X (include/plume_hip.h, plume_nullset_*; kernels in csrc/plume_nullset_kernels.hip): every answer against the definition
-- first-occurrence marking over every live item of every earlier insert followed by this call's items, restricted to this call -- computed both in Python and with the
engine's own plume_nullifier_first_occurrence on the concatenation; real nullifiers through "verify, then admit" on one stream; two caller streams; a multi-device
context; argument errors; the C++ façade.  Sets stay <= 2^23 records."""
import ctypes as C
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import zk_nullifier_sig_amd as plume
    return plume.default_engine()


def _pool(k, seed):
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 256, size=(k, 64), dtype=np.uint8)
    pool[0] = 0                                     # the identity is an ordinary record
    pool[2] = pool[1]
    pool[2, 63] ^= 1                                # differs in the last byte only
    return pool


def _expected(history, recs, live, ids):
    """fresh flags by the definition: live, not in `history` (a Python set, updated), smallest id among this call's live items with the record"""
    keys = [r.tobytes() for r in recs]
    best = {}
    for i, k in enumerate(keys):
        if live[i] and (k not in best or ids[i] < best[k]):
            best[k] = ids[i]
    fresh = np.array([1 if live[i] and keys[i] not in history and best[keys[i]] == ids[i] else 0 for i in range(len(keys))], dtype=np.uint8)
    history.update(best)
    return fresh


def test_insert_sequences_match_the_definition(eng):
    s = eng.nullifier_set(0)
    pool = _pool(1 << 20, 5)
    history, admitted = set(), []                   # admitted: every live record of every earlier insert, in order
    rng = np.random.default_rng(11)
    caps = []
    for k, n in enumerate([1, 65, 4096, 1 << 17, 1 << 20, 4096]):
        recs = pool[rng.integers(0, min(len(pool), 2 * n + 64), size=n)]
        live = (rng.random(n) > 0.15).astype(np.uint8) if k % 2 else np.ones(n, dtype=np.uint8)
        ids = ((1 << 62) - 3 * np.arange(n, dtype=np.uint64)).astype(np.uint64)     # reversed 64-bit ids: the last of several equal records wins
        fresh, cnt = s.insert(recs, live if k % 2 else None, ids)
        want = _expected(history, recs, live, ids)
        assert np.array_equal(fresh, want), (n, int(np.count_nonzero(fresh != want)))
        assert cnt == int(want.sum()) and len(s) == len(history)
        # the same flags from the engine's first-occurrence pass over everything admitted so far followed by this call (earlier items get the smaller ids)
        prev = np.concatenate(admitted) if admitted else np.zeros((0, 64), dtype=np.uint8)
        m = len(prev)
        order = np.argsort(ids, kind="stable")
        rank = np.empty(n, dtype=np.uint64)
        rank[order] = np.arange(n, dtype=np.uint64)
        first, _ = eng.nullifier_first_occurrence(np.concatenate([prev, recs]), np.concatenate([np.ones(m, np.uint8), live]),
                                                  np.concatenate([np.arange(m, dtype=np.uint64), m + rank]))
        assert np.array_equal(first[m:], fresh), n
        admitted.append(recs[live.astype(bool)])
        caps.append(s.capacity)
        assert 2 * len(s) <= caps[-1]
        # contains: everything admitted, plus records never inserted
        probe = np.concatenate([recs[:4096], _pool(64, 1000 + k)[3:]])
        assert np.array_equal(s.contains(probe), np.array([1 if r.tobytes() in history else 0 for r in probe], dtype=np.uint8))
    assert len(set(caps)) >= 3                      # grew several times from reserve=0
    s.close()


def test_export_into_a_new_set_and_clear(eng):
    pool = _pool(50000, 9)
    with eng.nullifier_set(100) as s:
        s.insert(pool[:30000])
        s.insert(pool[20000:], np.arange(30000) % 3 != 0)
        want = {r.tobytes() for r in pool[:30000]} | {r.tobytes() for i, r in enumerate(pool[20000:]) if i % 3 != 0}
        out = s.export()
        assert out.shape == (len(want), 64) and {r.tobytes() for r in out} == want
        with eng.nullifier_set() as t:
            fresh, cnt = t.insert(out)
            assert cnt == len(want) and fresh.all()
            assert np.array_equal(t.contains(pool), s.contains(pool))
        cap = s.capacity
        s.clear()
        assert len(s) == 0 and s.capacity == cap and not s.contains(pool).any() and s.export().shape == (0, 64)
        fresh, cnt = s.insert(pool[:10])
        assert cnt == 10


def test_verify_then_admit_on_one_stream(eng):
    """signed batches whose (sk, message) pairs repeat within and across batches; verify_batch_device, then insert_device(live = ok) on the same stream, no host round trip"""
    import torch
    from tests import synth
    n, pairs = 4096, 3000
    base = synth.sign_inputs(pairs, start=50000)
    dev = torch.device("cuda", eng.device_id)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    st = torch.cuda.Stream(dev)                      # (torch's default stream is handle 0, which the library reads as "the context's / the set's own stream")
    with eng.nullifier_set(0) as s:
        seen = set()
        for b in range(3):
            p = (np.arange(n) * 7 + 1000 * b) % pairs          # pair of item i: repeats inside the batch (n > pairs) and across batches
            x = synth.sign_inputs(n, start=10000 * (b + 1))    # fresh nonces
            x["sk"] = base["sk"][p].copy()
            msgs = base["msgs"][:32 * pairs].reshape(pairs, 32)[p]
            x["msgs"] = np.concatenate([msgs.reshape(-1), np.zeros(16, np.uint8)])
            signed = eng.sign_batch(1, x["msgs"], x["off"], x["sk"], x["r"])
            nul = signed["nullifier"].copy()
            bad = np.arange(n) % 13 == 3
            nul[bad, 5] ^= 1                                   # corrupted: verify fails, and the record is one no honest item has
            d = {k: t(signed[k]) for k in ("pk", "c", "s", "r_point", "hashed_to_curve_r")}
            dn, ok, fresh, cnt = t(nul), torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
            dm, do = t(x["msgs"]), t(x["off"].view(np.int64))
            torch.cuda.synchronize()
            eng.verify_batch_device(1, n, dm, do, 32 * n, d["pk"], dn, d["c"], d["s"], d["r_point"], d["hashed_to_curve_r"], ok, stream=st)
            s.insert_device(n, dn, ok, None, fresh, cnt, stream=st)      # behind the verify on the same stream: no host round trip
            st.synchronize()
            assert np.array_equal(ok.cpu().numpy(), (~bad).astype(np.uint8))
            want = np.zeros(n, dtype=np.uint8)
            for i in range(n):
                if not bad[i] and p[i] not in seen:
                    want[i] = 1
                    seen.add(p[i])
            # items of one pair share a nullifier: fresh = first honest occurrence of the pair, ever
            assert np.array_equal(fresh.cpu().numpy(), want) and int(cnt.item()) == int(want.sum())
            assert not s.contains(nul[bad]).any()
            assert s.contains(signed["nullifier"][~bad]).all()
        assert len(s) == len(seen)


def test_device_forms_on_two_streams_are_serialised(eng):
    import torch
    dev = torch.device("cuda", eng.device_id)
    pool = _pool(1 << 16, 21)
    rng = np.random.default_rng(3)
    calls = [pool[rng.integers(0, len(pool), size=n)] for n in (1 << 16, 1 << 15, 1 << 16, 333)]
    history = set()
    wants = [_expected(history, c, np.ones(len(c), np.uint8), np.arange(len(c))) for c in calls]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    with eng.nullifier_set(0) as s:
        ins = [torch.from_numpy(c).to(dev) for c in calls]
        outs = [torch.zeros(len(c), dtype=torch.uint8, device=dev) for c in calls]
        cnts = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in calls]
        found = torch.zeros(len(calls[0]), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        for k, c in enumerate(calls):
            s.insert_device(len(c), ins[k], None, None, outs[k], cnts[k], stream=streams[k % 2])
        s.contains_device(len(calls[0]), ins[0], found, stream=streams[1])
        torch.cuda.synchronize()
        for k in range(len(calls)):
            assert np.array_equal(outs[k].cpu().numpy(), wants[k]), k
            assert int(cnts[k].item()) == int(wants[k].sum())
        assert found.cpu().numpy().all() and len(s) == len(history)


def test_multi_device_context_and_outliving_the_context():
    import zk_nullifier_sig_amd as plume
    e = plume.Engine([0, 0])
    s = e.nullifier_set()
    e.close()                                        # the set lives on the first shard's device and does not need its context
    pool = _pool(5000, 31)
    fresh, cnt = s.insert(np.concatenate([pool, pool[:100]]))
    assert cnt == 5000 and fresh[:5000].all() and not fresh[5000:].any()
    assert s.contains(pool).all() and len(s) == 5000
    s.close()


def test_argument_errors(eng):
    import torch
    import zk_nullifier_sig_amd as plume
    from zk_nullifier_sig_amd import capi
    lib = capi._load()
    rec, out, cnt = np.zeros(64, np.uint8), np.zeros(1, np.uint8), C.c_uint64(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.plume_nullset_insert(None, 1, p(rec), None, None, p(out), C.byref(cnt)) == -1
    assert lib.plume_nullset_contains(None, 1, p(rec), p(out)) == -1
    h = C.c_void_p()
    assert lib.plume_nullset_create(eng._ctx, (1 << 31) + 1, C.byref(h)) == -1 and not h.value
    with eng.nullifier_set() as s:
        assert lib.plume_nullset_insert(s._h, 1, None, None, None, p(out), C.byref(cnt)) == -1
        assert lib.plume_nullset_insert(s._h, 1, p(rec), None, None, None, C.byref(cnt)) == -1
        assert lib.plume_nullset_export(s._h, 0, None, None) == -1
        tiny = torch.zeros(64, dtype=torch.uint8, device=torch.device("cuda", eng.device_id))
        with pytest.raises(plume.PlumeHipError, match=r"\(-1\)"):
            s.insert_device((1 << 30) + 1, tiny, None, None, tiny)
        with pytest.raises(plume.PlumeHipError, match=r"\(-1\)"):
            s.contains_device((1 << 30) + 1, tiny, tiny)
        with pytest.raises(plume.PlumeHipError, match=r"\(-1\)"):
            s.reserve((1 << 31) + 1)
        assert s.capacity == 64 and len(s) == 0                # nothing was allocated or changed
        s.insert(np.ones((3, 64), np.uint8))
        assert len(s) == 1
    with pytest.raises(plume.PlumeHipError):
        eng.nullifier_set((1 << 31) + 1)


def test_cpp_facade(tmp_path):
    import zk_nullifier_sig_amd as plume
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "nullset_test"
    libdir = plume.library_path().parent
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", str(root / "include"), str(root / "tests" / "abi_cpp" / "nullset_test.cpp"), "-L", str(libdir),
                    "-lplume_hip", f"-Wl,-rpath,{libdir}", "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "nullset_test ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
