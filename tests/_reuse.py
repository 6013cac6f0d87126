"""One table of calls for the tests that ask whether a call's result depends on what its context ran before (tests/test_gpu_context_reuse.py on the GPU,
tests/test_context_reuse.py for the runner itself).  Nothing here needs a GPU to import or to build the table: an entry holds a family's inputs at one size, what the
existing CPU restatements say of them, and a callable that makes the call on an engine in its host-pointer or its device-resident form.

Sizes: 321 items (one 256-lane workgroup, one 64-lane wavefront and one lane) and 65.  Every entry plants its family's invalid items; the planted positions of the two
sizes are disjoint (i % 7 == 3 at 321, i % 7 == 5 at 65, and each size's last item), so a flag or status byte left behind by the other size is a wrong one.

The device forms write into tensors pre-filled with 0xAA, so an output the call never wrote differs from every expected byte pattern that matters here."""
import hashlib

import numpy as np

LARGE, SMALL = 321, 65
FILL = 0xAA
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
AGG_SEED = hashlib.sha256(b"context reuse aggregate seed").digest()
SIGN_KEYS = ("pk", "nullifier", "c", "s", "r_point", "hashed_to_curve_r", "status")
VERIFY, ECDSA, ARMED = "verify", "ecdsa", "armed"          # what a call leaves in the context's redo list (plume_last_redo_tasks): the verifier's counters of a batch that
                                                           # files no task, another family's list, or the counters of a self-checked sign call (its planted r = 0 items may file tasks)


def bad_positions(n):
    """the planted invalid positions of a size, never shared between LARGE and SMALL: one residue of 7 each, and the last item (the lone lane of the last wavefront)"""
    i = np.arange(n)
    return np.flatnonzero((i % 7 == (3 if n >= LARGE else 5)) | (i == n - 1))


def _b32(v):
    return np.frombuffer(int(v).to_bytes(32, "big"), np.uint8)


# ---------------------------------------------------------------------------------------------------- device-form plumbing
class Pending:
    """a call that has been made: the host form's outputs (host), or the tensors an enqueued device-form call reads and writes, alive until collect()"""

    def __init__(self, eng=None, stream=None, host=None):
        self.keep, self.outs, self.host = [], {}, host
        if host is not None:
            return
        import torch
        self.torch, self.eng = torch, eng
        self.dev = torch.device("cuda", eng.device_id)
        self.stream = stream                               # a torch stream of the caller's, or None: the context's own stream (the NULL handle)

    def up(self, a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint64:
            a = a.view(np.int64)
        elif a.dtype == np.uint32:
            a = a.view(np.int32)
        t = self.torch.from_numpy(a.copy()).to(self.dev)
        self.keep.append(t)
        return t

    def out(self, name, shape, dtype=np.uint8):
        shape = (shape,) if np.isscalar(shape) else tuple(shape)
        nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        t = self.torch.full((max(nbytes, 1),), FILL, dtype=self.torch.uint8, device=self.dev)
        self.outs[name] = (t, nbytes, shape, np.dtype(dtype))
        return t

    def tensor(self, name):
        return self.outs[name][0]

    def ready(self):
        """everything uploaded and filled is ordered in front of the call: the caller's stream waits for torch's; the context's own stream is ordered by a synchronise"""
        if self.stream is None:
            self.torch.cuda.synchronize(self.dev)
        else:
            self.stream.wait_stream(self.torch.cuda.current_stream(self.dev))
        return self.stream

    def collect(self, sync=True):
        if self.host is not None:
            return self.host
        if sync:
            if self.stream is None:
                self.torch.cuda.synchronize(self.dev)
            else:
                self.stream.synchronize()
        got = {k: t.cpu().numpy()[:nbytes].view(dt).reshape(shape).copy() for k, (t, nbytes, shape, dt) in self.outs.items()}
        self.keep, self.outs = [], {}
        return got


class Entry:
    """family, n, the inputs, expected (name -> array; expected_device where the device form is given other inputs), host(eng, inputs) -> dict and
    device(eng, inputs, pending) which enqueues on pending.ready().  status: the names of the per-item status arrays.  redo: what the call leaves in the redo list --
    VERIFY, ECDSA, None, or a callable of the engine's self-check setting"""

    def __init__(self, family, n, inputs, expected, host, device=None, status=("status",), redo=None, expected_device=None):
        self.family, self.n, self.inputs, self.expected, self.host, self.device = family, n, inputs, expected, host, device
        self.status, self.redo, self.expected_device = tuple(status), redo, expected_device
        self.name = f"{family}[{n}]"

    def want(self, device):
        return self.expected_device if device and self.device is not None and self.expected_device is not None else self.expected

    def redo_after(self, selfcheck):
        return self.redo(selfcheck) if callable(self.redo) else self.redo

    def enqueue(self, engine, device, stream):
        if not (device and self.device is not None):
            return Pending(host=self.host(engine, self.inputs))
        p = Pending(engine, stream)
        self.device(engine, self.inputs, p)
        return p

    def run(self, engine, device, stream):
        answer = getattr(engine, "answer", None)          # a fake engine of the harness's self-test answers for itself
        if answer is not None:
            return answer(self, device)
        return self.enqueue(engine, device, stream).collect()


def differences(entry, got, device):
    """the names of the outputs that differ from the expected arrays in any byte (shape and dtype included); empty: the call is right"""
    want = entry.want(device)
    bad = [k for k in want if k not in got or got[k].shape != want[k].shape or got[k].dtype != want[k].dtype or not np.array_equal(got[k], want[k])]
    return bad + [k for k in got if k not in want]


def describe(entry, got, device):
    want = entry.want(device)
    out = []
    for k in differences(entry, got, device):
        if k in got and k in want and got[k].shape == want[k].shape:
            rows = np.flatnonzero((got[k].reshape(len(want[k]), -1) != want[k].reshape(len(want[k]), -1)).any(axis=1)) if want[k].ndim and len(want[k]) else []
            out.append(f"{k}: {len(rows)} rows differ, first {[int(x) for x in rows[:6]]}")
        else:
            out.append(f"{k}: shape/dtype {None if k not in got else (got[k].shape, got[k].dtype)} != {None if k not in want else (want[k].shape, want[k].dtype)}")
    return "; ".join(out)


# ---------------------------------------------------------------------------------------------------- the runner
class Step:
    def __init__(self, entry, device=False, stream=None, settings=None):
        self.entry, self.device, self.stream, self.settings = entry, device, stream, dict(settings or {})

    def label(self):
        s = "".join(f" {k}={v}" for k, v in sorted(self.settings.items()))
        return f"{self.entry.name} ({'device' if self.device else 'host'} form, stream {self.stream if not hasattr(self.stream, 'cuda_stream') else hex(self.stream.cuda_stream)}{s})"


SETTERS = {"selfcheck": "set_sign_selfcheck", "eq1_short": "set_eq1_short", "sign_uniform": "set_sign_uniform", "stage_timing": "set_stage_timing"}


class Leak(AssertionError):
    """a call whose outputs differ from those of a context that has done nothing else"""

    def __init__(self, index, step, previous, detail, seed=None):
        self.index, self.step, self.previous, self.detail, self.seed = index, step, previous, detail, seed
        super().__init__(f"seed {seed}, call {index}: {step.label()} differs from the fresh-context result after {previous.label() if previous else 'nothing'}: {detail}")


def run_steps(engine, steps, seed=None, check_redo=True, lanes=False):
    """the steps in order on one engine, every output byte of every call compared; raises Leak naming the first call that differs.  check_redo: plume_last_redo_tasks
    after every call whose context's redo list is known -- 0 behind a verify call (the count tests/test_gpu_round6.py asserts for inputs without its crafted items), an
    error behind an ECDSA-family call.  lanes: the engine deals device calls out to lanes, so only a device-form call's own lane is known"""
    state, selfcheck, previous = None, 0, None
    for index, step in enumerate(steps):
        for k, v in step.settings.items():
            getattr(engine, SETTERS[k])(v)
            if k == "selfcheck":
                selfcheck = v
        got = step.entry.run(engine, step.device, step.stream)
        if differences(step.entry, got, step.device):
            raise Leak(index, step, previous, describe(step.entry, got, step.device), seed)
        effect = step.entry.redo_after(selfcheck)
        if not lanes:
            state = effect or state
        known = (effect if step.device and step.entry.device is not None else None) if lanes else state
        if check_redo and known is not None and hasattr(engine, "last_redo_tasks"):
            try:
                count = engine.last_redo_tasks()
            except Exception as e:                         # PlumeHipError: the redo list is another family's
                count = e
            if known == VERIFY and count != 0:
                raise Leak(index, step, previous, f"plume_last_redo_tasks gave {count!r} behind a verify call of honest and corrupted items (0 expected)", seed)
            if known == ARMED and not (isinstance(count, int) and count >= 0):
                raise Leak(index, step, previous, f"plume_last_redo_tasks gave {count!r} behind a self-checked sign call (a count expected: its check is a verify call)", seed)
            if known == ECDSA and not (isinstance(count, Exception) and "another family" in str(count)):
                raise Leak(index, step, previous, f"plume_last_redo_tasks gave {count!r} behind an ECDSA-family call (an error expected: the list is not the verifier's)", seed)
        previous = step
    return len(steps)


def walk(table, seed, calls, streams, forms=(False, True), settings=True):
    """a seeded walk over all entries: before each call the form, the stream (one of `streams`: caller streams and None for the context's own), the self-check, the
    form of equation 1, the signer's schedule and stage timing are drawn"""
    rng = np.random.default_rng(seed)
    entries = [e for fam in table.values() for e in fam.values()]
    steps = []
    for _ in range(calls):
        e = entries[int(rng.integers(len(entries)))]
        st = {}
        if settings:
            st = {"selfcheck": int(rng.integers(2)), "eq1_short": (0, 1, 3)[int(rng.integers(3))], "sign_uniform": int(rng.integers(3)), "stage_timing": bool(rng.integers(2))}
        steps.append(Step(e, bool(forms[int(rng.integers(len(forms)))]), streams[int(rng.integers(len(streams)))], st))
    return steps


# ---------------------------------------------------------------------------------------------------- inputs the PLUME families share
def _plume_signed(n, version, start):
    from tests import _oracle_c as OC
    from tests import synth
    b = synth.sign_inputs(n, start=start)
    return b, OC.sign_batch(version, b["msgs"], b["off"], b["sk"], b["r"], nthreads=8)


def _plume_corrupted(n, version, start):
    """a verify batch with its planted items: a flipped s, c = n (no scalar), a pk off the curve, a neighbour's nullifier -- in turn"""
    b, sg = _plume_signed(n, version, start)
    v = dict(msgs=b["msgs"], off=b["off"], **{k: sg[k].copy() for k in ("pk", "nullifier", "c", "s", "r_point", "hashed_to_curve_r")})
    for j, i in enumerate(bad_positions(n)):
        kind = j % 4
        if kind == 0:
            v["s"][i, 31] ^= 1
        elif kind == 1:
            v["c"][i] = _b32(N)
        elif kind == 2:
            v["pk"][i, 63] ^= 1
        else:
            v["nullifier"][i] = sg["nullifier"][i - 1]
    return v


def _plume_device_inputs(p, v, keys):
    return [p.up(v["msgs"]), p.up(v["off"]), len(v["msgs"])] + [p.up(v[k]) if v.get(k) is not None else None for k in keys]


# ---------------------------------------------------------------------------------------------------- the families
def fam_verify(n, version):
    from tests import _oracle_c as OC
    v = _plume_corrupted(n, version, 9_100_000 + 1000 * version + n)
    rp, hr = (v["r_point"], v["hashed_to_curve_r"]) if version == 1 else (None, None)
    want = {"ok": OC.verify_batch(version, v["msgs"], v["off"], v["pk"], v["nullifier"], v["c"], v["s"], rp, hr, nthreads=8)}
    assert 0 < int(want["ok"].sum()) < n and not want["ok"][bad_positions(n)].any()

    def host(eng, v):
        return {"ok": eng.verify_batch(version, v["msgs"], v["off"], v["pk"], v["nullifier"], v["c"], v["s"], rp, hr)}

    def device(eng, v, p):
        m, off, nb, pk, nul, c, s, r, h = _plume_device_inputs(p, dict(v, r_point=rp, hashed_to_curve_r=hr), ("pk", "nullifier", "c", "s", "r_point", "hashed_to_curve_r"))
        eng.verify_batch_device(version, n, m, off, nb, pk, nul, c, s, r, h, p.out("ok", n), stream=p.ready())
    return Entry(f"verify_v{version}", n, v, want, host, device, status=("ok",), redo=VERIFY)


def fam_verify_non_zk(n):
    from tests import _oracle_c as OC
    v = _plume_corrupted(n, 1, 9_200_000 + n)
    want = {"ok": OC.verify_non_zk_batch(1, v["msgs"], v["off"], v["pk"], v["nullifier"], v["s"], v["r_point"], v["hashed_to_curve_r"], v["c"], nthreads=8)}
    assert (want["ok"] == 1).any() and (want["ok"][bad_positions(n)] != 1).all()

    def host(eng, v):
        return {"ok": eng.verify_non_zk_batch(1, v["msgs"], v["off"], v["pk"], v["nullifier"], v["s"], v["r_point"], v["hashed_to_curve_r"], v["c"])}

    def device(eng, v, p):
        m, off, nb, pk, nul, s, r, h, c = _plume_device_inputs(p, v, ("pk", "nullifier", "s", "r_point", "hashed_to_curve_r", "c"))
        eng.verify_non_zk_batch_device(1, n, m, off, nb, pk, nul, s, r, h, c, p.out("ok", n), stream=p.ready())
    return Entry("verify_non_zk", n, v, want, host, device, status=("ok",), redo=VERIFY)


def fam_verify_sec1(n):
    """the SEC1 ingest (V1): 33-byte records, decompressed on the GPU into scratch of its own with one reject flag per item.  Planted over pk, nullifier, r_point and
    hashed_to_curve_r in turn: a prefix that is none, an x with no point on the curve, the other root of a valid x; and a flipped s.  The per-item oracle of
    tests/_sec1.py (47 ms an item) gives the planted items' verdicts; an item that is not planted holds the lossless compression of four valid points, so its verdict is
    the C oracle's on the 64-byte records"""
    from tests import _oracle_c as OC
    from tests import _sec1 as S1
    b, sg = _plume_signed(n, 1, 9_700_000 + n)
    rec = {k: S1.compress(sg[k]) for k in ("pk", "nullifier", "r_point", "hashed_to_curve_r")}
    s = sg["s"].copy()
    keys = list(rec)
    for j, i in enumerate(bad_positions(n)):
        r, kind = rec[keys[(j // 4) % 4]], j % 4
        if kind == 0:
            r[i, 0] = 5
        elif kind == 1:
            r[i, 1:] = 0
            r[i, 32] = 5
        elif kind == 2:
            r[i, 0] ^= 1
        else:
            s[i, 31] ^= 1
    ok = OC.verify_batch(1, b["msgs"], b["off"], sg["pk"], sg["nullifier"], sg["c"], sg["s"], sg["r_point"], sg["hashed_to_curve_r"], nthreads=8)
    assert ok.all()
    for i in bad_positions(n):
        m = b["msgs"][int(b["off"][i]):int(b["off"][i + 1])].tobytes()
        ok[i] = 1 if S1.oracle_verify_sec1(1, m, rec["pk"][i], rec["nullifier"][i], sg["c"][i], s[i], rec["r_point"][i], rec["hashed_to_curve_r"][i]) else 0
    assert not ok[bad_positions(n)].any()
    v = dict(msgs=b["msgs"], off=b["off"], c=sg["c"], s=s, **rec)

    def host(eng, v):
        return {"ok": eng.verify_batch_sec1(1, v["msgs"], v["off"], v["pk"], v["nullifier"], v["c"], v["s"], v["r_point"], v["hashed_to_curve_r"])}

    def device(eng, v, p):
        args = _plume_device_inputs(p, v, ("pk", "nullifier", "c", "s", "r_point", "hashed_to_curve_r"))
        eng.verify_batch_sec1_device(1, n, *args, p.out("ok", n), stream=p.ready())
    return Entry("verify_sec1", n, v, {"ok": ok}, host, device, status=("ok",), redo=VERIFY)


def fam_sign_sec1(n):
    """sign with 33-byte output records: the C oracle's records, compressed (the identity, an all-zero record, stays all zero)"""
    from tests import _oracle_c as OC
    from tests import _sec1 as S1
    b = _sign_inputs(n, 9_800_000 + n)
    o = OC.sign_batch(2, b["msgs"], b["off"], b["sk"], b["r"], nthreads=8)
    want = {k: (S1.compress(o[k]) if o[k].ndim == 2 and o[k].shape[1] == 64 else o[k]) for k in SIGN_KEYS}
    assert want["status"][bad_positions(n)].all() and int((want["status"] != 0).sum()) == len(bad_positions(n))

    def host(eng, b):
        o = eng.sign_batch_sec1(2, b["msgs"], b["off"], b["sk"], b["r"])
        return {k: o[k] for k in SIGN_KEYS}
    return Entry("sign_sec1", n, b, want, host, None, redo=lambda selfcheck: ARMED if selfcheck else None)      # (the binding has no device form of it)


def fam_recover(n):
    from tests import _recover as R
    v = _plume_corrupted(n, 2, 9_300_000 + n)
    want = R.recover_batch(2, v["msgs"], v["off"], v["pk"], v["nullifier"], v["c"], v["s"], nthreads=8)
    assert {int(x) for x in want["status"]} == {R.MISMATCH, R.MATCH, R.INVALID}
    keys = ("r_point", "hashed_to_curve_r", "hashed_to_curve")

    def host(eng, v):
        return eng.recover_batch(2, v["msgs"], v["off"], v["pk"], v["nullifier"], v["c"], v["s"])

    def device(eng, v, p):
        m, off, nb, pk, nul, c, s = _plume_device_inputs(p, v, ("pk", "nullifier", "c", "s"))
        o = [p.out(k, (n, 64)) for k in keys] + [p.out("status", n)]
        eng.recover_batch_device(2, n, m, off, nb, pk, nul, c, s, *o, stream=p.ready())
    return Entry("recover", n, v, want, host, device, redo=VERIFY)


def fam_aggregate(n):
    from tests import _oracle_c as OC
    v = _plume_corrupted(n, 1, 9_400_000 + n)
    keys = ("pk", "nullifier", "c", "s", "r_point", "hashed_to_curve_r")
    rec, hash_ok = OC.aggregate_check(1, 0, v["msgs"], v["off"], *(v[k] for k in keys), AGG_SEED, nthreads=8)
    want = {"record": rec, "hash_ok": hash_ok}
    assert 0 < int(hash_ok.sum()) < n

    def record(r):                                         # the 72 bytes from the parsed form the host binding returns
        out = np.zeros(72, np.uint8)
        out[0], out[1] = int(r["all_ok"]), int(r["identity"])
        out[4:8] = np.frombuffer(int(r["n_bad"]).to_bytes(4, "little"), np.uint8)
        out[8:72] = np.frombuffer(r["point"], np.uint8)
        return out

    def host(eng, v):
        r = eng.aggregate_check(1, v["msgs"], v["off"], *(v[k] for k in keys), seed=AGG_SEED, mode=0)
        return {"record": record(r), "hash_ok": r["hash_ok"]}

    def device(eng, v, p):
        args = _plume_device_inputs(p, v, keys)
        hok, res = p.out("hash_ok", n), p.out("record", 72)
        eng.aggregate_check_device(1, 0, n, *args, AGG_SEED, 0, hok, res, stream=p.ready())
    assert np.array_equal(record(OC.parse_aggregate_record(rec)), rec)
    return Entry("aggregate", n, v, want, host, device, status=("hash_ok",))


def _sign_inputs(n, start):
    from tests import synth
    b = synth.sign_inputs(n, start=start)
    for j, i in enumerate(bad_positions(n)):               # sk = 0, sk = n, r = 0, r = n: no scalars of the reference's type
        b["sk" if j % 4 < 2 else "r"][i] = _b32(0 if j % 2 == 0 else N)
    return b


def fam_sign(n):
    from tests import _oracle_c as OC
    b = _sign_inputs(n, 9_500_000 + n)
    o = OC.sign_batch(1, b["msgs"], b["off"], b["sk"], b["r"], nthreads=8)
    want = {k: o[k] for k in SIGN_KEYS}
    assert want["status"][bad_positions(n)].all() and int((want["status"] != 0).sum()) == len(bad_positions(n))

    def host(eng, b):
        o = eng.sign_batch(1, b["msgs"], b["off"], b["sk"], b["r"])
        return {k: o[k] for k in SIGN_KEYS}

    def device(eng, b, p):
        m, off, nb, sk, r = _plume_device_inputs(p, b, ("sk", "r"))
        o = [p.out(k, (n, 32 if k in ("c", "s") else 64)) for k in SIGN_KEYS[:-1]] + [p.out("status", n)]
        eng.sign_batch_device(1, n, m, off, nb, sk, r, None, *o, stream=p.ready())
    return Entry("sign", n, b, want, host, device, redo=lambda selfcheck: ARMED if selfcheck else None)


def fam_sign_rfc6979(n):
    from tests import _oracle_c as OC
    from tests import _rfc6979 as R
    b = _sign_inputs(n, 9_600_000 + n)
    b["aux"] = np.random.default_rng(6979 + n).integers(0, 256, (n, 32), dtype=np.uint8)
    valid = np.ones(n, bool)
    for j, i in enumerate(bad_positions(n)):
        b["sk"][i] = _b32(0 if j % 2 == 0 else N)
        valid[i] = False
    # x = sk "as given": an item whose sk is no scalar still has a nonce, and its r_point, hashed_to_curve_r, c and s are computed from it (status 2 says not to use them)
    r = np.frombuffer(R.plume_nonces(2, b["msgs"], b["off"], b["sk"], None, b["aux"]), np.uint8).reshape(-1, 32)
    o = OC.sign_batch(2, b["msgs"], b["off"], b["sk"], r, nthreads=8)
    want = {k: o[k] for k in SIGN_KEYS}
    assert np.array_equal(want["status"] != 0, ~valid)

    def host(eng, b):
        o = eng.sign_batch_rfc6979(2, b["msgs"], b["off"], b["sk"], aux=b["aux"])
        return {k: o[k] for k in SIGN_KEYS}

    def device(eng, b, p):
        m, off, nb, sk, aux = _plume_device_inputs(p, b, ("sk", "aux"))
        o = [p.out(k, (n, 32 if k in ("c", "s") else 64)) for k in SIGN_KEYS[:-1]] + [p.out("status", n)]
        eng.sign_batch_rfc6979_device(2, n, m, off, nb, sk, aux, None, *o, stream=p.ready())
    return Entry("sign_rfc6979", n, b, want, host, device, redo=lambda selfcheck: ARMED if selfcheck else None)


def fam_eth_address(n):
    from tests import _keccak as K
    pk = K.sample_keys(n, 700 + n)
    bad = K.invalid_keys("affine64")
    for j, i in enumerate(bad_positions(n)):
        pk[i] = np.frombuffer(bad[j % len(bad)][1], np.uint8)
    addr, st = K.eth_address_batch(pk, None, "affine64", "eip55")
    assert (st[bad_positions(n)] == K.INVALID).all() and int((st == K.INVALID).sum()) == len(bad_positions(n))

    def host(eng, pk):
        a, s = eng.eth_address_batch(pk, None, "affine64", "eip55")
        return {"address": a, "status": s}

    def device(eng, pk, p):
        d = p.up(pk)
        eng.eth_address_batch_device(n, d, None, p.out("address", (n, 42)), p.out("status", n), "affine64", "eip55", stream=p.ready())
    return Entry("eth_address", n, pk, {"address": addr, "status": st}, host, device)


def fam_ecdsa_recover(n):
    from tests import _ecdsa as E
    h, r, s, v, _ = E.genuine(n, 800 + n, with_pk=False)
    for j, i in enumerate(bad_positions(n)):               # r = 0, s = n, a v that is none, r = p - 1 ... no signatures
        kind = j % 4
        if kind == 0:
            r[i] = 0
        elif kind == 1:
            s[i] = _b32(N)
        elif kind == 2:
            v[i] = 5
        else:
            r[i] = _b32(N - 1)
            v[i] = 0
    pk, addr, st = E.recover_batch(h, r, s, v, None, "sec1", "record64")
    assert (st[bad_positions(n)] == E.INVALID).all() and (st == E.MATCH).sum() == n - len(bad_positions(n))
    inp = dict(hash=h, r=r, s=s, v=v)

    def host(eng, a):
        k, ad, t = eng.ecdsa_recover_batch(a["hash"], a["r"], a["s"], a["v"], None, "sec1", "record64")
        return {"pk": k, "address": ad, "status": t}

    def device(eng, a, p):
        d = [p.up(a[k]) for k in ("hash", "r", "s", "v")]
        eng.ecdsa_recover_batch_device(n, *d, None, p.out("pk", (n, 33)), p.out("address", (n, 64)), p.out("status", n), "sec1", "record64", stream=p.ready())
    return Entry("ecdsa_recover", n, inp, {"pk": pk, "address": addr, "status": st}, host, device, redo=ECDSA)


def _sk_rows(n, seed):
    from tests import _ecdsa_sign as S
    return S.seeded(n, seed)


def fam_ecdsa_sign(n):
    """the message hash of n ragged messages, then the deterministic signature of each digest: two calls, the second fed by the first"""
    from tests import _ecdsa_sign as S
    sk, _, aux = _sk_rows(n, 900 + n)
    for j, i in enumerate(bad_positions(n)):
        sk[i] = _b32(0 if j % 2 == 0 else N + j)
    rng = np.random.default_rng(901 + n)
    lens = rng.integers(0, 300, n)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    msgs = rng.integers(0, 256, int(off[-1]) + 16, dtype=np.uint8)
    h = S.message_hash_batch(msgs[:int(off[-1])], off, S.EIP191)
    r, s, v, st = S.sign_batch(h, sk, aux, S.V27)
    assert (st[bad_positions(n)] == 2).all() and int((st != 0).sum()) == len(bad_positions(n))
    inp = dict(msgs=msgs, off=off, sk=sk, aux=aux)

    def host(eng, a):
        hh = eng.eth_message_hash_batch(a["msgs"], a["off"], "eip191")
        rr, ss, vv, tt = eng.ecdsa_sign_batch(hh, a["sk"], a["aux"], v27=True)
        return {"hash": hh, "r": rr, "s": ss, "v": vv, "status": tt}

    def device(eng, a, p):
        for k, shape in (("hash", (n, 32)), ("r", (n, 32)), ("s", (n, 32)), ("v", n), ("status", n)):
            p.out(k, shape)                                # (every output before ready(): torch fills them on its own stream)
        m, o, k, x = p.up(a["msgs"]), p.up(a["off"]), p.up(a["sk"]), p.up(a["aux"])
        st_ = p.ready()
        eng.eth_message_hash_batch_device(n, m, o, len(a["msgs"]), p.tensor("hash"), "eip191", stream=st_)
        eng.ecdsa_sign_batch_device(n, p.tensor("hash"), k, x, p.tensor("r"), p.tensor("s"), p.tensor("v"), p.tensor("status"), v27=True, stream=st_)
    return Entry("ecdsa_sign", n, inp, {"hash": h, "r": r, "s": s, "v": v, "status": st}, host, device, redo=lambda selfcheck: ECDSA if selfcheck else None)


def _transactions(n, seed):
    """n signed transactions of every kind and their keys"""
    from tests import _eth_tx as T
    sk, _, _ = _sk_rows(n, seed)
    return [T.build(i % 5, sk[i].tobytes(), chain_id=0 if i % 10 == 0 else 1 + i % 3, data=bytes(range(i % 40)), salt=i)[0] for i in range(n)], sk


def fam_eth_tx_sender(n):
    from tests import _ecdsa as E
    from tests import _eth_tx as T
    raws, sk = _transactions(n, 1000 + n)
    for j, i in enumerate(bad_positions(n)):               # ill-framed: a byte short, a byte long; and the other s of a signature (EIP-2)
        i, kind = int(i), j % 3
        raws[i] = raws[i][:-1] if kind == 0 else raws[i] + b"\x00" if kind == 1 else T.build(i % 5, sk[i].tobytes(), chain_id=1, salt=i, high_s=True)[0]
    txs, off = T.pack(raws)
    txs = np.concatenate([txs, np.zeros(16, np.uint8)])
    ps = T.parse_batch(txs[:int(off[-1])], off)
    pk, addr, st = E.recover_batch(ps["hash"], ps["r"], ps["s"], ps["v"], None, "affine64", "raw20", E.LOW_S)
    assert (st[bad_positions(n)] == E.INVALID).all() and int((st == E.MATCH).sum()) == n - len(bad_positions(n))
    want = {"pk": pk, "address": addr, "status": st, "chain_id": ps["chain_id"], "tx_type": ps["tx_type"]}
    inp = dict(txs=txs, off=off)

    def host(eng, a):
        k, ad, t, ch, ty = eng.eth_tx_sender_batch(a["txs"], a["off"])
        return {"pk": k, "address": ad, "status": t, "chain_id": ch, "tx_type": ty}

    def device(eng, a, p):
        eng.eth_tx_sender_batch_device(n, p.up(a["txs"]), p.up(a["off"]), int(a["off"][-1]), None, p.out("pk", (n, 64)), p.out("address", (n, 20)),
                                       p.out("chain_id", n, np.uint64), p.out("tx_type", n), p.out("status", n), stream=p.ready())
    return Entry("eth_tx_sender", n, inp, want, host, device, redo=ECDSA)


def fam_eth_tx_sign(n):
    from tests import _eth_tx as T
    from tests import _eth_tx_sign as X
    sk, _, aux = _sk_rows(n, 1100 + n)
    items = []
    for i in range(n):
        chain = 0 if i % 10 == 0 else 1 + i % 3
        items.append(T.signing_data(i % 5, T.default_fields(i % 5, chain, bytes(range(i % 40)), i), chain))
    for j, i in enumerate(bad_positions(n)):               # ill-framed items, and keys that are none
        kind = j % 3
        if kind == 0:
            items[i] = items[i][:-1]
        elif kind == 1:
            items[i] = items[i] + b"\x00"
        else:
            sk[i] = _b32(0)
    txs, off = T.pack(items)
    txs = np.concatenate([txs, np.zeros(16, np.uint8)])
    want = X.sign_batch(txs[:int(off[-1])], off, sk, aux)
    st = want["status"]
    assert st[bad_positions(n)].all() and int((st != 0).sum()) == len(bad_positions(n)) and {int(x) for x in st} == {0, 2, X.BAD_TX}
    inp = dict(txs=txs, off=off, sk=sk, aux=aux)
    keys = ("out", "out_len", "hash", "r", "s", "v", "chain_id", "tx_type", "status")

    def host(eng, a):
        res = eng.eth_tx_sign_slots(a["txs"], a["off"], a["sk"], a["aux"])
        return {k: res[k] for k in keys}

    def device(eng, a, p):
        nb = len(want["out"])
        o = {k: p.out(k, want[k].shape, want[k].dtype) for k in keys}
        eng.eth_tx_sign_batch_device(n, p.up(a["txs"]), p.up(a["off"]), int(a["off"][-1]), p.up(a["sk"]), p.up(a["aux"]), o["out"], nb, o["out_len"], o["status"],
                                     o["hash"], o["r"], o["s"], o["v"], o["chain_id"], o["tx_type"], stream=p.ready())
    return Entry("eth_tx_sign", n, inp, want, host, device, redo=lambda selfcheck: ECDSA if selfcheck else None)


def fam_hd(n):
    """master nodes of n seeds; private derivation over two levels (keys that are none planted); public derivation over two levels (records that are no key and hardened
    indices planted): three calls"""
    from tests import _hd as H
    rng = np.random.default_rng(1200 + n)
    seed = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    psk, pchain = H.seeded_nodes(n, 1201 + n)
    path = H.seeded_paths(n, 2, 1202 + n)
    ppath = (H.seeded_paths(n, 2, 1203 + n) & np.uint32(0x7FFFFFFF)).astype(np.uint32)
    ppk = H.pk_of(psk)
    psk = psk.copy()
    for j, i in enumerate(bad_positions(n)):
        psk[i] = _b32(0 if j % 2 == 0 else N)
        if j % 2 == 0:
            ppk[i, 63] ^= 1                                # off the curve
        else:
            ppath[i, 1] |= np.uint32(0x80000000)           # a hardened index has no public derivation
    msk, mchain, mst = H.master_batch(seed, 64)
    sk, chain, pk, addr, st = H.derive_priv_batch(psk, pchain, path, 2)
    qpk, qchain, qaddr, qst = H.derive_pub_batch(ppk, pchain, ppath, 2)
    assert (st[bad_positions(n)] == 2).all() and qst[bad_positions(n)].all() and int((st != 0).sum()) == len(bad_positions(n)) == int((qst != 0).sum())
    want = {"master_sk": msk, "master_chain": mchain, "master_status": mst, "sk": sk, "chain": chain, "pk": pk, "address": addr, "status": st,
            "pub_pk": qpk, "pub_chain": qchain, "pub_address": qaddr, "pub_status": qst}
    inp = dict(seed=seed, psk=psk, pchain=pchain, path=path, ppk=ppk, ppath=ppath)

    def host(eng, a):
        m = eng.hd_master_batch(a["seed"])
        d = eng.hd_derive_priv_batch(a["psk"], a["pchain"], a["path"])
        q = eng.hd_derive_pub_batch(a["ppk"], a["pchain"], a["ppath"])
        return {"master_sk": m[0], "master_chain": m[1], "master_status": m[2], "sk": d["sk"], "chain": d["chain"], "pk": d["pk"], "address": d["address"],
                "status": d["status"], "pub_pk": q["pk"], "pub_chain": q["chain"], "pub_address": q["address"], "pub_status": q["status"]}

    def device(eng, a, p):
        o = {k: p.out(k, w.shape) for k, w in want.items()}
        d = {k: p.up(x) for k, x in a.items()}
        st_ = p.ready()
        eng.hd_master_batch_device(n, d["seed"], 64, o["master_sk"], o["master_chain"], o["master_status"], stream=st_)
        eng.hd_derive_batch_device(False, 0, n, d["psk"], d["pchain"], d["path"], 2, o["sk"], o["chain"], o["pk"], o["address"], o["status"], stream=st_)
        eng.hd_derive_batch_device(True, 0, n, d["ppk"], d["pchain"], d["ppath"], 2, None, o["pub_chain"], o["pub_pk"], o["pub_address"], o["pub_status"], stream=st_)
    return Entry("hd", n, inp, want, host, device, status=("master_status", "status", "pub_status"))


def fam_kdf(n):
    """PBKDF2-HMAC-SHA512 with 3 iterations over the planted password lengths.  The host form refuses unsound offsets as a whole, so only the device form is given them:
    a planted item's end lies in front of its start"""
    from tests import _kdf as KD
    buf, off, salt, out, status = KD.planted_case(n, 3, 0, 12)
    assert not status.any()
    doff = off.copy()
    for i in bad_positions(n):
        doff[i + 1] = doff[i] - 1
    dout, dstatus = KD.pbkdf2_batch(buf, doff, len(buf), salt, 12, 3, 64, 0)
    assert (dstatus[bad_positions(n)] == KD.BAD_INPUT).all() and int((dstatus != 0).sum()) == len(bad_positions(n))
    inp = dict(buf=buf, off=off, doff=doff, salt=salt)

    def host(eng, a):
        o, s = eng.pbkdf2_sha512_batch((a["buf"], a["off"]), a["salt"], iterations=3, dklen=64)
        return {"out": o, "status": s}

    def device(eng, a, p):
        eng.pbkdf2_sha512_batch_device(n, p.up(a["buf"]), p.up(a["doff"]), len(a["buf"]), p.up(a["salt"]), 12, 3, 64, p.out("out", (n, 64)), p.out("status", n), flags=0,
                                       stream=p.ready())
    return Entry("kdf", n, inp, {"out": out, "status": status}, host, device, expected_device={"out": dout, "status": dstatus})


def fam_merkle(n):
    """the leaves of n address records (records that are none planted), the tree over them, the proofs of every leaf (indices outside the tree planted) and their check
    against the root: four calls"""
    from tests import _merkle as M
    rng = np.random.default_rng(1400 + n)
    items = np.zeros((n, 64), np.uint8)
    items[:, 44:] = rng.integers(0, 256, (n, 20), dtype=np.uint8)
    for j, i in enumerate(bad_positions(n)):
        items[i, j % 44] = 1 + j
    leaf, lst = M.leaf_batch(M.LEAF_ADDRESS, M.ADDR_RECORD64, items)
    tree, leaf_pos = M.build(leaf, True)
    depth = M.max_proof_len(n)
    pos = np.array(leaf_pos, np.uint32)
    pos[bad_positions(n)[::2]] = 2 * n - 1 + 5
    proof, plen = M.proof_batch(tree, pos, depth)
    vproof = proof.copy()
    vproof[bad_positions(n)[1] + 1, 0, 7] ^= 4             # and one proof that leads elsewhere
    vst = M.verify_batch(M.LEAF_ADDRESS, M.ADDR_RECORD64, items, None, depth, vproof, plen, tree[0])
    assert {int(x) for x in vst} == {M.MISMATCH, M.MATCH, M.INVALID} and (lst[bad_positions(n)] == M.INVALID).all()
    tree_a = np.frombuffer(b"".join(tree), np.uint8).reshape(-1, 32).copy()
    want = {"leaf": leaf, "leaf_status": lst, "tree": tree_a, "leaf_pos": np.array(leaf_pos, np.uint32), "proof": proof, "proof_len": plen, "verify_status": vst}
    inp = dict(items=items, pos=pos, vproof=vproof, depth=depth, root=tree_a[0].copy())

    def host(eng, a):
        lf, ls = eng.merkle_leaf_batch(a["items"], None, "address", "record64")
        tr, lp = eng.merkle_tree_build(lf, True)
        pr, pl = eng.merkle_proof_batch(tr, a["pos"], a["depth"])
        vs = eng.merkle_verify_batch(a["items"], a["vproof"], pl, tr[0], None, "address", "record64")
        return {"leaf": lf, "leaf_status": ls, "tree": tr, "leaf_pos": lp, "proof": pr, "proof_len": pl, "verify_status": vs}

    def device(eng, a, p):
        o = {k: p.out(k, w.shape, w.dtype) for k, w in want.items()}
        it, ps, vp, rt = p.up(a["items"]), p.up(a["pos"]), p.up(a["vproof"]), p.up(a["root"])
        st_ = p.ready()
        eng.merkle_leaf_batch_device(n, it, None, o["leaf"], o["leaf_status"], "address", "record64", stream=st_)
        eng.merkle_tree_build_device(n, o["leaf"], o["tree"], o["leaf_pos"], True, stream=st_)
        eng.merkle_proof_batch_device(n, o["tree"], n, ps, a["depth"], o["proof"], o["proof_len"], stream=st_)
        eng.merkle_verify_batch_device(n, it, None, a["depth"], vp, o["proof_len"], rt, o["verify_status"], "address", "record64", stream=st_)
    return Entry("merkle", n, inp, want, host, device, status=("leaf_status", "proof_len", "verify_status"))


def fam_dedup(n):
    """first occurrences among n records drawn from n / 3 (items that are not live planted), by the definition tests/test_gpu_nullset.py states"""
    from tests.test_gpu_nullset import _expected
    rng = np.random.default_rng(1500 + n)
    pool = rng.integers(0, 256, (max(n // 3, 2), 64), dtype=np.uint8)
    recs = pool[rng.integers(0, len(pool), n)]
    live = np.ones(n, np.uint8)
    live[bad_positions(n)] = 0
    ids = ((1 << 62) - 3 * np.arange(n, dtype=np.uint64)).astype(np.uint64)
    first = _expected(set(), recs, live, ids)
    assert 0 < int(first.sum()) < n and not first[bad_positions(n)].any()
    want = {"first": first, "count": np.array([int(first.sum())], np.uint64)}
    inp = dict(recs=recs, live=live, ids=ids)

    def host(eng, a):
        f, c = eng.nullifier_first_occurrence(a["recs"], a["live"], a["ids"])
        return {"first": f, "count": np.array([c], np.uint64)}

    def device(eng, a, p):
        eng.nullifier_first_occurrence_device(n, p.up(a["recs"]), p.up(a["live"]), p.up(a["ids"]), p.out("first", n), p.out("count", 1, np.uint64), stream=p.ready())
    return Entry("dedup", n, inp, want, host, device, status=("first",))


FAMILIES = {
    "verify_v1": lambda n: fam_verify(n, 1), "verify_v2": lambda n: fam_verify(n, 2), "verify_non_zk": fam_verify_non_zk, "verify_sec1": fam_verify_sec1,
    "sign_sec1": fam_sign_sec1, "recover": fam_recover, "aggregate": fam_aggregate,
    "sign": fam_sign, "sign_rfc6979": fam_sign_rfc6979, "eth_address": fam_eth_address, "ecdsa_recover": fam_ecdsa_recover, "ecdsa_sign": fam_ecdsa_sign,
    "eth_tx_sender": fam_eth_tx_sender, "eth_tx_sign": fam_eth_tx_sign, "hd": fam_hd, "kdf": fam_kdf, "merkle": fam_merkle, "dedup": fam_dedup,
}
_TABLE = {}


def table(families=None):
    """family -> {LARGE: entry, SMALL: entry}, computed once per process (leave the arrays unchanged)"""
    for name in families or FAMILIES:
        if name not in _TABLE:
            _TABLE[name] = {n: FAMILIES[name](n) for n in (LARGE, SMALL)}
    return {name: _TABLE[name] for name in (families or FAMILIES)}
