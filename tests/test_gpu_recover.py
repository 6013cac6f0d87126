"""plume_recover_batch on the MI355X (include/plume_hip.h; last kernel in csrc/plume_recover_kernels.hip): r_point = s G - c pk, hashed_to_curve_r = s H - c nullifier
and H, recomputed by the V2 verify pipeline and WRITTEN instead of only hashed.  Expected values come from the reference's vector, the golden fixtures, the restatement
of the definition in tests/_recover.py (oracles only) and, in the closed loop, from the library's own signer and verifier -- whose results the other suites pin."""
import json
from pathlib import Path

import numpy as np
import pytest

from tests import _fuzz
from tests import _oracle_c as OC
from tests import _recover as R
from tests import synth

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLD = json.loads((ROOT / "tests" / "golden" / "golden_batches.json").read_text())
OUTS = ("r_point", "hashed_to_curve_r", "hashed_to_curve")
ALL = OUTS + ("status",)


@pytest.fixture(scope="module")
def eng():
    import zk_nullifier_sig_amd as plume
    e = plume.Engine(0)
    yield e
    e.close()


def _arrays(items):
    mb, off = OC.pack_msgs([bytes.fromhex(it["msg"]) for it in items])
    return dict(msgs=mb, off=off, pk=OC.arr(items, "pk", 64), nullifier=OC.arr(items, "nullifier", 64), c=OC.arr(items, "c", 32), s=OC.arr(items, "s", 32))


def _host(eng, ver, v, fmt=0, want=ALL):
    return eng.recover_batch(ver, v["msgs"], v["off"], v["pk"], v["nullifier"], v["c"], v["s"], fmt=fmt, want=want)


def _device(eng, ver, v, fmt=0, want=ALL, stream=None, fill=0xAA, off=None, msgs_bytes=None, sync=True, e=None):
    """one device-form call into tensors pre-filled with `fill`; returns every array (the ones not wanted still hold the fill)"""
    import torch
    dev = torch.device(f"cuda:{eng.device_id}")
    n = len(v["off"]) - 1
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    W = 33 if fmt == 1 else 64
    o = {k: torch.full((n, W), fill, dtype=torch.uint8, device=dev) for k in OUTS}
    o["status"] = torch.full((n,), fill, dtype=torch.uint8, device=dev)
    s = stream or torch.cuda.Stream(dev)                                 # (never torch's default stream: its handle is NULL, which the library reads as "the context's own stream")
    d = dict(msgs=t(v["msgs"]), off=t((v["off"] if off is None else off).view(np.int64)), pk=t(v["pk"]), nullifier=t(v["nullifier"]), c=t(v["c"]), s=t(v["s"]))
    s.wait_stream(torch.cuda.current_stream(dev))
    g = lambda k: o[k] if k in want else None  # noqa: E731
    (e or eng).recover_batch_device(ver, n, d["msgs"], d["off"], int(v["off"][-1]) if msgs_bytes is None else msgs_bytes, d["pk"], d["nullifier"], d["c"], d["s"],
                                    g("r_point"), g("hashed_to_curve_r"), g("hashed_to_curve"), g("status"), fmt=fmt, stream=s)
    if not sync:
        return o, d
    s.synchronize()
    return {k: x.cpu().numpy() for k, x in o.items()}


def _device_verify(eng, ver, v, rp=None, hr=None):
    import torch
    dev = torch.device(f"cuda:{eng.device_id}")
    n = len(v["off"]) - 1
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    ok = torch.full((n,), 0xAA, dtype=torch.uint8, device=dev)
    eng.verify_batch_device(ver, n, t(v["msgs"]), t(v["off"].view(np.int64)), int(v["off"][-1]), t(v["pk"]), t(v["nullifier"]), t(v["c"]), t(v["s"]), t(rp), t(hr), ok)
    torch.cuda.synchronize(dev)
    return ok.cpu().numpy()


def _same(a, b, what, keys=ALL):
    for k in keys:
        assert np.array_equal(np.asarray(a[k]).reshape(-1).view(np.uint8), np.asarray(b[k]).reshape(-1).view(np.uint8)), f"{what}: {k} differs"


# ------------------------------------------------------------------------------------------------------- the reference's vector
@pytest.mark.parametrize("ver", [1, 2])
def test_reference_vector(eng, kats, ver):
    k = kats["plume_vector"]
    pt = lambda name: np.frombuffer(bytes.fromhex(k[name + "_x"]) + bytes.fromhex(k[name + "_y"]), np.uint8).reshape(1, 64).copy()  # noqa: E731
    sc = lambda name: np.frombuffer(bytes.fromhex(k[name]), np.uint8).reshape(1, 32).copy()  # noqa: E731
    mb, off = OC.pack_msgs([k["msg_utf8"].encode()])
    v = dict(msgs=mb, off=off, pk=pt("pk"), nullifier=pt("nullifier"), c=sc(f"c_v{ver}"), s=sc(f"s_v{ver}"))
    for got in (_host(eng, ver, v), _device(eng, ver, v)):
        assert np.array_equal(got["r_point"], pt("g_r")) and np.array_equal(got["hashed_to_curve_r"], pt("h_r")) and np.array_equal(got["hashed_to_curve"], pt("h"))
        assert list(got["status"]) == [R.MATCH]
    assert list(_host(eng, 3 - ver, v)["status"]) == [R.MISMATCH]      # the other version's hash of the same points


# ------------------------------------------------------------------------------------------------------- golden fixtures
@pytest.mark.parametrize("ver", [1, 2])
def test_golden_sign_records(eng, ver):
    items = GOLD[f"sign_v{ver}"]
    assert len(items) == 64
    got = _host(eng, ver, _arrays(items))
    assert np.array_equal(got["r_point"], OC.arr(items, "r_point", 64))
    assert np.array_equal(got["hashed_to_curve_r"], OC.arr(items, "hashed_to_curve_r", 64))
    assert np.array_equal(got["hashed_to_curve"], OC.arr(items, "h", 64))
    assert (got["status"] == R.MATCH).all()


@pytest.fixture(scope="module")
def golden_v2():
    """verify_v2 (256 items) and edge (120 items) with the restatement's results, computed once"""
    out = {}
    for name, items in (("verify_v2", GOLD["verify_v2"]), ("edge", GOLD["edge"])):
        v = _arrays(items)
        out[name] = (items, v, R.recover_batch(2, v["msgs"], v["off"], v["pk"], v["nullifier"], v["c"], v["s"], nthreads=16))
    return out


@pytest.mark.parametrize("name,n,holds", [("verify_v2", 256, (R.MISMATCH, R.MATCH)), ("edge", 120, (R.MISMATCH, R.MATCH, R.INVALID))])
def test_golden_verify_batches(eng, golden_v2, name, n, holds):
    """each batch is asserted to hold at least one item of every status it can hold, so that no comparison below runs on an empty case: `edge` holds all three;
    `verify_v2` is 240 honest items and 16 with a flipped s, c, message or a neighbour's nullifier -- every one a value of the reference's types, so it holds no
    status 3 (the restatement's counts: verify_v2 16 / 240 / 0, edge 75 / 27 / 18 items of status 0 / 1 / 3)"""
    items, v, want = golden_v2[name]
    assert len(items) == n
    got = _host(eng, 2, v)
    for st in (R.MISMATCH, R.MATCH, R.INVALID):
        assert (want["status"] == st).any() == (st in holds), f"{name}: items of status {st}"
    _same(got, want, name)
    v2 = [i for i, it in enumerate(items) if it.get("version", 2) == 2]            # (edge mixes V1 and V2 records: the fixture's ok is a V2 verdict for the V2 ones)
    assert len(v2) >= 30
    assert [int(got["status"][i] == R.MATCH) for i in v2] == [items[i]["ok"] for i in v2]
    assert np.array_equal(got["status"] == R.MATCH, eng.verify_batch(2, v["msgs"], v["off"], v["pk"], v["nullifier"], v["c"], v["s"]) == 1)


def test_redo_tasks_are_those_of_a_v2_verify(eng, golden_v2):
    _, v, _ = golden_v2["edge"]
    eng.verify_batch(2, v["msgs"], v["off"], v["pk"], v["nullifier"], v["c"], v["s"])
    after_verify = eng.last_redo_tasks()
    _host(eng, 2, v)
    assert eng.last_redo_tasks() == after_verify
    assert eng.last_msm_kernel() == "k_verify_msm_pair"
    eng.set_stage_timing(True)
    try:
        _device(eng, 2, v)
        names = [k for k, _ in eng.last_stage_times()]
    finally:
        eng.set_stage_timing(False)
    assert names[-2:] == ["to_affine", "recover_finalize"] and "verify_msm" in names and "verify_finalize" not in names


# ------------------------------------------------------------------------------------------------------- closed loop
def _closed_loop_batch(eng, n, seed):
    """even items signed as V1, odd items as V2, then corrupted by tests/_fuzz.py (with the r = 0 signature planted)"""
    b = synth.sign_inputs(n, seed=seed)
    s1 = eng.sign_batch(1, b["msgs"], b["off"], b["sk"], b["r"])
    s2 = eng.sign_batch(2, b["msgs"], b["off"], b["sk"], b["r"])
    assert np.array_equal(s1["r_point"], s2["r_point"]) and np.array_equal(s1["hashed_to_curve_r"], s2["hashed_to_curve_r"])
    signed = {k: s2[k].copy() for k in ("pk", "nullifier", "c", "s", "r_point", "hashed_to_curve_r")}
    signed["c"][0::2] = s1["c"][0::2]
    signed["s"][0::2] = s1["s"][0::2]
    v = _fuzz.fuzz_verify_batch(2, signed, b, seed)
    clean = np.ones(n, dtype=bool)
    for k in ("pk", "nullifier", "c", "s"):
        clean &= (v[k] == signed[k]).all(axis=1)
    lens = np.diff(b["off"].astype(np.int64))
    assert (lens == lens[0]).all()
    L = int(lens[0])
    clean &= (v["msgs"][:n * L].reshape(n, L) == b["msgs"][:n * L].reshape(n, L)).all(axis=1)
    return v, signed, clean


@pytest.mark.parametrize("n,sub", [(1, 1), (3, 1), (257, 1), (1025, 1), (16385, 1), (65537, 1), (1 << 17, 2)])
def test_closed_loop(eng, n, sub):
    """sizes: one item; less than a quad of items; more than one workgroup; across the 1024-item slice grid; just past the pair kernel (2^14); past the two-role
    ingest (2^16); two overlapped sub-batches (2^17 is the smallest call that is cut)"""
    v, signed, clean = _closed_loop_batch(eng, n, 1000 + n)
    eng.set_sub_batches(sub)
    try:
        got = _device(eng, 2, v)
        got1 = _device(eng, 1, v)
        ok2 = _device_verify(eng, 2, v)
        ok1 = _device_verify(eng, 1, v, got1["r_point"], got1["hashed_to_curve_r"])
    finally:
        eng.set_sub_batches(1)
    assert np.array_equal(got["status"] == R.MATCH, ok2 == 1)
    assert np.array_equal(got1["status"] == R.MATCH, ok1 == 1)
    _same(got, got1, "the points do not depend on the version", OUTS)
    assert np.array_equal(got["status"] == R.INVALID, got1["status"] == R.INVALID)
    for k in OUTS:
        assert not got[k][got["status"] == R.INVALID].any()
    if n >= 257:                                                        # (the smallest batches may hold no honest item of one of the two kinds)
        assert (ok2 == 1).any() and (ok1 == 1).any() and (ok2 == 0).any() and (got["status"] == R.INVALID).any()
    assert clean.any() or n < 3
    assert np.array_equal(got["r_point"][clean], signed["r_point"][clean]) and np.array_equal(got["hashed_to_curve_r"][clean], signed["hashed_to_curve_r"][clean])
    assert (got["status"][clean & (np.arange(n) % 2 == 1)] == R.MATCH).all() and (got1["status"][clean & (np.arange(n) % 2 == 0)] == R.MATCH).all()
    if n <= 1025:                                                       # ... and, where the oracles are quick enough, every item against the definition
        _same(got, R.recover_batch(2, v["msgs"], v["off"], v["pk"], v["nullifier"], v["c"], v["s"], nthreads=16), f"n={n}")


# ------------------------------------------------------------------------------------------------------- forms and formats
@pytest.fixture(scope="module")
def mixed(eng):
    """1001 items (no multiple of 4) of every status, with the 64-byte results of the host form"""
    v, _, _ = _closed_loop_batch(eng, 1001, 77)
    ref = {ver: _host(eng, ver, v) for ver in (1, 2)}
    for st in (R.MISMATCH, R.MATCH, R.INVALID):
        assert (ref[1]["status"] == st).any() and (ref[2]["status"] == st).any()
    return v, ref


@pytest.mark.parametrize("ver", [1, 2])
def test_host_form_equals_device_form_in_every_format(eng, mixed, ver):
    from zk_nullifier_sig_amd import capi
    v, ref = mixed
    _same(_device(eng, ver, v), ref[ver], "device form")
    assert (ref[ver]["r_point"] == 0).all(axis=1).any()                 # identity records are among them (the planted r = 0 items, the rejected ones)
    for fmt, conv in ((R.FMT_SEC1, R.sec1_of), (R.FMT_REGISTERS, R.registers_of)):
        want = {k: conv(ref[ver][k]) for k in OUTS}
        want["status"] = ref[ver]["status"]
        _same(_host(eng, ver, v, fmt=fmt), want, f"host form, format {fmt}")
        _same(_device(eng, ver, v, fmt=fmt), want, f"device form, format {fmt}")
    # ... which are sec1_compress and registers_from_be of the 64-byte records
    assert np.array_equal(R.registers_of(ref[ver]["r_point"]).reshape(-1, 8).view("<u8").reshape(-1, 2, 4), capi.registers_from_be(ref[ver]["r_point"].reshape(-1, 2, 32)))
    assert R.sec1_of(ref[ver]["r_point"][:16]).tobytes() == b"".join(OC.sec1_compress(r.tobytes()).ljust(33, b"\0") for r in ref[ver]["r_point"][:16])
    # page-locked caller arrays: the two-lane host pipeline
    pv = {k: capi.pinned_copy(x) for k, x in v.items() if k in ("msgs", "off", "pk", "nullifier", "c", "s")}
    _same(_host(eng, ver, pv), ref[ver], "page-locked")


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_every_subset_of_null_outputs(eng, mixed, fmt):
    v, ref = mixed
    full = _device(eng, 2, v, fmt=fmt)
    for mask in range(1, 15):
        want = tuple(k for j, k in enumerate(ALL) if mask & (1 << j))
        got = _device(eng, 2, v, fmt=fmt, want=want, fill=0x5A + mask)
        for k in ALL:
            if k in want:
                assert np.array_equal(got[k], full[k]), (fmt, mask, k)
            else:
                assert (got[k] == 0x5A + mask).all(), (fmt, mask, k, "an array that was not given was written")
        if mask in (1, 8, 6):
            _same(_host(eng, 2, v, fmt=fmt, want=want), {k: full[k] for k in want}, f"host form, mask {mask}", want)
    with pytest.raises(Exception, match="no output array"):
        _device(eng, 2, v, want=())


def test_multi_device_context_and_two_lanes_in_flight(eng, mixed):
    import torch

    import zk_nullifier_sig_amd as plume
    v, ref = mixed
    n = 1000
    cut = dict(msgs=v["msgs"], off=v["off"][:n + 1], **{k: v[k][:n] for k in ("pk", "nullifier", "c", "s")})
    want = {k: ref[2][k][:n] for k in ALL}
    multi = plume.Engine([0, 0, 0])
    try:
        assert multi.num_shards() == 3
        _same(_host(multi, 2, cut), want, "three shards")
    finally:
        multi.close()
    e2 = plume.Engine(0)
    try:
        e2.set_in_flight(2)
        dev = torch.device("cuda:0")
        streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
        pending = [_device(eng, 2 - (j & 1), cut, stream=streams[j & 1], sync=False, e=e2) for j in range(4)]
        torch.cuda.synchronize(dev)
        for j, (o, _keep) in enumerate(pending):
            _same({k: x.cpu().numpy() for k, x in o.items()}, {k: ref[2 - (j & 1)][k][:n] for k in ALL}, f"in flight, call {j}")
    finally:
        e2.close()


def test_device_form_rejects_bad_offsets_without_touching_neighbours(eng):
    items = GOLD["sign_v2"][:8]
    v = _arrays(items)
    off = v["off"].copy()
    off[4] = off[3] - 1                                                  # item 3 decreases; item 4 becomes the span [off[3] - 1, off[5]): another message
    msgs_bytes = int(off[-1]) - 2                                        # item 7 reaches past the buffer
    got = _device(eng, 2, v, off=off, msgs_bytes=msgs_bytes)
    msgs = [v["msgs"][int(off[i]):int(off[i + 1])].tobytes() if i not in (3, 7) else b"" for i in range(8)]
    mb, moff = OC.pack_msgs(msgs)
    want = R.recover_batch(2, mb, moff, v["pk"], v["nullifier"], v["c"], v["s"])
    for k in ALL:
        want[k][[3, 7]] = R.INVALID if k == "status" else 0
    _same(got, want, "bad offsets")
    assert list(got["status"]) == [1, 1, 1, 3, 0, 1, 1, 3]
    assert np.array_equal(got["r_point"][4], OC.arr(items, "r_point", 64)[4]) and not np.array_equal(got["hashed_to_curve_r"][4], OC.arr(items, "hashed_to_curve_r", 64)[4])


def test_argument_checks(eng, mixed):
    import ctypes as C
    v, _ = mixed
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.zeros(64, np.uint8)
    for ver, fmt, text in ((3, 0, "version"), (0, 0, "version"), (2, 3, "format"), (2, -1, "format")):
        rc = eng._lib.plume_recover_batch(eng._ctx, ver, fmt, 1, p(v["msgs"]), p(v["off"]), p(v["pk"]), p(v["nullifier"]), p(v["c"]), p(v["s"]), p(out), None, None, None)
        assert rc != 0 and text in eng._lib.plume_last_error().decode(), (ver, fmt)
    assert eng._lib.plume_recover_batch(eng._ctx, 2, 0, 1, p(v["msgs"]), p(v["off"]), p(v["pk"]), None, p(v["c"]), p(v["s"]), p(out), None, None, None) != 0
    assert eng._lib.plume_recover_batch(eng._ctx, 2, 0, 0, None, None, None, None, None, None, None, None, None, None) == 0      # an empty batch is no error, as for verify
    assert not out.any()
    eng.set_chunk(512)
    try:
        with pytest.raises(Exception, match="chunk"):
            _device(eng, 2, v)
        _same(_host(eng, 2, v), mixed[1][2], "host form cut by the chunk limit")
    finally:
        eng.set_chunk(1 << 20)
