"""plume_ecdsa_recover_batch on the MI355X (include/plume_hip.h; kernels in csrc/plume_ecdsa_kernels.hip, lane bodies in csrc/plume_ecdsa.h): the public key and the
Ethereum address behind every ECDSA signature, byte for byte against the pure-Python restatement of tests/_ecdsa.py (pinned to OpenSSL by
tests/test_ecdsa_restatement.py) and the vectors of tests/golden/ecdsa_recover_kats.json.  Every comparison is bit-exact and leaves no item out.  The block is 256 lanes
and a wavefront 64; the batched inversions take 8 points per lane."""
import ctypes as C

import numpy as np
import pytest

from tests import _ecdsa as E
from tests import _keccak as K

pytestmark = pytest.mark.gpu

PKF, ADF = ("affine64", "sec1"), ("raw20", "record64", "eip55")
PAIRS = [(pf, af) for pf in PKF for af in ADF]
FILL = 0xAA
NMIX = 2000                    # 1000 uniformly random items interleaved with 1000 genuine signatures
MID = 960                      # the crafted items sit at [MID, MID + their number): across the wavefront boundary at 1024


def _kat_rows():
    kats = E.load_kats()
    rows = [(bytes.fromhex(e["hash"]), bytes.fromhex(e["r"]), bytes.fromhex(e["s"]), e["v"]) for e in kats["openssl"] + kats["crafted"]]
    return rows, len(kats["openssl"]), [c["name"] for c in kats["crafted"]]


def _arrays(rows):
    n = len(rows)
    a = lambda k: np.frombuffer(b"".join(row[k] for row in rows), np.uint8).reshape(n, 32).copy()  # noqa: E731
    return a(0), a(1), a(2), np.array([row[3] for row in rows], np.uint8)


def test_a_context_that_only_recovers_builds_the_comb_and_never_the_window_table():
    """first in the file, on a context of its own, at n = 257: free device memory drops by the comb (252 MiB) and kilobytes of workspace, never by the verifier's 1 GiB
    window table.  Read the way tests/test_gpu_eth_address.py reads it: torch.cuda.mem_get_info around open / use / close"""
    import torch
    import zk_nullifier_sig_amd as plume
    H, R, S, V, _ = E.genuine(257, 41, with_pk=False)
    torch.cuda.synchronize()
    e = plume.Engine(0)
    try:
        free1, _ = torch.cuda.mem_get_info(0)
        pk, address, status = e.ecdsa_recover_batch(H, R, S, V)
        torch.cuda.synchronize()
        free2, _ = torch.cuda.mem_get_info(0)
        wpk, wad, wst = E.recover_batch(H, R, S, V)
        assert np.array_equal(pk, wpk) and np.array_equal(address, wad) and np.array_equal(status, wst) and (status == E.MATCH).all()
    finally:
        e.close()
    assert free1 - free2 < (512 << 20), (free1, free2)


@pytest.fixture(scope="module")
def eng():
    import zk_nullifier_sig_amd as plume
    e = plume.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def kat():
    rows, nk, names = _kat_rows()
    return dict(arrays=_arrays(rows), nk=nk, names=names)


@pytest.fixture(scope="module")
def mix():
    """NMIX items: uniformly random (hash, r, s, v in {0, 1, 27, 28}) at the even positions -- about half of random r have no square root -- and genuine signatures at the
    odd ones, so both outcomes share wavefronts; the identity construction at lane 0, a doubling construction at lane 63, R = G at lane 64, every crafted item from MID on.
    Computed once; the restatement's answers are cached per item (tests/_ecdsa.py)."""
    rng = np.random.default_rng(2026)
    H, R, S, V, _ = E.genuine(NMIX // 2, 42, with_pk=False)
    h = np.zeros((NMIX, 32), np.uint8); r = h.copy(); s = h.copy(); v = np.zeros(NMIX, np.uint8)
    h[1::2], r[1::2], s[1::2], v[1::2] = H, R, S, V
    h[0::2] = rng.integers(0, 256, (NMIX // 2, 32), dtype=np.uint8); r[0::2] = rng.integers(0, 256, (NMIX // 2, 32), dtype=np.uint8)
    s[0::2] = rng.integers(0, 256, (NMIX // 2, 32), dtype=np.uint8); v[0::2] = rng.choice(np.array([0, 1, 27, 28], np.uint8), NMIX // 2)
    rows, nk, names = _kat_rows()
    ch, cr, cs, cv = _arrays(rows[nk:])
    for pos, name in ((0, "identity: R = k G, hash = s k"), (63, "doubling: R = k G, hash = -s k"), (64, "R = G")):
        k = names.index(name)
        h[pos], r[pos], s[pos], v[pos] = ch[k], cr[k], cs[k], cv[k]
    nc = len(cv)
    h[MID:MID + nc], r[MID:MID + nc], s[MID:MID + nc], v[MID:MID + nc] = ch, cr, cs, cv
    _, raw, st = E.recover_batch(h, r, s, v)
    random_invalid = int((st[0:MID:2] == E.INVALID).sum())
    assert 0.35 * (MID // 2) < random_invalid < 0.65 * (MID // 2)                   # about half of the random items, and every genuine one recovers
    assert (st[1:MID:2] == E.MATCH).all() and st[0] == E.INVALID and st[63] == E.MATCH and st[64] == E.MATCH
    return dict(arrays=(h, r, s, v), raw=raw, status=st)


def _device(eng, arrays, n, expect, pf, af, low_s=False, stream=None, pk=True, address=True, status=True, sync=True):
    """one device-form call on the first n items into tensors pre-filled with FILL"""
    import torch
    dev = torch.device(f"cuda:{eng.device_id}")
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a[:n])).to(dev)  # noqa: E731
    o = dict(pk=torch.full((n, K.PK_WIDTH[pf]), FILL, dtype=torch.uint8, device=dev), address=torch.full((n, K.ADDR_WIDTH[af]), FILL, dtype=torch.uint8, device=dev),
             status=torch.full((n,), FILL, dtype=torch.uint8, device=dev))
    st = stream or torch.cuda.Stream(dev)                                # (never torch's default stream: its handle is NULL, which the library reads as "the context's own stream")
    d = [t(a) for a in arrays] + [t(expect)]
    st.wait_stream(torch.cuda.current_stream(dev))
    eng.ecdsa_recover_batch_device(n, d[0], d[1], d[2], d[3], d[4], o["pk"] if pk else None, o["address"] if address else None, o["status"] if status else None,
                                   pk_format=pf, addr_format=af, low_s=low_s, stream=st)
    if not sync:
        return o, d
    st.synchronize()
    return {k: x.cpu().numpy() for k, x in o.items()}


def _both_forms(eng, arrays, n, pf, af, low_s=False, expect=None):
    """the host form and the device form on the first n items against the restatement: every output byte, every status byte"""
    h, r, s, v = (a[:n] for a in arrays)
    ex = None if expect is None else expect[:n]
    wpk, wad, wst = E.recover_batch(h, r, s, v, ex, pf, af, E.LOW_S if low_s else 0)
    pk, address, status = eng.ecdsa_recover_batch(h, r, s, v, ex, pf, af, low_s)
    assert np.array_equal(status, wst) and np.array_equal(pk, wpk) and np.array_equal(address, wad), (n, pf, af, low_s, "host form")
    got = _device(eng, arrays, n, ex, pf, af, low_s)
    assert np.array_equal(got["status"], wst) and np.array_equal(got["pk"], wpk) and np.array_equal(got["address"], wad), (n, pf, af, low_s, "device form")
    return wst


@pytest.mark.parametrize("pf,af", PAIRS)
def test_kats_and_crafted_items_in_every_format_pair(eng, kat, pf, af):
    n = len(kat["arrays"][3])
    for low_s in (False, True):
        st = _both_forms(eng, kat["arrays"], n, pf, af, low_s)
        named = dict(zip(kat["names"], st[kat["nk"]:]))
        if not low_s:
            assert (st[:kat["nk"]] == E.MATCH).all()
            assert named["identity: R = k G, hash = s k"] == E.INVALID and named["doubling: R = k G, hash = -s k"] == E.MATCH and named["r = n - 1, v = 0"] == E.INVALID
            assert named["comb doubling: u2 R = G, u1 = 1"] == E.MATCH and named["comb identity: u2 R = G, u1 = -1"] == E.INVALID
        assert named["s = (n + 1) / 2, flags = 1"] == (E.INVALID if low_s else E.MATCH) and named["s = (n - 1) / 2, flags = 1"] == E.MATCH


def test_openssl_keys_come_back(eng, kat):
    want = "".join(e["pk"] for e in E.load_kats()["openssl"])
    h, r, s, v = (a[:kat["nk"]] for a in kat["arrays"])
    pk, _, status = eng.ecdsa_recover_batch(h, r, s, v)
    assert pk.tobytes().hex() == want and (status == E.MATCH).all()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes_around_wavefront_workgroup_and_inversion_groups(eng, mix, n):
    pf, af = PAIRS[n % len(PAIRS)]
    _both_forms(eng, mix["arrays"], n, pf, af)


@pytest.mark.parametrize("pf,af", PAIRS)
def test_random_and_genuine_items_sharing_wavefronts(eng, mix, pf, af):
    st = _both_forms(eng, mix["arrays"], NMIX, pf, af)
    assert np.array_equal(st, mix["status"])


def test_low_s_over_the_crafted_stretch(eng, mix):
    arrays = tuple(a[MID - 60:MID + 140] for a in mix["arrays"])
    st = _both_forms(eng, arrays, 200, "sec1", "record64", low_s=True)
    assert (st == E.INVALID).sum() > (mix["status"][MID - 60:MID + 140] == E.INVALID).sum()


def _tiled(mix, n):
    reps = -(-n // NMIX)
    return tuple(np.concatenate([a] * reps)[:n] for a in mix["arrays"]), np.concatenate([mix["raw"]] * reps)[:n], np.concatenate([mix["status"]] * reps)[:n]


def test_4097_items_with_three_sub_batches_and_with_chunks_of_1000(mix):
    import zk_nullifier_sig_amd as plume
    arrays, raw, status = _tiled(mix, 4097)
    e = plume.Engine(0)
    try:
        e.set_sub_batches(3)
        got = _device(e, arrays, 4097, None, "affine64", "raw20")
        assert np.array_equal(got["address"], raw) and np.array_equal(got["status"], status)
        e.set_sub_batches(1)
        e.set_chunk(1000)
        pk, address, st = e.ecdsa_recover_batch(*arrays, addr_format="raw20")
        assert np.array_equal(address, raw) and np.array_equal(st, status) and np.array_equal(pk, got["pk"])
        with pytest.raises(plume.PlumeHipError, match="chunk"):
            _device(e, arrays, 4097, None, "affine64", "raw20")                       # the device form is one call of at most a chunk, as for verify
    finally:
        e.close()


def test_a_call_that_really_is_cut_into_sub_batches(mix, monkeypatch):
    """plume_set_sub_batches cuts a call only from 2 x 8192 items on and, by default, from 2^17: with the threshold lowered, 16385 items run as two slices"""
    import zk_nullifier_sig_amd as plume
    monkeypatch.setenv("PLUME_OVERLAP_MIN", "1024")
    arrays, raw, status = _tiled(mix, 16385)
    e = plume.Engine(0)
    try:
        e.set_sub_batches(2)
        got = _device(e, arrays, 16385, raw, "sec1", "eip55")
        tile = lambda a: np.concatenate([a] * 9)[:16385]  # noqa: E731
        wpk, wad, _ = E.recover_batch(*mix["arrays"], None, "sec1", "eip55")
        assert np.array_equal(got["status"], status) and np.array_equal(got["pk"], tile(wpk)) and np.array_equal(got["address"], tile(wad))
    finally:
        e.close()


def test_expect_right_one_flipped_bit_and_invalid_items(eng, mix):
    rng = np.random.default_rng(4)
    invalid = mix["status"] == E.INVALID
    expect = mix["raw"].copy()
    expect[invalid] = rng.integers(1, 256, (int(invalid.sum()), 20), dtype=np.uint8)         # an invalid item is status 3 whatever expect holds
    wrong = np.array(sorted(set(rng.integers(0, NMIX, 200).tolist()) - set(np.flatnonzero(invalid).tolist())))
    for k, i in enumerate(wrong):
        expect[i, k % 20] ^= np.uint8(1 << (k % 8))                    # one bit, every byte position in turn
    want = mix["status"].copy()
    want[wrong] = E.MISMATCH
    st = _both_forms(eng, mix["arrays"], NMIX, "affine64", "raw20", expect=expect)
    assert np.array_equal(st, want) and len(wrong) > 50
    got = _device(eng, mix["arrays"], NMIX, expect, "sec1", "eip55")
    assert got["pk"][wrong].any(axis=1).all() and got["address"][wrong].any(axis=1).all()     # a mismatch still writes pk and address
    assert not got["pk"][invalid].any() and not got["address"][invalid].any()


def test_each_optional_output_null_in_turn(eng, mix):
    n = 300
    full = _device(eng, mix["arrays"], n, mix["raw"], "sec1", "eip55")
    for drop in ("pk", "address", "status"):
        keep = {k: k != drop for k in ("pk", "address", "status")}
        got = _device(eng, mix["arrays"], n, mix["raw"], "sec1", "eip55", **keep)
        for k in keep:
            assert np.array_equal(got[k], full[k]) if keep[k] else (got[k] == FILL).all(), (drop, k)
        h, r, s, v = (a[:n] for a in mix["arrays"])
        out = dict(zip(("pk", "address", "status"), eng.ecdsa_recover_batch(h, r, s, v, mix["raw"][:n], "sec1", "eip55", want=tuple(k for k in keep if keep[k]))))
        assert out[drop] is None and all(np.array_equal(out[k], full[k]) for k in keep if keep[k])
    got = _device(eng, mix["arrays"], n, None, "sec1", "eip55", pk=False, address=False)      # status alone
    assert np.array_equal(got["status"], mix["status"][:n])
    with pytest.raises(Exception, match="no output array"):
        _device(eng, mix["arrays"], n, None, "sec1", "eip55", pk=False, address=False, status=False)


def test_argument_errors(eng, mix):
    h, r, s, v = (np.ascontiguousarray(a[:4]) for a in mix["arrays"])
    out = np.zeros(4 * 64, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    call = lambda flags, pf, af, n=4, hp=p(h): eng._lib.plume_ecdsa_recover_batch(eng._ctx, flags, pf, af, n, hp, p(r), p(s), p(v), None, p(out), None, None)  # noqa: E731
    assert call(0, 0, 0) == 0
    for bad in ((2, 0, 0), (-1, 0, 0), (0, 2, 0), (0, -1, 0), (0, 0, 3), (0, 0, -1)):
        assert call(*bad) == -1, bad
    assert call(0, 0, 0, 4, None) == -1 and call(0, 0, 0, 0, None) == 0                      # an empty batch is a successful no-op


@pytest.mark.parametrize("lead", [1, 3])
def test_output_arrays_at_odd_byte_offsets_inside_a_larger_tensor(eng, mix, lead):
    import torch
    dev = torch.device(f"cuda:{eng.device_id}")
    n = 300
    stream = torch.cuda.Stream(dev)
    for pf, af in (("sec1", "raw20"), ("sec1", "eip55"), ("affine64", "record64")):          # strides 33 + 20, 33 + 42, 64 + 64
        P, W = K.PK_WIDTH[pf], K.ADDR_WIDTH[af]

        def inside(data, width):
            """`lead` bytes behind the start of a 256-byte aligned allocation, 32 guard bytes in front and behind"""
            big = torch.full((32 + lead + width * n + 32 + 16,), FILL, dtype=torch.uint8, device=dev)
            view = big[32 + lead:32 + lead + width * n]
            if data is not None:
                view.copy_(torch.from_numpy(np.ascontiguousarray(data).reshape(-1)).to(dev))
            return big, view
        ins = [inside(a[:n], w) for a, w in zip(mix["arrays"], (32, 32, 32, 1))]
        bex, vex = inside(mix["raw"][:n], 20)
        bpk, vpk = inside(None, P)
        bad, vad = inside(None, W)
        bst, vst = inside(None, 1)
        assert vad.data_ptr() % 16 == (32 + lead) % 16
        stream.wait_stream(torch.cuda.current_stream(dev))
        eng.ecdsa_recover_batch_device(n, ins[0][1], ins[1][1], ins[2][1], ins[3][1], vex, vpk, vad, vst, pk_format=pf, addr_format=af, stream=stream)
        stream.synchronize()
        wpk, wad, wst = E.recover_batch(*(a[:n] for a in mix["arrays"]), mix["raw"][:n], pf, af)
        assert np.array_equal(vpk.cpu().numpy().reshape(n, P), wpk) and np.array_equal(vad.cpu().numpy().reshape(n, W), wad) and np.array_equal(vst.cpu().numpy(), wst), (pf, af)
        for big, width in ((bpk, P), (bad, W), (bst, 1)):
            b = big.cpu().numpy()
            assert (b[:32 + lead] == FILL).all() and (b[32 + lead + width * n:] == FILL).all(), (pf, af, "guard bytes")
        for (big, view), a, w in zip(ins, mix["arrays"], (32, 32, 32, 1)):
            assert np.array_equal(view.cpu().numpy(), np.ascontiguousarray(a[:n]).reshape(-1))


def test_round_trip_with_the_address_call_and_the_nullifier_set(eng, mix):
    n = 600
    h, r, s, v = (a[:n] for a in mix["arrays"])
    pk, rec, st = eng.ecdsa_recover_batch(h, r, s, v, addr_format="record64")
    ok = st == E.MATCH
    addr2, st2 = eng.eth_address_batch(pk[ok])                                              # 0.11 on the recovered keys gives the recovered addresses
    assert (st2 == K.MATCH).all() and np.array_equal(addr2, rec[ok][:, 44:]) and not rec[:, :44].any()
    _, st3 = eng.eth_address_batch(pk[~ok])
    assert (st3 == K.INVALID).all()                                                         # the zero record of an invalid item is no key
    with eng.nullifier_set() as members:
        fresh, n_fresh = members.insert(rec[ok])
        assert n_fresh == len(np.unique(rec[ok], axis=0)) and members.contains(rec[ok]).all()
        other = rec[ok].copy()
        other[:, 63] ^= 1
        assert not members.contains(other).any()


def test_two_calls_back_to_back_on_a_caller_stream_and_two_shards(eng, mix):
    import torch
    import zk_nullifier_sig_amd as plume
    s = torch.cuda.Stream(torch.device(f"cuda:{eng.device_id}"))
    o1, keep1 = _device(eng, mix["arrays"], 1000, None, "affine64", "eip55", stream=s, sync=False)
    o2, keep2 = _device(eng, mix["arrays"], 257, None, "sec1", "raw20", stream=s, sync=False)
    s.synchronize()
    assert np.array_equal(o1["status"].cpu().numpy(), mix["status"][:1000]) and np.array_equal(o2["address"].cpu().numpy(), mix["raw"][:257])
    assert np.array_equal(o1["address"].cpu().numpy(), E.recover_batch(*(a[:1000] for a in mix["arrays"]), None, "affine64", "eip55")[1])
    del keep1, keep2
    m = plume.Engine([0, 0])
    try:
        h, r, sv, v = (a[:1000] for a in mix["arrays"])
        pk, address, st = m.ecdsa_recover_batch(h, r, sv, v)
        assert np.array_equal(address, mix["raw"][:1000]) and np.array_equal(st, mix["status"][:1000])
        with pytest.raises(plume.PlumeHipError, match="single-device"):
            _device(m, mix["arrays"], 4, None, "affine64", "raw20")
    finally:
        m.close()
