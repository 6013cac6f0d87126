"""plume_eth_tx_parse_batch / plume_eth_tx_sender_batch on the GPU (k_eth_tx_parse, then the recover stages) against the restatement of tests/_eth_tx.py: the committed
fixture byte for byte at batch sizes around the wavefront and the block, 2 048 single-byte mutants in every output, the device form at odd byte offsets with the bytes
around every output untouched and rejected offsets invalid, the sender call against parse + ecdsa_recover_batch and against the signers' own keys in every format, the
stage list, and a plume_init_multi context."""
import numpy as np
import pytest

from tests import _ecdsa as E
from tests import _eth_tx as T
from tests import _keccak as K

pytestmark = pytest.mark.gpu

FILL = 0xAA
NAMES = ("hash", "r", "s", "v", "chain_id", "tx_type", "status")
SIZES = (1, 63, 64, 65, 255, 256, 257)
RECOVER_STAGES = ["ecdsa_prepare", "tables", "ecdsa_mul", "to_affine", "ecdsa_finalize"]


@pytest.fixture(scope="module")
def eng():
    import zk_nullifier_sig_amd as plume
    e = plume.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def fixture():
    """the committed items, packed, with what the fixture says of them as the arrays the library writes (checked against the restatement on the CPU:
    tests/test_eth_tx_restatement.py)"""
    items = T.load_kats()["items"]
    txs, off = T.pack([bytes.fromhex(e["raw"]) for e in items])
    n = len(items)
    arr = lambda key: np.frombuffer(b"".join(bytes.fromhex(e[key]) for e in items), np.uint8).reshape(n, 32).copy()  # noqa: E731
    want = {"hash": arr("hash"), "r": arr("r"), "s": arr("s"), "v": np.array([e["v"] for e in items], np.uint8), "chain_id": np.array([int(e["chain_id"]) for e in items], np.uint64),
            "tx_type": np.array([e["tx_type"] for e in items], np.uint8), "status": np.array([e["status"] for e in items], np.uint8)}
    assert n >= max(SIZES)
    return items, txs, off, want


@pytest.fixture(scope="module")
def mutant_batch(fixture):
    items = fixture[0]
    raws = [bytes.fromhex(e["raw"]) for e in items if e["status"] == T.OK and len(e["raw"]) < 2000]
    txs, off = T.pack(T.mutants(raws, 2048, 20261018))
    return txs, off, T.parse_batch(txs, off)


def _same(got, want, what, upto=None):
    for k in NAMES:
        w = want[k] if upto is None else want[k][:upto]
        assert got[k].dtype == w.dtype and np.array_equal(got[k], w), (what, k, np.flatnonzero((got[k].reshape(len(w), -1) != w.reshape(len(w), -1)).any(axis=1))[:8])


def test_the_fixture_byte_for_byte_at_sizes_around_the_block(eng, fixture):
    items, txs, off, want = fixture
    _same(eng.eth_tx_parse_batch(txs, off), want, "the whole fixture")
    for n in SIZES:                                                          # the last wavefront is partial
        _same(eng.eth_tx_parse_batch(txs, off[:n + 1]), want, n, upto=n)
    e155 = T.load_kats()["eip155"]
    got = eng.eth_tx_parse_batch(*T.pack([bytes.fromhex(e155["raw"])]))
    assert got["hash"][0].tobytes().hex() == e155["hash"] and got["r"][0].tobytes().hex() == e155["r"] and got["s"][0].tobytes().hex() == e155["s"]
    assert (int(got["v"][0]), int(got["chain_id"][0]), int(got["tx_type"][0]), int(got["status"][0])) == (0, 1, 0, T.OK)
    txid = eng.eth_message_hash_batch(*T.pack([bytes.fromhex(e155["raw"])]), "keccak256")       # the transaction id is the existing call's
    assert txid[0].tobytes().hex() == e155["id"]


def test_every_output_of_2048_mutants(eng, mutant_batch):
    txs, off, want = mutant_batch
    valid = int((want["status"] == T.OK).sum())
    assert 200 <= valid <= 1848, valid
    _same(eng.eth_tx_parse_batch(txs, off), want, "mutants")


def _device_parse(eng, txs, off, nbytes, shift_in, shift_out, optional=True):
    import torch
    n = len(off) - 1
    dev = torch.device(f"cuda:{eng.device_id}")
    dm = torch.full((len(txs) + 64,), FILL, dtype=torch.uint8, device=dev)
    dm[shift_in:shift_in + len(txs)] = torch.from_numpy(np.ascontiguousarray(txs)).to(dev)
    width = {"hash": 32, "r": 32, "s": 32, "v": 1, "tx_type": 1, "status": 1}
    outs = {k: torch.full((w * n + 64,), FILL, dtype=torch.uint8, device=dev) for k, w in width.items()}
    chain = torch.full((n + 2,), -1, dtype=torch.int64, device=dev)
    doff = torch.from_numpy(np.ascontiguousarray(off).view(np.int64)).to(dev)
    sh = {k: (shift_out + 3 * j) % 16 for j, k in enumerate(width)}
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    eng.eth_tx_parse_batch_device(n, dm[shift_in:], doff, nbytes, outs["hash"][sh["hash"]:], outs["r"][sh["r"]:], outs["s"][sh["s"]:], outs["v"][sh["v"]:],
                                  chain[1:] if optional else None, outs["tx_type"][sh["tx_type"]:] if optional else None, outs["status"][sh["status"]:] if optional else None,
                                  stream=st)
    st.synchronize()
    got = {}
    for k, w in width.items():
        a = outs[k].cpu().numpy()
        if not optional and k in ("tx_type", "status"):
            assert (a == FILL).all(), k
            continue
        assert (a[:sh[k]] == FILL).all() and (a[sh[k] + w * n:] == FILL).all(), f"{k}: bytes outside the array were written"
        got[k] = a[sh[k]:sh[k] + w * n].reshape((n, 32) if w == 32 else (n,))
    c = chain.cpu().numpy()
    if optional:
        assert c[0] == -1 and c[-1] == -1
        got["chain_id"] = c[1:-1].view(np.uint64)
    else:
        assert (c == -1).all()
    return got


def test_device_form_at_odd_offsets_and_rejected_offsets(eng, fixture):
    items, txs, off, want = fixture
    nbytes = int(off[-1])
    for shift_in, shift_out in ((1, 3), (7, 0), (0, 5), (4, 9)):
        _same(_device_parse(eng, txs, off, nbytes, shift_in, shift_out), want, (shift_in, shift_out))
    got = _device_parse(eng, txs, off, nbytes, 3, 1, optional=False)           # chain_id, tx_type and status are optional
    for k in ("hash", "r", "s", "v"):
        assert np.array_equal(got[k], want[k]), k
    bad = off.copy()
    bad[6] = bad[5] - 1                                                      # item 5 runs backwards; item 6 then starts one byte early
    cut = int(off[200]) + 1                                                  # ... and everything from item 200 on reaches past txs_bytes
    w = T.parse_batch(txs, bad, txs_bytes=cut)
    assert w["status"][5] == T.INVALID and (w["status"][200:] == T.INVALID).all() and (w["status"][:200] == T.OK).sum() > 100
    _same(_device_parse(eng, txs[:cut], bad, cut, 5, 2), w, "rejected offsets")


@pytest.fixture(scope="module")
def signers(fixture):
    """{item index: (public key, address)} of every item somebody signed: sk G by the restatement, once"""
    return {i: T.sender_of(bytes.fromhex(e["sk"])) for i, e in enumerate(fixture[0]) if e["sk"] is not None}


@pytest.mark.parametrize("low_s", [True, False])
def test_sender_equals_parse_then_recover_and_the_signers_keys(eng, fixture, signers, low_s):
    items, txs, off, want = fixture
    n = len(items)
    parsed = eng.eth_tx_parse_batch(txs, off)
    signed, keys = sorted(signers), signers
    assert len(signed) > 100 and any(items[i]["high_s"] for i in signed)
    for pf in ("affine64", "sec1"):
        for af in ("raw20", "record64", "eip55"):
            for with_expect in (False, True):
                expect = None
                if with_expect:
                    expect = np.zeros((n, 20), np.uint8)
                    for i in signed:
                        expect[i] = np.frombuffer(keys[i][1], np.uint8)
                    expect[signed[7], 19] ^= 1                               # one mismatch planted
                pk, addr, st, chain, typ = eng.eth_tx_sender_batch(txs, off, expect=expect, pk_format=pf, addr_format=af, low_s=low_s)
                rpk, raddr, rst = eng.ecdsa_recover_batch(parsed["hash"], parsed["r"], parsed["s"], parsed["v"], expect=expect, pk_format=pf, addr_format=af, low_s=low_s)
                what = (pf, af, with_expect, low_s)
                assert np.array_equal(pk, rpk) and np.array_equal(addr, raddr) and np.array_equal(st, rst), what
                assert np.array_equal(chain, want["chain_id"]) and np.array_equal(typ, want["tx_type"]), what
                assert (st[want["status"] == T.INVALID] == 3).all() and not pk[want["status"] == T.INVALID].any() and not addr[want["status"] == T.INVALID].any(), what
                for i in signed:
                    if low_s and items[i]["high_s"]:
                        assert st[i] == 3 and not pk[i].any() and not addr[i].any(), (what, items[i]["name"])
                        continue
                    assert pk[i].tobytes() == E.pk_record(keys[i][0], pf) and addr[i].tobytes() == K.record_of(keys[i][1], af), (what, items[i]["name"])
                    assert st[i] == (0 if with_expect and i == signed[7] else 1), (what, items[i]["name"])
    rzero = [i for i, e in enumerate(items) if e["status"] == T.OK and int(e["r"], 16) == 0]
    assert rzero and (st[rzero] == 3).all() and (typ[rzero] == want["tx_type"][rzero]).all() and (chain[rzero] == want["chain_id"][rzero]).all()


def test_sender_device_form_stage_list_and_arguments(eng, fixture):
    import torch
    from zk_nullifier_sig_amd import capi
    items, txs, off, want = fixture
    n, nbytes = len(items), int(off[-1])
    dev = torch.device(f"cuda:{eng.device_id}")
    host = eng.eth_tx_sender_batch(txs, off)
    dm = torch.from_numpy(np.ascontiguousarray(txs[:nbytes])).to(dev)
    doff = torch.from_numpy(off.view(np.int64)).to(dev)
    pk = torch.full((64 * n + 64,), FILL, dtype=torch.uint8, device=dev)
    addr = torch.full((20 * n + 64,), FILL, dtype=torch.uint8, device=dev)
    status = torch.full((n + 64,), FILL, dtype=torch.uint8, device=dev)
    typ = torch.full((n + 64,), FILL, dtype=torch.uint8, device=dev)
    chain = torch.full((n,), -1, dtype=torch.int64, device=dev)
    eng.set_stage_timing(True)
    try:
        st = torch.cuda.Stream(dev)
        st.wait_stream(torch.cuda.current_stream(dev))
        eng.eth_tx_sender_batch_device(n, dm, doff, nbytes, None, pk[1:], addr[3:], chain, typ[5:], status[7:], stream=st)
        st.synchronize()
        assert [k for k, _ in eng.last_stage_times()] == ["eth_tx_parse"] + RECOVER_STAGES
        d = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        eng.eth_tx_parse_batch_device(n, dm, doff, nbytes, d, d.clone(), d.clone(), torch.empty(n, dtype=torch.uint8, device=dev))
        torch.cuda.synchronize(dev)
        assert [k for k, _ in eng.last_stage_times()] == ["eth_tx_parse"]
    finally:
        eng.set_stage_timing(False)
    for t, sh, w, ref in ((pk, 1, 64, host[0]), (addr, 3, 20, host[1]), (status, 7, 1, host[2]), (typ, 5, 1, host[4])):
        a = t.cpu().numpy()
        assert (a[:sh] == FILL).all() and (a[sh + w * n:] == FILL).all() and np.array_equal(a[sh:sh + w * n], ref.reshape(-1)), w
    assert np.array_equal(chain.cpu().numpy().view(np.uint64), host[3])
    try:
        eng.set_chunk(100)
        for k, a in enumerate(eng.eth_tx_sender_batch(txs, off)):            # the host form cuts the batch into pieces
            assert np.array_equal(a, host[k]), k
        _same(eng.eth_tx_parse_batch(txs, off), want, "chunks of 100")
        with pytest.raises(capi.PlumeHipError):                              # the device form of the sender takes at most one chunk
            eng.eth_tx_sender_batch_device(n, dm, doff, nbytes, None, pk, addr, chain, typ, status)
        eng.set_chunk(1 << 20)
        eng.set_sub_batches(2)
        for k, a in enumerate(eng.eth_tx_sender_batch(txs, off)):
            assert np.array_equal(a, host[k]), k
    finally:
        eng.set_chunk(1 << 20)
        eng.set_sub_batches(1)
    empty = eng.eth_tx_parse_batch(np.zeros(16, np.uint8), np.zeros(1, np.uint64))
    assert empty["hash"].shape == (0, 32) and eng.eth_tx_sender_batch(np.zeros(16, np.uint8), np.zeros(1, np.uint64))[2].shape == (0,)
    down = off[:9].copy()
    down[4] = down[3] - 1
    with pytest.raises(capi.PlumeHipError):                                  # the host forms refuse offsets that decrease
        eng.eth_tx_parse_batch(txs, down)
    with pytest.raises(capi.PlumeHipError):
        eng.eth_tx_sender_batch(txs, down)
    p = capi._ptr
    o = {k: np.zeros((4, 64), np.uint8) for k in "abc"}
    fn = eng._lib.plume_eth_tx_sender_batch
    assert fn(eng._ctx, 0, 0, 0, 4, p(txs), p(off), None, p(o["a"]), p(o["b"]), None, None, p(o["c"])) == 0
    for flags, pf, af in ((2, 0, 0), (0x100, 0, 0), (0, 2, 0), (0, 0, 3), (0, -1, 0)):
        assert fn(eng._ctx, flags, pf, af, 4, p(txs), p(off), None, p(o["a"]), p(o["b"]), None, None, p(o["c"])) != 0, (flags, pf, af)
    assert fn(eng._ctx, 0, 0, 0, 4, p(txs), p(off), None, None, None, None, None, None) != 0
    assert eng._lib.plume_eth_tx_parse_batch(eng._ctx, 4, p(txs), p(off), p(o["a"]), p(o["b"]), p(o["c"]), None, None, None, None) != 0      # v is required


def test_a_three_shard_context_gives_the_same_bytes(eng, fixture, mutant_batch):
    import zk_nullifier_sig_amd as plume
    items, txs, off, want = fixture
    multi = plume.Engine([eng.device_id] * 3)
    try:
        _same(multi.eth_tx_parse_batch(txs, off), want, "plume_init_multi([d, d, d])")
        _same(multi.eth_tx_parse_batch(mutant_batch[0], mutant_batch[1]), mutant_batch[2], "plume_init_multi([d, d, d]), mutants")
        one, three = eng.eth_tx_sender_batch(txs, off, addr_format="eip55"), multi.eth_tx_sender_batch(txs, off, addr_format="eip55")
        for k, (a, b) in enumerate(zip(one, three)):
            assert np.array_equal(a, b), k
    finally:
        multi.close()
