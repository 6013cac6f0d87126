"""plume_eth_tx_sign_batch on the MI355X (include/plume_hip.h; kernels k_eth_tx_sign_frame and k_eth_tx_sign_assemble in csrc/plume_eth_tx_sign_kernels.hip, lane bodies in
csrc/plume_eth_tx_sign.h, the unchanged ECDSA sign stages between them): byte for byte against the restatement of tests/_eth_tx_sign.py -- itself pinned to EIP-155's
published example and to the 108 signed items of tests/golden/eth_tx_kats.json -- over both fixtures as one batch of 424 items (the four ~65 KB items next to 100-byte ones,
framed and unframed items interleaved inside every 64-lane wavefront), and round trips through the library's own receiving side: plume_eth_tx_sender_batch,
plume_eth_tx_parse_batch.  Every comparison is bit-exact and leaves no item out."""
import numpy as np
import pytest

from tests import _ecdsa as E
from tests import _eth_tx as T
from tests import _eth_tx_sign as X
from tests import _keccak as K

pytestmark = pytest.mark.gpu

FILL = 0xAA
RECORDS = ("hash", "r", "s", "v", "chain_id", "tx_type")
ERR_ARG = -1                                                                 # PLUME_ERR_ARG
SIGN_STAGES = ["ecdsa_sign_nonce", "ecdsa_sign_gmul", "to_affine", "ecdsa_sign_finalize"]
RECOVER_STAGES = ["ecdsa_prepare", "tables", "ecdsa_mul", "to_affine", "ecdsa_finalize"]


@pytest.fixture(scope="module")
def eng():
    import zk_nullifier_sig_amd as plume
    e = plume.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def batch():
    """both fixtures as one batch and the restatement's answer, computed once"""
    items, keys = X.fixture_batch()
    txs, off = T.pack(items)
    sk = np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 32).copy()
    want = X.sign_batch(txs, off, sk)
    framed = np.array([X.frame_unsigned(it) is not None for it in items])
    for b in range(0, len(items), 64):                                       # framed and unframed items inside every wavefront
        assert 0 < framed[b:b + 64].sum() < len(framed[b:b + 64])
    assert (want["status"] == 0).sum() == 108 + 4 + 11 and sum(len(it) > 60000 for it in items) == 4
    return dict(items=items, keys=keys, txs=txs, off=off, sk=sk, want=want)


@pytest.fixture(scope="module")
def plain(eng, batch):
    """the host-form call over the whole batch, made once"""
    return eng.eth_tx_sign_slots(batch["txs"], batch["off"], batch["sk"])


def _same(got, want, off, what):
    assert np.array_equal(got["status"], want["status"]), (what, "status", np.flatnonzero(got["status"] != want["status"])[:8])
    assert np.array_equal(got["out_len"], want["out_len"]), (what, "out_len")
    assert got["out"].shape == want["out"].shape
    bad = np.flatnonzero(got["out"] != want["out"])
    assert bad.size == 0, (what, "out differs first at byte", int(bad[0]))
    for k in RECORDS:
        if k in got:
            assert np.array_equal(got[k], want[k]), (what, k)
    for (start, length), ln in zip(X.slot_bounds(off), got["out_len"]):     # (implied by the comparison above; stated because it is the contract)
        assert not got["out"][start + int(ln):start + length].any()


def test_both_fixtures_in_one_host_call(eng, batch, plain):
    _same(plain, batch["want"], batch["off"], "host form")
    assert (plain["out_len"] <= np.diff(batch["off"]).astype(np.int64) + X.GROWTH).all()
    n, nbytes = len(batch["items"]), int(batch["off"][-1])
    assert eng._lib.plume_eth_tx_sign_out_bytes(n, nbytes) == nbytes + 68 * n == plain["out"].size
    # the committed vectors, by name
    kats = {e["unsigned"]: e for e in X.load_kats()["items"]}
    raws = X.compact(plain["out"], plain["out_len"], batch["off"])
    seen = 0
    for it, raw, st in zip(batch["items"], raws, plain["status"]):
        e = kats.get(it.hex())
        if e is not None:
            assert (raw.hex(), int(st)) == (e["raw"], e["status"]), e["name"]
            seen += 1
    assert seen >= 56
    # the façade's compaction
    raw2, st2, rec = eng.eth_tx_sign_batch(batch["items"], batch["sk"], records=True)
    assert raw2 == raws and np.array_equal(st2, plain["status"]) and np.array_equal(rec["chain_id"], batch["want"]["chain_id"])


def test_eip155_example_and_all_108_fixture_transactions(eng):
    kats = T.load_kats()
    ex = kats["eip155"]
    es = [e for e in kats["items"] if e["sk"] and not e["high_s"] and e["status"] == T.OK]
    assert len(es) == 108
    unsigned = [bytes.fromhex(ex["signing_data"])] + [X.unsigned_of(bytes.fromhex(e["raw"])) for e in es]
    sk = np.frombuffer(bytes.fromhex(ex["sk"]) + b"".join(bytes.fromhex(e["sk"]) for e in es), np.uint8)
    raw, st = eng.eth_tx_sign_batch(unsigned, sk)
    assert not st.any()
    assert raw[0].hex() == ex["raw"]
    assert [r.hex() for r in raw[1:]] == [e["raw"] for e in es]


def test_chunks_and_shards_give_identical_bytes(eng, batch, plain):
    import zk_nullifier_sig_amd as plume
    try:
        eng.set_chunk(64)                                                    # seven pieces, the last partial
        _same(eng.eth_tx_sign_slots(batch["txs"], batch["off"], batch["sk"]), plain, batch["off"], "chunks of 64")
        eng.set_chunk(1000)
        sub = slice(5, 70)                                                   # a call whose first offset is not zero
        got = eng.eth_tx_sign_slots(batch["txs"], batch["off"][5:71], batch["sk"][sub])
        raws = X.compact(plain["out"], plain["out_len"], batch["off"])
        assert X.compact(got["out"], got["out_len"], batch["off"][5:71]) == raws[sub] and np.array_equal(got["status"], plain["status"][sub])
    finally:
        eng.set_chunk(1 << 20)
    multi = plume.Engine([eng.device_id] * 3)
    try:
        _same(multi.eth_tx_sign_slots(batch["txs"], batch["off"], batch["sk"]), plain, batch["off"], "plume_init_multi([d, d, d])")
    finally:
        multi.close()


def _device(eng, n, txs, off, sk, aux=None, shift=0, out_bytes=None, txs_bytes=None, records=True):
    """one device-form call on the first n items into tensors pre-filled with FILL, every byte array `shift` bytes into its tensor"""
    import torch
    dev = torch.device(f"cuda:{eng.device_id}")
    off = np.ascontiguousarray(off[:n + 1])
    nbytes = int(off[n]) if txs_bytes is None else txs_bytes
    full = int(off[n]) - int(off[0]) + X.GROWTH * n
    out_bytes = full if out_bytes is None else out_bytes

    def t(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        x = torch.full((a.size + 16,), FILL, dtype=torch.uint8, device=dev)
        x[shift:shift + a.size] = torch.from_numpy(a).to(dev)
        return x[shift:]
    dt = t(txs[:nbytes])
    doff = torch.from_numpy(off.view(np.int64)).to(dev)
    dsk, daux = t(sk[:n]), None if aux is None else t(aux[:n])
    width = dict(out=None, status=1, hash=32, r=32, s=32, v=1, tx_type=1)
    o = {k: torch.full(((out_bytes if w is None else w * n) + 64,), FILL, dtype=torch.uint8, device=dev) for k, w in width.items() if records or k in ("out", "status")}
    out_len = torch.full((n + 2,), -1, dtype=torch.int32, device=dev)
    chain = torch.full((n + 2,), -1, dtype=torch.int64, device=dev) if records else None
    lead = 32 + shift                                                        # guard bytes in front of every byte array as well
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    eng.eth_tx_sign_batch_device(n, dt, doff, nbytes, dsk, daux, o["out"][lead:], out_bytes, out_len[1:], o["status"][lead:],
                                 **({k2: o[k][lead:] for k, k2 in (("hash", "hash32"), ("r", "r"), ("s", "s"), ("v", "v"), ("tx_type", "tx_type"))} if records else {}),
                                 chain_id=None if chain is None else chain[1:], stream=st)
    st.synchronize()
    res = {}
    for k, x in o.items():
        g = x.cpu().numpy()
        size = out_bytes if width[k] is None else width[k] * n
        assert (g[:lead] == FILL).all() and (g[lead + size:] == FILL).all(), f"{k}: bytes outside the array were written"
        res[k] = g[lead:lead + size].reshape((n, 32) if width[k] == 32 else (-1,))
    gl = out_len.cpu().numpy()
    assert gl[0] == -1 and gl[-1] == -1
    res["out_len"] = gl[1:-1].astype(np.uint32)
    if chain is not None:
        gc = chain.cpu().numpy()
        assert gc[0] == -1 and gc[-1] == -1
        res["chain_id"] = gc[1:-1].astype(np.uint64)
    return res


def test_device_form_at_odd_offsets_with_guards_and_a_cut_slot(eng, batch, plain):
    n, off = len(batch["items"]), batch["off"]
    for shift in (1, 3):
        got = _device(eng, n, batch["txs"], off, batch["sk"], shift=shift)
        _same(got, plain, off, f"device form, arrays at byte offset {shift}")
    # an out_bytes that cuts the last slot by one byte: that item reports BAD_TX and writes nothing, its neighbours are intact
    m = max(j for j in range(n) if plain["status"][j] == 0) + 1              # end the batch with an item that is signed
    full = int(off[m]) + X.GROWTH * m
    got = _device(eng, m, batch["txs"], off, batch["sk"], shift=1, out_bytes=full - 1)
    start = X.slot_bounds(off[:m + 1])[m - 1][0]
    assert got["status"][m - 1] == X.BAD_TX and got["out_len"][m - 1] == 0 and not got["hash"][m - 1].any() and got["chain_id"][m - 1] == 0
    assert np.array_equal(got["status"][:m - 1], plain["status"][:m - 1]) and np.array_equal(got["out_len"][:m - 1], plain["out_len"][:m - 1])
    assert np.array_equal(got["out"][:start], plain["out"][:start])
    assert (got["out"][start:] == FILL).all()                                # the cut item wrote no byte of out
    # offsets the span rule rejects: txs_bytes ends inside item 9
    cut = int(off[9]) + 1
    want = X.sign_batch(batch["txs"], off[:13], batch["sk"][:12], txs_bytes=cut)
    got = _device(eng, 12, batch["txs"], off, batch["sk"], shift=3, txs_bytes=cut)
    assert np.array_equal(got["status"], want["status"]) and (got["status"][9:] == X.BAD_TX).all()
    s9 = X.slot_bounds(off[:13])[9][0]
    assert np.array_equal(got["out"][:s9], want["out"][:s9]) and (got["out"][s9:] == FILL).all()


def _round_trip(eng, batch, res, what, signed):
    """the compacted output through the receiving side: every signed item recovers the address of sk G, and the parser reports what the signer reported"""
    off = batch["off"]
    raws = X.compact(res["out"], res["out_len"], off)
    good = np.flatnonzero(res["status"] == 0)
    assert len(good) == signed                                               # the count the restatement predicts
    txs2, off2 = T.pack([raws[j] for j in good])
    pk, address, status, chain_id, tx_type = eng.eth_tx_sender_batch(txs2, off2, low_s=True)
    assert (status == E.MATCH).all(), what
    for k, j in enumerate(good):
        q, addr = T.sender_of(batch["keys"][j])
        assert address[k].tobytes() == addr and pk[k].tobytes() == E.pk_record(q, "affine64"), (what, j)
    p = eng.eth_tx_parse_batch(txs2, off2)
    assert (p["status"] == T.OK).all()
    for k in ("hash", "r", "s", "v", "chain_id", "tx_type"):
        assert np.array_equal(p[k], res[k][good]), (what, k)
    assert np.array_equal(chain_id, res["chain_id"][good]) and np.array_equal(tx_type, res["tx_type"][good])


def test_round_trip_through_sender_and_parse(eng, batch, plain):
    _round_trip(eng, batch, plain, "plain", int((batch["want"]["status"] == 0).sum()))


def test_aux_selfcheck_and_uniform_levels(eng, batch, plain):
    n, off = len(batch["items"]), batch["off"]
    aux = np.frombuffer(b"".join(K.keccak256(b"aux %d" % j) for j in range(n)), np.uint8).reshape(n, 32)
    hedged = eng.eth_tx_sign_slots(batch["txs"], off, batch["sk"], aux)
    want = X.sign_batch(batch["txs"], off, batch["sk"], aux)
    _same(hedged, want, off, "hedged")
    # An item with chainId 2^63 - 18 is signed when its nonce gives parity 0 and refused (v = 2^64) when it gives 1, and aux changes the nonce: such items may be signed in one
    # call and refused in the other.  How many items are signed in both is the restatement's to say
    good = (plain["status"] == 0) & (hedged["status"] == 0)
    assert good.sum() == ((batch["want"]["status"] == 0) & (want["status"] == 0)).sum() > 100 and np.array_equal(hedged["status"] == X.BAD_TX, plain["status"] == X.BAD_TX) and not np.array_equal(hedged["out"], plain["out"])
    assert all(not np.array_equal(hedged["r"][j], plain["r"][j]) for j in np.flatnonzero(good))
    assert np.array_equal(hedged["hash"][good], plain["hash"][good])
    _round_trip(eng, batch, hedged, "hedged", int((want["status"] == 0).sum()))
    level0 = eng.sign_uniform()
    eng.set_stage_timing(True)
    try:
        _same(_device(eng, n, batch["txs"], off, batch["sk"]), plain, off, "device form")
        assert [k for k, _ in eng.last_stage_times()] == ["eth_tx_sign_frame"] + SIGN_STAGES + ["eth_tx_sign_assemble"]
        eng.set_sign_selfcheck(1)
        _same(eng.eth_tx_sign_slots(batch["txs"], off, batch["sk"]), plain, off, "self-check, host form")
        _same(_device(eng, n, batch["txs"], off, batch["sk"], shift=1), plain, off, "self-check, device form")
        assert [k for k, _ in eng.last_stage_times()] == ["eth_tx_sign_frame"] + SIGN_STAGES + RECOVER_STAGES + ["ecdsa_sign_release", "eth_tx_sign_assemble"]
        eng.set_sign_selfcheck(0)
        for level in (0, 1, 2):
            eng.set_sign_uniform(level)
            _same(_device(eng, n, batch["txs"], off, batch["sk"], records=False), {k: plain[k] for k in ("out", "out_len", "status")}, off, ("uniform level", level))
        eng.set_sign_uniform(level0)
        eng.set_sub_batches(2)
        _same(_device(eng, n, batch["txs"], off, batch["sk"]), plain, off, "two sub-batches")
    finally:
        eng.set_sub_batches(1)
        eng.set_sign_uniform(level0)
        eng.set_stage_timing(False)
        eng.set_sign_selfcheck(0)


def test_argument_errors_and_the_empty_batch(eng, batch):
    import ctypes as C

    from zk_nullifier_sig_amd import capi
    raw, st = eng.eth_tx_sign_batch([], np.zeros((0, 32), np.uint8))
    assert raw == [] and st.shape == (0,)
    fn = eng._lib.plume_eth_tx_sign_batch
    assert fn(eng._ctx, 0, 0, None, None, None, None, None, None, None, None, None, None, None, None, None) == 0
    items = batch["items"][:4]
    txs, off = T.pack(items)
    sk = batch["sk"][:4].copy()
    out, out_len, status = np.zeros(len(txs) + 68 * 4, np.uint8), np.zeros(4, np.uint32), np.zeros(4, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    nul = [None] * 6
    assert fn(eng._ctx, 0, 4, p(txs), p(off), p(sk), None, p(out), p(out_len), *nul, p(status)) == 0
    assert np.array_equal(status, batch["want"]["status"][:4])
    for flags in (1, 2, 0x100):                                              # flags must be 0 for now
        assert fn(eng._ctx, flags, 4, p(txs), p(off), p(sk), None, p(out), p(out_len), *nul, p(status)) == ERR_ARG
    for missing in range(5):                                                 # tx_off, sk, out, out_len, status are required
        args = [p(off), p(sk), p(out), p(out_len), p(status)]
        args[missing] = None
        assert fn(eng._ctx, 0, 4, p(txs), args[0], args[1], None, args[2], args[3], *nul, args[4]) == ERR_ARG, missing
    bad = off.copy()
    bad[2] = bad[1] - 1                                                      # decreasing offsets: an argument error in the host form
    with pytest.raises(capi.PlumeHipError):
        eng.eth_tx_sign_slots(txs, bad, sk)
    assert fn(None, 0, 4, p(txs), p(off), p(sk), None, p(out), p(out_len), *nul, p(status)) == ERR_ARG
    try:
        eng.set_chunk(64)
        with pytest.raises(capi.PlumeHipError):                              # the device form takes at most one chunk
            _device(eng, 100, batch["txs"], batch["off"], batch["sk"])
    finally:
        eng.set_chunk(1 << 20)
