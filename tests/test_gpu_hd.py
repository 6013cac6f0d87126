"""plume_hd_master_batch, plume_hd_derive_priv_batch and plume_hd_derive_pub_batch on the MI355X (include/plume_hip.h; kernels in csrc/plume_hd_kernels.hip, lane bodies in
csrc/plume_hd.h and csrc/plume_sha512.h): byte for byte against the restatement of tests/_hd.py -- itself pinned to BIP-32's test vector 1 and to the Hardhat / Anvil default
accounts.  The kernels run 256-lane workgroups of 64-lane wavefronts: n = 1, 63, 64, 65 (a partial wavefront, a whole one, one lane over), 257 and 1025 (one lane over one
and over four workgroups).  Hardened and non-hardened indices are mixed inside every wavefront at every level (tests/_hd.seeded_paths).  Every comparison is bit-exact and
leaves no item out."""
import numpy as np
import pytest

from tests import _hd as H
from tests import _keccak as K

pytestmark = pytest.mark.gpu

ERR_ARG = -1                                                                 # PLUME_ERR_ARG
PRIV = ("sk", "chain", "pk", "address", "status")
PUB = ("pk", "chain", "address", "status")
PRIV_STAGES = lambda d: ["hd_priv_load"] + ["hd_gmul", "to_affine", "hd_priv_step"] * d + ["hd_gmul", "to_affine", "hd_finish"]  # noqa: E731
PUB_STAGES = lambda d: ["hd_pub_load"] + ["hd_pub_step", "to_affine"] * d + ["hd_finish"]  # noqa: E731


@pytest.fixture(scope="module")
def eng():
    import zk_nullifier_sig_amd as plume
    e = plume.Engine(0)
    yield e
    e.close()


def _same(got, want, names, what):
    for name, w in zip(names, want):
        assert name in got, (what, name)
        g = got[name] if isinstance(got[name], np.ndarray) else got[name].cpu().numpy()
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))[:8])
    bad = want[-1] != 0                                                      # (implied by the comparison; stated because it is the contract: a status means zero records)
    for name in names[:-1]:
        g = got[name] if isinstance(got[name], np.ndarray) else got[name].cpu().numpy()
        assert not g[bad].any(), (what, name)


_REF = {}


def reference(n, depth, salt=0):
    """seeded parents and paths with invalid parents planted among good lanes, and the restatement's answers for both forms -- computed once per shape"""
    key = (n, depth, salt)
    if key not in _REF:
        sk, chain = H.seeded_nodes(n, 1000 * depth + n + salt)
        path = H.seeded_paths(n, depth, 2000 * depth + n + salt)
        if n >= 63:
            for j, v in enumerate((0, H.N, 2**256 - 1)):                     # sk = 0, n, 2^256 - 1 among good lanes
                sk[5 + 19 * j] = np.frombuffer(H.b32(v), np.uint8)
            hard = path[:64] >= H.H
            assert (hard.any(axis=0) & (~hard).any(axis=0)).all()            # hardened and not inside one wavefront at every level
        ppath = path & np.uint32(0x7FFFFFFF)
        pk = H.pk_of(np.where((sk == 0).all(axis=1, keepdims=True) | (sk[:, :1] >= 0x80), np.uint8(1), sk))      # (a stand-in key for the planted scalars)
        if n >= 63:
            ppath[7, depth - 1] = 2**31                                      # a hardened index in the public form
            ppath[40, 0] = 2**32 - 1
            for j, (_, rec) in enumerate(K.invalid_keys("affine64")):        # off curve, all-zero, coordinates >= p, ... among good lanes
                pk[3 + 8 * j] = np.frombuffer(rec, np.uint8)
        _REF[key] = dict(sk=sk, chain=chain, path=path, ppath=ppath, pk=pk, priv=H.derive_priv_batch(sk, chain, path, depth), pub=H.derive_pub_batch(pk, chain, ppath, depth))
    return _REF[key]


@pytest.mark.parametrize("n,depth", [(1, 1), (63, 5), (64, 8), (65, 5), (257, 1), (1025, 1)])
def test_private_and_public_forms_against_the_restatement(eng, n, depth):
    ref = reference(n, depth)
    _same(eng.hd_derive_priv_batch(ref["sk"], ref["chain"], ref["path"]), ref["priv"], PRIV, "private, host form")
    _same(eng.hd_derive_pub_batch(ref["pk"], ref["chain"], ref["ppath"]), ref["pub"], PUB, "public, host form")
    if n >= 63:
        st = ref["priv"][4]
        assert [int(st[5 + 19 * j]) for j in range(3)] == [H.BAD_SCALAR] * 3 and (st == 0).sum() == n - 3      # the neighbours of the planted lanes are derived
        st = ref["pub"][3]
        assert st[7] == st[40] == H.HARDENED_PUB and (st[3:3 + 8 * 7:8] == H.BAD_SCALAR).all() and (st == 0).sum() == n - 9
    # the device form, everything resident: equal to the host form
    eng.set_stage_timing(True)
    try:
        _same(eng.hd_derive_priv_batch(ref["sk"], ref["chain"], ref["path"], device=True), ref["priv"], PRIV, "private, device form")
        assert [k for k, _ in eng.last_stage_times()] == PRIV_STAGES(depth)
        _same(eng.hd_derive_pub_batch(ref["pk"], ref["chain"], ref["ppath"], device=True), ref["pub"], PUB, "public, device form")
        assert [k for k, _ in eng.last_stage_times()] == PUB_STAGES(depth)
    finally:
        eng.set_stage_timing(False)


@pytest.mark.parametrize("pk_format", ["affine64", "sec1"])
@pytest.mark.parametrize("addr_format", ["raw20", "record64", "eip55"])
def test_every_record_format(eng, pk_format, addr_format):
    ref = reference(65, 2)
    want = H.derive_priv_batch(ref["sk"], ref["chain"], ref["path"], 2, 0, pk_format, addr_format)
    _same(eng.hd_derive_priv_batch(ref["sk"], ref["chain"], ref["path"], pk_format, addr_format), want, PRIV, (pk_format, addr_format))
    pk = H.pk_of(np.where((ref["sk"] == 0).all(axis=1, keepdims=True) | (ref["sk"][:, :1] >= 0x80), np.uint8(1), ref["sk"]), pk_format)
    for j, (_, rec) in enumerate(K.invalid_keys(pk_format)):                 # SEC1: prefix 00, 04, 05, x >= p, x with no root
        pk[3 + 8 * j] = np.frombuffer(rec, np.uint8)
    want = H.derive_pub_batch(pk, ref["chain"], ref["ppath"], 2, 0, pk_format, addr_format)
    assert (want[3][3:3 + 8 * 7:8] == H.BAD_SCALAR).all()
    _same(eng.hd_derive_pub_batch(pk, ref["chain"], ref["ppath"], pk_format, addr_format), want, PUB, (pk_format, addr_format, "public"))


def _at(torch, dev, arr, shift, fill=0xAA):
    """the bytes of arr in device memory `shift` bytes behind a 16-byte boundary, between guard bytes; returns (buffer, view)"""
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    buf = torch.full((32 + 16 + raw.size + 32,), fill, dtype=torch.uint8, device=dev)
    view = buf[32 + shift:32 + shift + raw.size]
    view.copy_(torch.from_numpy(raw.copy()))
    return buf, view


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_device_form_with_every_array_off_its_alignment(eng, shift):
    import torch
    dev = torch.device("cuda", eng.device_id)
    n, depth = 65, 5
    ref = reference(n, depth)
    for pub, parent, path, want, names in ((False, ref["sk"], ref["path"], ref["priv"], PRIV), (True, ref["pk"], ref["ppath"], ref["pub"], PUB)):
        ins = [_at(torch, dev, a, shift + j) for j, a in enumerate((parent, ref["chain"], path))]
        outs = {name: _at(torch, dev, np.zeros_like(w), shift + j, fill=0x55) for j, (name, w) in enumerate(zip(names, want))}
        st = torch.cuda.Stream(dev)
        st.wait_stream(torch.cuda.current_stream(dev))
        eng.hd_derive_batch_device(pub, 0, n, ins[0][1], ins[1][1], ins[2][1], depth, None if pub else outs["sk"][1], outs["chain"][1], outs["pk"][1], outs["address"][1],
                                   outs["status"][1], stream=st)
        st.synchronize()
        got = {name: outs[name][1].cpu().numpy().reshape(w.shape) for name, w in zip(names, want)}
        _same(got, want, names, ("pub" if pub else "priv", shift))
        for name, (buf, view) in outs.items():                               # nothing outside the arrays is written
            b = buf.cpu().numpy()
            lo = 32 + shift + list(names).index(name)
            assert (b[:lo] == 0x55).all() and (b[lo + view.numel():] == 0x55).all(), name
        for (buf, view), a in zip(ins, (parent, ref["chain"], path)):        # the inputs are unchanged
            assert np.array_equal(view.cpu().numpy(), np.ascontiguousarray(a).view(np.uint8).reshape(-1))


def test_shared_parent_and_shared_path(eng):
    n, depth = 65, 5
    ref = reference(n, depth)
    sk1, c1, p1 = ref["sk"][:1], ref["chain"][:1], ref["path"][:1]
    pk1, pp1 = ref["pk"][:1], ref["ppath"][:1]
    for device in (False, True):
        _same(eng.hd_derive_priv_batch(sk1, c1, ref["path"], device=device), H.derive_priv_batch(sk1, c1, ref["path"], depth, H.SHARED_PARENT), PRIV, ("shared parent", device))
        _same(eng.hd_derive_priv_batch(ref["sk"], ref["chain"], p1, device=device), H.derive_priv_batch(ref["sk"], ref["chain"], p1, depth, H.SHARED_PATH), PRIV, ("shared path", device))
        _same(eng.hd_derive_pub_batch(pk1, c1, ref["ppath"], device=device), H.derive_pub_batch(pk1, c1, ref["ppath"], depth, H.SHARED_PARENT), PUB, ("pub, shared parent", device))
        _same(eng.hd_derive_pub_batch(ref["pk"], ref["chain"], pp1, device=device), H.derive_pub_batch(ref["pk"], ref["chain"], pp1, depth, H.SHARED_PATH), PUB, ("pub, shared path", device))
    # both together: every item is the same child.  The façade tells n from its arrays, so this one goes through the ABI
    import ctypes as C
    m = 70
    out = {k: np.zeros((m, w), np.uint8) for k, w in (("sk", 32), ("chain", 32), ("pk", 64), ("address", 20))}
    status = np.full(m, 0xFF, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = eng._lib.plume_hd_derive_priv_batch(eng._ctx, 3, 0, 0, m, p(np.ascontiguousarray(sk1)), p(np.ascontiguousarray(c1)), p(np.ascontiguousarray(p1)), depth, p(out["sk"]),
                                             p(out["chain"]), p(out["pk"]), p(out["address"]), p(status))
    assert rc == 0
    want = H.derive_priv_batch(sk1, c1, p1, depth, 3, n=m)
    _same(dict(out, status=status), want, PRIV, "both shared")
    assert want[4][0] == 0 and (out["sk"] == out["sk"][0]).all()


def test_known_answers(eng):
    # BIP-32 test vector 1
    sk, chain, status = eng.hd_master_batch(np.frombuffer(H.V1_SEED, np.uint8).reshape(1, 16))
    assert (sk[0].tobytes().hex(), chain[0].tobytes().hex(), int(status[0])) == (H.V1["m"][0], H.V1["m"][1], 0)
    got = eng.hd_derive_priv_batch(sk, chain, np.array([[H.H]], np.uint32))
    assert (got["sk"][0].tobytes().hex(), got["chain"][0].tobytes().hex()) == H.V1["m/0'"][:2]
    got2 = eng.hd_derive_priv_batch(sk, chain, np.array([[H.H, 1]], np.uint32))
    assert (got2["sk"][0].tobytes().hex(), got2["chain"][0].tobytes().hex()) == H.V1["m/0'/1"][:2]
    pub = eng.hd_derive_pub_batch(got["pk"], got["chain"], np.array([[1]], np.uint32), want=("chain",))      # CKDpub from (m/0') G gives (m/0'/1) G and the same chain
    assert np.array_equal(pub["pk"], got2["pk"]) and np.array_equal(pub["chain"], got2["chain"])
    # the Hardhat / Anvil accounts: the depth-5 path from the master, and CKDpub from the account node's public key
    seed = H.hardhat_seed()
    assert seed.hex() == H.HARDHAT_SEED
    sk, chain, status = eng.hd_master_batch(np.frombuffer(seed, np.uint8).reshape(1, 64))
    assert status[0] == 0
    path = np.array([H.parse_path(f"{H.HARDHAT_ACCOUNT_PATH}/{i}") for i in range(3)], np.uint32)
    kids = eng.hd_derive_priv_batch(sk, chain, path)
    assert [r.tobytes().hex() for r in kids["sk"]] == [c[0] for c in H.HARDHAT_CHILDREN] and [r.tobytes().hex() for r in kids["address"]] == [c[1] for c in H.HARDHAT_CHILDREN]
    acct = eng.hd_derive_priv_batch(sk, chain, np.array([H.parse_path(H.HARDHAT_ACCOUNT_PATH)], np.uint32))
    assert (acct["sk"][0].tobytes().hex(), acct["chain"][0].tobytes().hex()) == H.HARDHAT_ACCOUNT
    watch = eng.hd_derive_pub_batch(acct["pk"], acct["chain"], np.arange(3, dtype=np.uint32).reshape(3, 1))
    assert np.array_equal(watch["address"], kids["address"]) and np.array_equal(watch["pk"], kids["pk"]) and np.array_equal(watch["chain"], kids["chain"])


@pytest.mark.parametrize("seed_len", [16, 33, 64])
def test_master_batch(eng, seed_len):
    import torch
    n = 257
    seeds = np.random.default_rng(seed_len).integers(0, 256, (n, seed_len), dtype=np.uint8)
    want = H.master_batch(seeds, seed_len)
    got = eng.hd_master_batch(seeds)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    dev = torch.device("cuda", eng.device_id)
    s = _at(torch, dev, seeds, 1)
    outs = [_at(torch, dev, np.zeros_like(w), 2 + j, fill=0x55) for j, w in enumerate(want)]
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    eng.hd_master_batch_device(n, s[1], seed_len, outs[0][1], outs[1][1], outs[2][1], stream=st)
    st.synchronize()
    for j, ((buf, view), w) in enumerate(zip(outs, want)):
        assert np.array_equal(view.cpu().numpy().reshape(w.shape), w)
        b = buf.cpu().numpy()
        assert (b[:32 + 2 + j] == 0x55).all() and (b[32 + 2 + j + view.numel():] == 0x55).all()


def test_chunks_sub_batches_and_uniform_levels(eng):
    n, depth = 1025, 1
    ref = reference(n, depth)
    level0 = eng.sign_uniform()
    try:
        for chunk in (1025, 513, 100):                                        # one piece, two, many
            eng.set_chunk(chunk)
            _same(eng.hd_derive_priv_batch(ref["sk"], ref["chain"], ref["path"]), ref["priv"], PRIV, ("chunk", chunk))
            _same(eng.hd_derive_pub_batch(ref["pk"], ref["chain"], ref["ppath"]), ref["pub"], PUB, ("chunk", chunk, "public"))
        # a shared parent is staged as a secret and wiped behind every piece: it has to reach every piece all the same
        _same(eng.hd_derive_priv_batch(ref["sk"][1:2], ref["chain"][1:2], ref["path"]), H.derive_priv_batch(ref["sk"][1:2], ref["chain"][1:2], ref["path"], depth, H.SHARED_PARENT),
              PRIV, "shared parent in pieces")
        import zk_nullifier_sig_amd as plume
        with pytest.raises(plume.PlumeHipError):                             # the device form takes at most one chunk
            eng.hd_derive_priv_batch(ref["sk"], ref["chain"], ref["path"], device=True)
        eng.set_chunk(1 << 20)
        ref5 = reference(65, 5)
        for level in (0, 1, 2):
            eng.set_sign_uniform(level)
            _same(eng.hd_derive_priv_batch(ref5["sk"], ref5["chain"], ref5["path"], device=True), ref5["priv"], PRIV, ("uniform level", level))
        eng.set_sign_uniform(level0)
        eng.set_sub_batches(3)
        _same(eng.hd_derive_priv_batch(ref["sk"], ref["chain"], ref["path"], device=True), ref["priv"], PRIV, "three sub-batches")
        _same(eng.hd_derive_pub_batch(ref["pk"], ref["chain"], ref["ppath"], device=True), ref["pub"], PUB, "three sub-batches, public")
    finally:
        eng.set_chunk(1 << 20)
        eng.set_sub_batches(1)
        eng.set_sign_uniform(level0)


def test_cross_check_at_size(eng):
    """2^16 items against the library's own older kernels instead of the slow restatement, which checks a seeded sample of 256"""
    import torch
    n, depth = 1 << 16, 2
    sk, chain = H.seeded_nodes(n, 65536)
    path = H.seeded_paths(n, depth, 65537)
    priv = eng.hd_derive_priv_batch(sk, chain, path, device=True)
    dev = priv["sk"].device
    assert int(priv["status"].count_nonzero()) == 0
    # derive_pub(sk_par G, ...) equals the child_pk of derive_priv.  The parents are the 2^16 nodes one level down -- sk_par G is the pk the private form reports for
    # them --, their last level is taken both ways
    ppath = path & np.uint32(0x7FFFFFFF)
    both = eng.hd_derive_priv_batch(sk, chain, ppath, device=True)
    par = eng.hd_derive_priv_batch(sk, chain, ppath[:, :1], device=True)
    last = torch.from_numpy(np.ascontiguousarray(ppath[:, 1:]).view(np.int32)).to(dev)
    pub = eng.hd_derive_pub_batch(par["pk"], par["chain"], last, want=("chain", "address"), device=True)
    assert int(pub["status"].count_nonzero()) == 0
    assert torch.equal(pub["pk"], both["pk"]) and torch.equal(pub["chain"], both["chain"]) and torch.equal(pub["address"], both["address"])
    # the address equals eth_address_batch(child_pk)
    addr, st = eng.eth_address_batch(priv["pk"].cpu().numpy())
    assert (st == 1).all() and np.array_equal(addr, priv["address"].cpu().numpy())
    # the restatement on a seeded sample of 256
    idx = np.sort(np.random.default_rng(256).choice(n, 256, replace=False))
    want = H.derive_priv_batch(sk[idx], chain[idx], path[idx], depth)
    pick = torch.from_numpy(idx).to(dev)
    _same({k: v[pick] for k, v in priv.items()}, want, PRIV, "sample")


def test_end_to_end_on_the_device_into_the_transaction_signer(eng):
    import torch

    from tests import _eth_tx as T
    n = 257
    seed = H.hardhat_seed()
    sk, chain, _ = eng.hd_master_batch(np.frombuffer(seed, np.uint8).reshape(1, 64))
    acct = eng.hd_derive_priv_batch(sk, chain, np.array([H.parse_path(H.HARDHAT_ACCOUNT_PATH)], np.uint32))
    kids = eng.hd_derive_priv_batch(acct["sk"], acct["chain"], np.arange(n, dtype=np.uint32).reshape(n, 1), addr_format="eip55", device=True)
    assert int(kids["status"].count_nonzero()) == 0
    assert kids["address"][0].cpu().numpy().tobytes() == b"0xf39Fd6e51aad88F6F4ce6aB8827279cffFb92266"
    dev = kids["sk"].device
    rng = np.random.default_rng(1559)
    items = [T.signing_data(2, T.default_fields(2, 31337, rng.integers(0, 256, int(rng.integers(0, 70)), dtype=np.uint8).tobytes(), salt=i)) for i in range(n)]   # type-02 payloads
    txs, off = T.pack(items)
    nbytes = int(off[-1])
    d_txs, d_off = torch.from_numpy(txs).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev)
    out = torch.zeros(nbytes + 68 * n, dtype=torch.uint8, device=dev)
    out_len, status = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    eng.eth_tx_sign_batch_device(n, d_txs, d_off, nbytes, kids["sk"], None, out, out.numel(), out_len, status, stream=st)      # the derived sk tensor, no host copy
    st.synchronize()
    assert int(status.count_nonzero()) == 0
    ob, ln = out.cpu().numpy().tobytes(), out_len.cpu().numpy()
    raws = [ob[int(off[i]) + 68 * i:][:int(ln[i])] for i in range(n)]
    stx, soff = T.pack(raws)
    _, address, st, _, _ = eng.eth_tx_sender_batch(stx, soff, addr_format="eip55")
    assert (st == 1).all() and np.array_equal(address, kids["address"].cpu().numpy())


def test_argument_errors_and_the_empty_batch(eng):
    import ctypes as C
    lib, ctx = eng._lib, eng._ctx
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.plume_hd_master_batch(ctx, 0, None, 16, None, None, None) == 0
    assert lib.plume_hd_derive_priv_batch(ctx, 0, 0, 0, 0, None, None, None, 1, None, None, None, None, None) == 0
    assert lib.plume_hd_derive_pub_batch(ctx, 0, 0, 0, 0, None, None, None, 1, None, None, None, None) == 0
    n = 4
    ref = reference(1, 1)
    sk, chain = H.seeded_nodes(n, 7)
    path = np.zeros((n, 8), np.uint32)
    o_sk, o_chain, o_pk, o_ad = (np.full((n, w), 0x77, np.uint8) for w in (32, 32, 64, 20))
    st = np.full(n, 0x77, np.uint8)
    untouched = lambda: all((a == 0x77).all() for a in (o_sk, o_chain, o_pk, o_ad, st))  # noqa: E731
    priv = lambda flags, depth, args=None, fmt=(0, 0): lib.plume_hd_derive_priv_batch(ctx, flags, fmt[0], fmt[1], n, *(args or [p(sk), p(chain), p(path)]), depth,  # noqa: E731
                                                                                   p(o_sk), p(o_chain), p(o_pk), p(o_ad), p(st))
    for depth in (0, 9, 2**40):
        assert priv(0, depth) == ERR_ARG and untouched()
    for flags in (4, 8, 0x103):
        assert priv(flags, 1) == ERR_ARG and untouched()
    for fmt in ((2, 0), (0, 3), (-1, 0)):
        assert priv(0, 1, fmt=fmt) == ERR_ARG and untouched()
    for missing in range(3):
        args = [p(sk), p(chain), p(path)]
        args[missing] = None
        assert priv(0, 1, args) == ERR_ARG and untouched()
    assert lib.plume_hd_derive_priv_batch(ctx, 0, 0, 0, n, p(sk), p(chain), p(path), 1, None, p(o_chain), p(o_pk), p(o_ad), p(st)) == ERR_ARG and untouched()     # child_sk is required
    assert lib.plume_hd_derive_priv_batch(ctx, 0, 0, 0, n, p(sk), p(chain), p(path), 1, p(o_sk), p(o_chain), p(o_pk), p(o_ad), None) == ERR_ARG and untouched()  # status too
    pk = H.pk_of(sk)
    assert lib.plume_hd_derive_pub_batch(ctx, 0, 0, 0, n, p(pk), p(chain), p(path), 1, None, p(o_chain), p(o_ad), p(st)) == ERR_ARG and untouched()                 # child_pk is required
    assert lib.plume_hd_derive_pub_batch(ctx, 0, 0, 0, n, p(pk), p(chain), p(path), 9, p(o_pk), p(o_chain), p(o_ad), p(st)) == ERR_ARG and untouched()
    seeds = np.zeros((n, 64), np.uint8)
    for seed_len in (0, 15, 65, 128):
        assert lib.plume_hd_master_batch(ctx, n, p(seeds), seed_len, p(o_sk), p(o_chain), p(st)) == ERR_ARG and untouched()
    assert lib.plume_hd_master_batch(ctx, n, None, 16, p(o_sk), p(o_chain), p(st)) == ERR_ARG and untouched()
    assert lib.plume_hd_master_batch(None, n, p(seeds), 16, p(o_sk), p(o_chain), p(st)) == ERR_ARG
    # the optional outputs may be NULL
    assert lib.plume_hd_derive_priv_batch(ctx, 0, 0, 0, n, p(sk), p(chain), p(path), 8, p(o_sk), None, None, None, p(st)) == 0
    want = H.derive_priv_batch(sk, chain, path, 8)
    assert np.array_equal(o_sk, want[0]) and np.array_equal(st, want[4]) and (o_chain == 0x77).all() and (o_pk == 0x77).all() and (o_ad == 0x77).all()
    # a zero sk fed on into a signer reports BAD_SCALAR there
    bad = eng.hd_derive_priv_batch(np.zeros((1, 32), np.uint8), ref["chain"], ref["path"])
    assert bad["status"][0] == H.BAD_SCALAR and not bad["sk"].any()
    _, _, _, sst = eng.ecdsa_sign_batch(np.zeros((1, 32), np.uint8), bad["sk"])
    assert sst[0] == 2
