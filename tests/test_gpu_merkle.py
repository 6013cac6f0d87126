"""plume_merkle_leaf_batch / _tree_build / _proof_batch / _verify_batch on the GPU (k_merkle_leaf, k_merkle_sort_*, k_merkle_place, k_merkle_level, k_merkle_top,
k_merkle_proof, k_merkle_verify) against the restatement of tests/_merkle.py: the committed fixture through every call in host and device forms, the device arrays at byte
offsets 1 and 4 with the bytes around every output untouched; a size sweep n = 2^k - 1, 2^k, 2^k + 1 for k = 0 .. 12 and n = 2^16 + 3, sorted and unsorted -- the smallest
shapes that cross a single node, two leaf depths, the fused top's 256-node depth, the LDS tile's last local merge and the first stages in the workspace -- with every proof
(or a seeded 4096) verified and one mutated element per proof refused; raw transactions to a root and back, all on the device.
Expected trees above 256 leaves are made level by level with plume_eth_message_hash_batch (mode 0: the keccak_stream kernel, pinned by its own tests) over 64-byte pairs
ordered with numpy; expected orders come from numpy.lexsort."""
import numpy as np
import pytest

from tests import _merkle as M

pytestmark = pytest.mark.gpu

FILL = 0xAA
SWEEP = sorted({n for k in range(13) for n in (2**k - 1, 2**k, 2**k + 1) if n >= 1}) + [2**16 + 3]
LEAF_NAMES = {0: "hash32", 1: "address", 2: "address_uint256"}
ADDR_NAMES = {0: "raw20", 1: "record64"}


@pytest.fixture(scope="module")
def eng():
    import zk_nullifier_sig_amd as plume
    e = plume.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def kats():
    return M.load_kats()


def _u8(hexstr, *shape):
    return np.frombuffer(bytes.fromhex(hexstr), np.uint8).reshape(*shape).copy()


def _tree_inputs(t):
    W = M.item_width(t["leaf_format"], t["addr_format"])
    return _u8(t["items"], t["n"], W), None if t["amounts"] is None else _u8(t["amounts"], t["n"], 32)


# ------------------------------------------------------------------------------------------------ the fixture, host forms
def test_the_fixture_through_the_host_forms(eng, kats):
    trees = {}
    for t in kats["trees"]:
        items, amounts = _tree_inputs(t)
        n, lf, af = t["n"], LEAF_NAMES[t["leaf_format"]], ADDR_NAMES[t["addr_format"]]
        leaf, st = eng.merkle_leaf_batch(items, amounts, lf, af)
        assert leaf.tobytes().hex() == t["leaves"] and list(st) == t["leaf_status"], t["name"]
        tree, pos = eng.merkle_tree_build(leaf, bool(t["sort"]))
        assert tree.tobytes().hex() == t["tree"] and list(pos) == t["leaf_pos"], t["name"]
        assert eng.merkle_max_proof_len(n) == t["depth"] == M.max_proof_len(n)
        proof, ln = eng.merkle_proof_batch(tree, pos)
        assert proof.shape == (n, t["depth"], 32) and proof.tobytes().hex() == t["proofs"] and list(ln) == t["proof_len"], t["name"]
        trees[t["name"]] = tree
    assert trees["openzeppelin readme"][0].tobytes().hex() == kats["oz_root"] == "d4dee0beab2d53f2cc83e567171bd2820e49898130a22622b10ead383e90bd77"
    for c in kats["proof_cases"]:
        proof, ln = eng.merkle_proof_batch(trees[c["tree"]], np.array(c["pos"], np.uint32), c["depth"])
        assert proof.tobytes().hex() == c["proofs"] and list(ln) == c["proof_len"], (c["tree"], c["depth"])
    for c in kats["verify_cases"]:
        m, W = len(c["status"]), M.item_width(c["leaf_format"], c["addr_format"])
        st = eng.merkle_verify_batch(_u8(c["items"], m, W), _u8(c["proofs"], m, c["depth"], 32), np.array(c["proof_len"], np.uint8), _u8(c["root"], 32),
                                     None if c["amounts"] is None else _u8(c["amounts"], m, 32), LEAF_NAMES[c["leaf_format"]], ADDR_NAMES[c["addr_format"]])
        assert list(st) == c["status"], (c["tree"], [w for w, a, b in zip(c["what"], st, c["status"]) if a != b])


def test_arguments(eng, kats):
    from zk_nullifier_sig_amd import capi
    leaf = np.zeros((4, 32), np.uint8)
    with pytest.raises(capi.PlumeHipError):
        eng.merkle_leaf_batch(np.zeros((2, 42), np.uint8), None, "address", "eip55")
    with pytest.raises(capi.PlumeHipError):
        eng.merkle_tree_build(np.zeros((0, 32), np.uint8))
    fn = eng._lib.plume_merkle_tree_build
    tree = np.zeros((7, 32), np.uint8)
    assert fn(eng._ctx, 2, 4, capi._ptr(leaf), capi._ptr(tree), None) == -1          # an unknown flag bit
    assert fn(eng._ctx, 1, (1 << 26) + 1, capi._ptr(leaf), capi._ptr(tree), None) == -1
    assert fn(eng._ctx, 1, 4, capi._ptr(leaf), capi._ptr(tree), None) == 0           # leaf_pos is optional
    assert eng._lib.plume_merkle_leaf_batch(eng._ctx, 3, 0, 4, capi._ptr(leaf), None, capi._ptr(tree), None) == -1
    assert eng._lib.plume_merkle_leaf_batch(eng._ctx, 2, 0, 4, capi._ptr(leaf), None, capi._ptr(tree), None) == -1   # no amounts
    assert eng.merkle_proof_batch(tree, np.zeros(0, np.uint32))[1].shape == (0,) and eng.merkle_leaf_batch(np.zeros((0, 20), np.uint8))[0].shape == (0, 32)
    assert [eng.merkle_max_proof_len(n) for n in (0, 1, 2, 3, 4, 5, 2**26)] == [0, 0, 1, 2, 2, 3, 26]


# ------------------------------------------------------------------------------------------------ the fixture, device forms at byte offsets
def _dev_bytes(dev, data, shift):
    import torch
    data = np.ascontiguousarray(data).reshape(-1)
    t = torch.full((len(data) + 64,), FILL, dtype=torch.uint8, device=dev)
    if len(data):
        t[shift:shift + len(data)] = torch.from_numpy(data).to(dev)
    return t


def _out(dev, nbytes):
    import torch
    return torch.full((nbytes + 64,), FILL, dtype=torch.uint8, device=dev)


def _take(t, shift, nbytes, what):
    a = t.cpu().numpy()
    assert (a[:shift] == FILL).all() and (a[shift + nbytes:] == FILL).all(), f"{what}: bytes outside the array were written"
    return a[shift:shift + nbytes]


@pytest.mark.parametrize("shift", [1, 4, 0])
def test_the_fixture_through_the_device_forms(eng, kats, shift):
    import torch
    dev = torch.device(f"cuda:{eng.device_id}")
    stream = torch.cuda.Stream(dev)
    for t in kats["trees"]:
        items, amounts = _tree_inputs(t)
        n, depth, lf, af = t["n"], t["depth"], LEAF_NAMES[t["leaf_format"]], ADDR_NAMES[t["addr_format"]]
        d_items, d_amt = _dev_bytes(dev, items, shift), None if amounts is None else _dev_bytes(dev, amounts, shift + 1)
        d_leaf, d_st, d_tree, d_proof, d_len, d_vst = _out(dev, 32 * n), _out(dev, n), _out(dev, 32 * (2 * n - 1)), _out(dev, 32 * depth * n), _out(dev, n), _out(dev, n)
        d_pos = torch.full((n + 2,), -1, dtype=torch.int32, device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            eng.merkle_leaf_batch_device(n, d_items[shift:], None if d_amt is None else d_amt[shift + 1:], d_leaf[shift:], d_st[shift + 2:], lf, af, stream=stream)
            eng.merkle_tree_build_device(n, d_leaf[shift:], d_tree[shift:], d_pos[1:], bool(t["sort"]), stream=stream)
            eng.merkle_proof_batch_device(n, d_tree[shift:], n, d_pos[1:], depth, d_proof[shift + 3:], d_len[shift:], stream=stream)
            eng.merkle_verify_batch_device(n, d_items[shift:], None if d_amt is None else d_amt[shift + 1:], depth, d_proof[shift + 3:], d_len[shift:], d_tree[shift:],
                                           d_vst[shift + 5:], lf, af, stream=stream)
        stream.synchronize()
        assert _take(d_leaf, shift, 32 * n, "leaf").tobytes().hex() == t["leaves"] and list(_take(d_st, shift + 2, n, "status")) == t["leaf_status"], t["name"]
        assert _take(d_tree, shift, 32 * (2 * n - 1), "tree").tobytes().hex() == t["tree"], t["name"]
        pos = d_pos.cpu().numpy()
        assert pos[0] == -1 and pos[-1] == -1 and list(pos[1:-1]) == t["leaf_pos"], t["name"]
        assert _take(d_proof, shift + 3, 32 * depth * n, "proof").tobytes().hex() == t["proofs"] and list(_take(d_len, shift, n, "proof_len")) == t["proof_len"], t["name"]
        assert list(_take(d_vst, shift + 5, n, "verify status")) == [1 if s == 1 else 3 for s in t["leaf_status"]], t["name"]
    for c in kats["verify_cases"]:
        m, depth = len(c["status"]), c["depth"]
        d_items, d_proof, d_len, d_root = (_dev_bytes(dev, _u8(c["items"], -1), shift), _dev_bytes(dev, _u8(c["proofs"], -1), shift + 2),
                                           _dev_bytes(dev, np.array(c["proof_len"], np.uint8), shift), _dev_bytes(dev, _u8(c["root"], 32), shift + 7))
        d_amt = None if c["amounts"] is None else _dev_bytes(dev, _u8(c["amounts"], -1), shift)
        d_vst = _out(dev, m)
        eng.merkle_verify_batch_device(m, d_items[shift:], None if d_amt is None else d_amt[shift:], depth, d_proof[shift + 2:] if depth else None, d_len[shift:],
                                       d_root[shift + 7:], d_vst[shift:], LEAF_NAMES[c["leaf_format"]], ADDR_NAMES[c["addr_format"]])
        torch.cuda.synchronize(dev)
        assert list(_take(d_vst, shift, m, "verify status")) == c["status"], c["tree"]


def test_stage_lists(eng):
    import torch
    dev = torch.device(f"cuda:{eng.device_id}")
    eng.set_stage_timing(True)
    try:
        for n, sort, want in ((300, True, ["merkle_sort", "merkle_place", "merkle_top"]), (1, True, ["merkle_place"]), (2, False, ["merkle_place", "merkle_top"]),
                              (512, False, ["merkle_place", "merkle_top"]), (513, True, ["merkle_sort", "merkle_place", "merkle_levels", "merkle_top"])):
            leaf = torch.from_numpy(np.random.default_rng(n).integers(0, 256, (n, 32), dtype=np.uint8)).to(dev)
            tree = torch.empty((2 * n - 1, 32), dtype=torch.uint8, device=dev)
            eng.merkle_tree_build_device(n, leaf, tree, None, sort)
            torch.cuda.synchronize(dev)
            assert [k for k, _ in eng.last_stage_times()] == want, n
    finally:
        eng.set_stage_timing(False)


# ------------------------------------------------------------------------------------------------ the size sweep
def _gt(a, b):
    """a > b, rows of bytes compared as big-endian numbers"""
    diff = a != b
    first = diff.argmax(axis=1)
    r = np.arange(len(a))
    return diff.any(axis=1) & (a[r, first] > b[r, first])


def _expected_tree(eng, leaves, sort):
    """(tree, leaf_pos) by numpy and the message-hash call"""
    n = len(leaves)
    order = np.lexsort((np.arange(n),) + tuple(leaves[:, 31 - k] for k in range(32))) if sort else np.arange(n)
    tree = np.zeros((2 * n - 1, 32), np.uint8)
    tree[n - 1:] = leaves[order][::-1]
    leaf_pos = np.zeros(n, np.uint32)
    leaf_pos[order] = 2 * n - 2 - np.arange(n)
    d = (n - 1).bit_length() - 1 if n >= 2 else -1
    while d >= 0:
        idx = np.arange(2**d - 1, min(2**(d + 1) - 2, n - 2) + 1)
        a, b = tree[2 * idx + 1], tree[2 * idx + 2]
        swap = _gt(a, b)[:, None]
        pairs = np.concatenate([np.where(swap, b, a), np.where(swap, a, b)], axis=1)
        msgs = np.concatenate([pairs.reshape(-1), np.zeros(16, np.uint8)])
        tree[idx] = eng.eth_message_hash_batch(msgs, np.arange(len(idx) + 1, dtype=np.uint64) * 64, "keccak256")
        d -= 1
    return tree, leaf_pos


def _expected_proofs(tree, pos, depth):
    t = pos.astype(np.int64)
    out, ln = np.zeros((len(pos), depth, 32), np.uint8), np.floor(np.log2(t + 1)).astype(np.uint8)
    for s in range(depth):
        act = t > 0
        sib = np.where(t & 1, t + 1, t - 1)
        out[act, s] = tree[sib[act]]
        t = np.where(act, (t - 1) // 2, t)
    return out, ln


def test_the_helper_of_the_sweep_agrees_with_the_restatement(eng):
    for n in (1, 2, 3, 6, 37):
        rng = np.random.default_rng(n)
        leaves = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        if n > 3:
            leaves[3] = leaves[1]
        for sort in (True, False):
            tree, pos = _expected_tree(eng, leaves, sort)
            wt, wp = M.build([x.tobytes() for x in leaves], sort)
            assert tree.tobytes() == b"".join(wt) and list(pos) == wp, (n, sort)
            d = M.max_proof_len(n)
            p, ln = _expected_proofs(tree, pos, d)
            q, lq = M.proof_batch(wt, wp, d)
            assert np.array_equal(p, q) and np.array_equal(ln, lq), (n, sort)


@pytest.mark.parametrize("n", SWEEP)
def test_size_sweep(eng, n):
    rng = np.random.default_rng(1000 + n)
    leaves = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if n > 4:
        leaves[n // 2] = leaves[1]                                            # a duplicate leaf: the input index decides
        leaves[n - 1] = leaves[0]
        leaves[n - 1, 31] ^= 1                                                # ... and a pair that differs in its last bit
    depth = M.max_proof_len(n)
    for sort in (True, False):
        if n <= 256:
            wt, wp = M.build([x.tobytes() for x in leaves], sort)
            want_tree, want_pos = np.frombuffer(b"".join(wt), np.uint8).reshape(-1, 32), np.array(wp, np.uint32)
        else:
            want_tree, want_pos = _expected_tree(eng, leaves, sort)
        tree, pos = eng.merkle_tree_build(leaves, sort)
        assert np.array_equal(pos, want_pos), (n, sort, np.flatnonzero(pos != want_pos)[:8])
        assert np.array_equal(tree, want_tree), (n, sort, np.flatnonzero((tree != want_tree).any(axis=1))[:8])
        pick = np.arange(n) if n <= 4096 else np.sort(rng.choice(n, 4096, replace=False))
        proof, ln = eng.merkle_proof_batch(tree, pos[pick], depth)
        wproof, wln = _expected_proofs(want_tree, want_pos[pick], depth)
        assert np.array_equal(ln, wln) and np.array_equal(proof, wproof), (n, sort)
        st = eng.merkle_verify_batch(leaves[pick], proof, ln, tree[0], leaf_format="hash32")
        assert (st == M.MATCH).all(), (n, sort, np.flatnonzero(st != M.MATCH)[:8])
        if depth:
            mut = proof.copy()
            k = np.arange(len(pick))
            live = ln > 0
            mut[k[live], (k % np.maximum(ln, 1))[live], (k % 32)[live]] ^= (1 << (k % 8)).astype(np.uint8)[live]
            st = eng.merkle_verify_batch(leaves[pick], mut, ln, tree[0], leaf_format="hash32")
            assert (st[live] == M.MISMATCH).all() and (st[~live] == M.MATCH).all(), (n, sort, np.flatnonzero(st[live] != M.MISMATCH)[:8])


# ------------------------------------------------------------------------------------------------ raw transactions to a root and back
def test_transactions_to_root_and_back_on_the_device(eng):
    import torch
    from tests import _eth_tx as T
    items = [e for e in T.load_kats()["items"] if e["sk"] is not None and not e["high_s"] and e["status"] == T.OK and int(e["r"], 16) != 0]
    assert len(items) > 100
    txs, off = T.pack([bytes.fromhex(e["raw"]) for e in items])
    n, nbytes = len(items), int(off[-1])
    dev = torch.device(f"cuda:{eng.device_id}")
    d_txs, d_off = torch.from_numpy(txs).to(dev), torch.from_numpy(off.view(np.int64)).to(dev)
    rec = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
    st = torch.zeros(n, dtype=torch.uint8, device=dev)
    leaf = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    lst = torch.empty(n, dtype=torch.uint8, device=dev)
    tree = torch.empty((2 * n - 1, 32), dtype=torch.uint8, device=dev)
    pos = torch.empty(n, dtype=torch.int32, device=dev)
    depth = eng.merkle_max_proof_len(n)
    proof = torch.empty((n, depth, 32), dtype=torch.uint8, device=dev)
    ln = torch.empty(n, dtype=torch.uint8, device=dev)
    vst = torch.empty(n, dtype=torch.uint8, device=dev)
    eng.eth_tx_sender_batch_device(n, d_txs, d_off, nbytes, None, None, rec, None, None, st, addr_format="record64")
    eng.merkle_leaf_batch_device(n, rec, None, leaf, lst, "address", "record64")
    eng.merkle_tree_build_device(n, leaf, tree, pos, True)
    eng.merkle_proof_batch_device(n, tree, n, pos, depth, proof, ln)
    eng.merkle_verify_batch_device(n, rec, None, depth, proof, ln, tree, vst, "address", "record64")       # the root is the tree's first node, where it lies
    torch.cuda.synchronize(dev)
    assert (st.cpu().numpy() == 1).all() and (lst.cpu().numpy() == M.MATCH).all() and (vst.cpu().numpy() == M.MATCH).all()
    senders = [T.sender_of(bytes.fromhex(e["sk"]))[1] for e in items]
    assert rec.cpu().numpy()[:, 44:].tobytes() == b"".join(senders)
    want_tree, want_pos = M.build([M.leaf_of(M.LEAF_ADDRESS, M.ADDR_RAW20, a) for a in senders], sort=True)
    assert tree[0].cpu().numpy().tobytes() == want_tree[0] and list(pos.cpu().numpy()) == want_pos
    other = rec.clone()
    other[5, 63] ^= 1                                                        # somebody who is not on the list, and a record that is no address record
    other[9, 3] = 1
    eng.merkle_verify_batch_device(n, other, None, depth, proof, ln, tree, vst, "address", "record64")
    torch.cuda.synchronize(dev)
    got = vst.cpu().numpy()
    assert got[5] == M.MISMATCH and got[9] == M.INVALID and (np.delete(got, [5, 9]) == M.MATCH).all()
