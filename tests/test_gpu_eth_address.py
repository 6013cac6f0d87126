"""plume_eth_address_batch on the MI355X (include/plume_hip.h; kernel in csrc/plume_eth_kernels.hip, lane body in csrc/plume_keccak.h): the Ethereum address of every public
key, byte for byte against the pure-Python restatement of tests/_keccak.py (pinned by tests/test_eth_keccak_restatement.py) and the public vectors of
tests/golden/eth_address_kats.json.  The block is 256 lanes: batch sizes 1, 255, 256, 257, 1000."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

from tests import _keccak as K

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
KATS = json.loads((ROOT / "tests" / "golden" / "eth_address_kats.json").read_text())
PKF, ADF = ("affine64", "sec1"), ("raw20", "record64", "eip55")
N = 1000
PLANTED = (0, 37, 100, 300, 511, 768, 999)          # first, mid-wavefront, ..., last: one position per kind of invalid key
FILL = 0xAA


def test_a_context_that_only_computes_addresses_builds_no_table():
    """first in the file, on a context of its own: the call works, and device memory does not drop by anything like a table (the verifier's window table is 1 GiB, the
    signer's comb 252 MiB); the project's accounting for that is torch.cuda.mem_get_info around open / use / close, as tests/test_gpu_round5.py uses it"""
    import torch
    import zk_nullifier_sig_amd as plume
    keys = np.frombuffer(b"".join(bytes.fromhex(v["pk"]) for v in KATS["addresses"]), np.uint8)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info(0)
    e = plume.Engine(0)
    try:
        free1, _ = torch.cuda.mem_get_info(0)
        address, status = e.eth_address_batch(keys, addr_format="eip55")
        assert [a.tobytes().decode() for a in address] == [v["address"] for v in KATS["addresses"]] and list(status) == [K.MATCH] * 3
        big = np.tile(keys.reshape(3, 64), (1 << 16, 1))
        address, status = e.eth_address_batch(big)
        assert (status == K.MATCH).all() and np.array_equal(address[:3], address[-3:])
        rc = e._lib.plume_eth_address_batch(e._ctx, 0, 0, 3, keys.ctypes.data_as(C.c_void_p), None, None, None)
        assert rc != 0 and e._lib.plume_last_error() == b"no output array"
        torch.cuda.synchronize()
        free2, _ = torch.cuda.mem_get_info(0)
    finally:
        e.close()
    assert free1 - free2 < (128 << 20), (free0, free1, free2)        # staging of 3 * 2^16 items is 17 MiB


@pytest.fixture(scope="module")
def eng():
    import zk_nullifier_sig_amd as plume
    e = plume.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ref():
    """N keys in both formats with every invalid kind planted at PLANTED, and what the restatement says about them, computed once: raw addresses, records in the three
    formats, status without expect"""
    pts = K.sample_keys(N, 5)
    raw = np.zeros((N, 20), np.uint8)
    eip = np.zeros((N, 42), np.uint8)
    for i in range(N):
        if i in PLANTED:
            continue
        a = K.address_of(K.decode_pk(pts[i].tobytes()))
        raw[i] = np.frombuffer(a, np.uint8)
        eip[i] = np.frombuffer(K.eip55(a).encode(), np.uint8)
    status = np.full(N, K.MATCH, np.uint8)
    status[list(PLANTED)] = K.INVALID
    keys = {"affine64": pts.copy(), "sec1": np.concatenate([2 + (pts[:, 63:64] & 1), pts[:, :32]], axis=1)}
    for fmt in PKF:
        bad = K.invalid_keys(fmt)
        assert len(bad) == len(PLANTED)
        for pos, (_, rec) in zip(PLANTED, bad):
            keys[fmt][pos] = np.frombuffer(rec, np.uint8)
        for i in (1, 36, 38, 998):                                    # spot checks of the shortcut above against the whole restatement
            a, st = K.eth_address_batch(keys[fmt][i], None, fmt, "eip55")
            assert np.array_equal(a[0], eip[i]) and st[0] == K.MATCH
        a, st = K.eth_address_batch(keys[fmt][list(PLANTED)], None, fmt, "record64")
        assert not a.any() and (st == K.INVALID).all()
    rec64 = np.concatenate([np.zeros((N, 44), np.uint8), raw], axis=1)
    return dict(keys=keys, raw=raw, status=status, address={"raw20": raw, "record64": rec64, "eip55": eip})


def _device(eng, pk, expect, pk_format, addr_format, stream=None, address=True, status=True, sync=True):
    """one device-form call into tensors pre-filled with FILL"""
    import torch
    dev = torch.device(f"cuda:{eng.device_id}")
    n = len(pk)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    o = dict(address=torch.full((n, K.ADDR_WIDTH[addr_format]), FILL, dtype=torch.uint8, device=dev), status=torch.full((n,), FILL, dtype=torch.uint8, device=dev))
    s = stream or torch.cuda.Stream(dev)                                 # (never torch's default stream: its handle is NULL, which the library reads as "the context's own stream")
    d = dict(pk=t(pk), expect=t(expect))
    s.wait_stream(torch.cuda.current_stream(dev))
    eng.eth_address_batch_device(n, d["pk"], d["expect"], o["address"] if address else None, o["status"] if status else None, pk_format=pk_format, addr_format=addr_format, stream=s)
    if not sync:
        return o, d
    s.synchronize()
    return {k: x.cpu().numpy() for k, x in o.items()}


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_every_format_at_sizes_around_the_block(eng, ref, n):
    for pf in PKF:
        for af in ADF:
            address, status = eng.eth_address_batch(ref["keys"][pf][:n], None, pf, af)
            assert np.array_equal(address, ref["address"][af][:n]), (pf, af, "host form")
            assert np.array_equal(status, ref["status"][:n]), (pf, af, "host form")
            got = _device(eng, ref["keys"][pf][:n], None, pf, af)
            assert np.array_equal(got["address"], ref["address"][af][:n]) and np.array_equal(got["status"], ref["status"][:n]), (pf, af, "device form")


def test_public_vectors_through_the_c_abi(eng):
    want = [v["address"] for v in KATS["addresses"]]
    raw = np.frombuffer(b"".join(bytes.fromhex(a[2:]) for a in want), np.uint8).reshape(3, 20)
    for pf, key in (("affine64", "pk"), ("sec1", "pk_sec1")):
        keys = np.frombuffer(b"".join(bytes.fromhex(v[key]) for v in KATS["addresses"]), np.uint8)
        address, status = eng.eth_address_batch(keys, raw, pf, "eip55")
        assert [a.tobytes().decode() for a in address] == want and list(status) == [K.MATCH] * 3
        address, status = eng.eth_address_batch(keys, raw[::-1], pf, "raw20")
        assert np.array_equal(address, raw) and list(status) == [K.MISMATCH, K.MATCH, K.MISMATCH]
        got = _device(eng, keys.reshape(3, -1).copy(), raw.copy(), pf, "record64")
        assert np.array_equal(got["address"][:, 44:], raw) and not got["address"][:, :44].any() and list(got["status"]) == [K.MATCH] * 3


def test_invalid_keys_at_the_first_the_last_and_mid_wavefront_positions(eng, ref):
    for pf in PKF:
        for af in ADF:
            got = _device(eng, ref["keys"][pf], ref["raw"], pf, af)      # expect given: the zero address here -- status 3 whatever expect holds
            for pos in PLANTED:
                assert got["status"][pos] == K.INVALID and not got["address"][pos].any(), (pf, af, pos)
                for nb in (pos - 1, pos + 1):
                    if 0 <= nb < N and nb not in PLANTED:
                        assert got["status"][nb] == K.MATCH and np.array_equal(got["address"][nb], ref["address"][af][nb]), (pf, af, nb)
            assert np.array_equal(got["address"], ref["address"][af]) and np.array_equal(got["status"], ref["status"])


def test_expect_matching_wrong_status_only_and_address_only(eng, ref):
    rng = np.random.default_rng(3)
    expect = ref["raw"].copy()
    expect[list(PLANTED)] = rng.integers(1, 256, (len(PLANTED), 20), dtype=np.uint8)     # an invalid key is status 3 whatever expect holds
    wrong = np.array(sorted(set(rng.integers(0, N, 120).tolist()) - set(PLANTED)))
    for k, i in enumerate(wrong):
        expect[i, k % 20] ^= np.uint8(1 << (k % 8))                    # one bit, every byte position in turn
    want = ref["status"].copy()
    want[wrong] = K.MISMATCH
    for pf in PKF:
        address, status = eng.eth_address_batch(ref["keys"][pf], expect, pf, "raw20")
        assert np.array_equal(status, want) and np.array_equal(address, ref["raw"])
        got = _device(eng, ref["keys"][pf], expect, pf, "eip55", address=False)          # status only
        assert np.array_equal(got["status"], want) and (got["address"] == FILL).all()
        got = _device(eng, ref["keys"][pf], expect, pf, "eip55", status=False)           # address only
        assert np.array_equal(got["address"], ref["address"]["eip55"]) and (got["status"] == FILL).all()
    with pytest.raises(Exception, match="no output array"):
        _device(eng, ref["keys"]["affine64"], expect, "affine64", "raw20", address=False, status=False)


def test_host_form_in_chunks_of_300(ref):
    import zk_nullifier_sig_amd as plume
    e = plume.Engine(0)
    try:
        e.set_chunk(300)
        for pf, af in (("affine64", "eip55"), ("sec1", "raw20"), ("affine64", "record64")):
            address, status = e.eth_address_batch(ref["keys"][pf], ref["raw"], pf, af)
            assert np.array_equal(address, ref["address"][af]) and np.array_equal(status, ref["status"]), (pf, af)
    finally:
        e.close()


def test_two_shards_on_one_device(ref):
    import zk_nullifier_sig_amd as plume
    m = plume.Engine([0, 0])
    try:
        assert m.num_shards() == 2
        for pf, af, n in (("affine64", "raw20", N), ("sec1", "eip55", 257), ("affine64", "record64", 1)):
            address, status = m.eth_address_batch(ref["keys"][pf][:n], ref["raw"][:n], pf, af)
            assert np.array_equal(address, ref["address"][af][:n]) and np.array_equal(status, ref["status"][:n]), (pf, af, n)
        with pytest.raises(plume.PlumeHipError, match="single-device"):
            _device(m, ref["keys"]["affine64"][:4], None, "affine64", "raw20")
    finally:
        m.close()


def test_two_calls_back_to_back_on_a_caller_stream(eng, ref):
    import torch
    s = torch.cuda.Stream(torch.device(f"cuda:{eng.device_id}"))
    o1, keep1 = _device(eng, ref["keys"]["affine64"], ref["raw"], "affine64", "eip55", stream=s, sync=False)
    o2, keep2 = _device(eng, ref["keys"]["sec1"][:257], None, "sec1", "record64", stream=s, sync=False)
    s.synchronize()
    assert np.array_equal(o1["address"].cpu().numpy(), ref["address"]["eip55"]) and np.array_equal(o1["status"].cpu().numpy(), ref["status"])
    assert np.array_equal(o2["address"].cpu().numpy(), ref["address"]["record64"][:257]) and np.array_equal(o2["status"].cpu().numpy(), ref["status"][:257])
    del keep1, keep2


@pytest.mark.parametrize("lead", [1, 3, 8, 13])
def test_arrays_at_odd_byte_offsets_inside_a_larger_tensor(eng, ref, lead):
    import torch
    dev = torch.device(f"cuda:{eng.device_id}")
    n = 300
    s = torch.cuda.Stream(dev)
    for pf in PKF:
        for af in ADF:
            P, W = K.PK_WIDTH[pf], K.ADDR_WIDTH[af]

            def inside(data, width):
                """`lead` bytes behind the start of a 256-byte aligned allocation, 32 guard bytes in front and behind"""
                big = torch.full((32 + lead + width * n + 32 + 16,), FILL, dtype=torch.uint8, device=dev)
                view = big[32 + lead:32 + lead + width * n]
                if data is not None:
                    view.copy_(torch.from_numpy(np.ascontiguousarray(data).reshape(-1)).to(dev))
                return big, view
            bpk, vpk = inside(ref["keys"][pf][:n], P)
            bex, vex = inside(ref["raw"][:n], 20)
            bad, vad = inside(None, W)
            bst, vst = inside(None, 1)
            assert vad.data_ptr() % 16 == (32 + lead) % 16
            s.wait_stream(torch.cuda.current_stream(dev))
            eng.eth_address_batch_device(n, vpk, vex, vad, vst, pk_format=pf, addr_format=af, stream=s)
            s.synchronize()
            assert np.array_equal(vad.cpu().numpy().reshape(n, W), ref["address"][af][:n]) and np.array_equal(vst.cpu().numpy(), ref["status"][:n]), (pf, af)
            for big, width in ((bad, W), (bst, 1)):
                b = big.cpu().numpy()
                assert (b[:32 + lead] == FILL).all() and (b[32 + lead + width * n:] == FILL).all(), (pf, af, "guard bytes")
            assert np.array_equal(vpk.cpu().numpy().reshape(n, P), ref["keys"][pf][:n]) and np.array_equal(vex.cpu().numpy().reshape(n, 20), ref["raw"][:n])
