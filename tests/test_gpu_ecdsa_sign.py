"""plume_eth_message_hash_batch and plume_ecdsa_sign_batch on the MI355X (include/plume_hip.h; kernels k_eth_message_hash in csrc/plume_eth_kernels.hip and
csrc/plume_ecdsa_sign_kernels.hip, lane bodies in csrc/plume_keccak.h and csrc/plume_ecdsa_sign.h): byte for byte against the restatement of tests/_ecdsa_sign.py and the
vectors of tests/golden/ecdsa_sign_kats.json (pinned to the published RFC 6979 vectors and to OpenSSL's verifier by tests/golden/make_ecdsa_sign_kats.py), and round trips
through the library's own verifier side: plume_ecdsa_recover_batch, plume_eth_address_batch.  Every comparison is bit-exact and leaves no item out.  The block is 256
lanes and a wavefront 64; the batched inversion takes 8 points per lane."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import _ecdsa as E
from tests import _ecdsa_sign as S

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
FILL = 0xAA
NBIG = 2048
SIZES = (1, 255, 256, 257)
SIGN_STAGES = ["ecdsa_sign_nonce", "ecdsa_sign_gmul", "to_affine", "ecdsa_sign_finalize"]
RECOVER_STAGES = ["ecdsa_prepare", "tables", "ecdsa_mul", "to_affine", "ecdsa_finalize"]


@pytest.fixture(scope="module")
def eng():
    import zk_nullifier_sig_amd as plume
    e = plume.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def kats():
    return S.load_kats()


# ------------------------------------------------------------------------------------------------ the message hash
@pytest.fixture(scope="module")
def ragged(kats):
    """the fixture's messages of both modes, ten times over, with a filler message in front of every repetition whose length moves the repetition's first byte to the next
    residue mod 8, so that every message starts on every residue: (messages, {mode: digests}), the restatement's answers computed once"""
    base = [bytes.fromhex(e["msg"]) for e in kats["hash"]]
    msgs, total, first = [], 0, []
    for rep in range(10):
        filler = bytes([rep]) * ((rep - total - 1) % 8 + 1)                   # 1 .. 8 bytes: the repetition then starts at rep mod 8
        msgs += [filler] + base
        first.append((total + len(filler)) % 8)
        total += len(filler) + sum(len(m) for m in base)
    assert first[:8] == list(range(8)) and len(msgs) >= max(SIZES)
    buf = b"".join(msgs)
    off = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint64)
    want = {mode: S.message_hash_batch(buf, off, mode) for mode in (S.KECCAK256, S.EIP191)}
    for e in kats["hash"]:                                                   # the committed digests are among them
        assert bytes.fromhex(e["digest"]) == want[e["mode"]][1 + base.index(bytes.fromhex(e["msg"]))].tobytes()
    return msgs, want


def _pack(msgs):
    from zk_nullifier_sig_amd.capi import pack_messages
    return pack_messages(msgs)


@pytest.mark.parametrize("mode", [S.KECCAK256, S.EIP191])
def test_message_hash_over_the_ragged_fixture(eng, ragged, mode):
    msgs, want = ragged
    buf, off = _pack(msgs)
    assert np.array_equal(eng.eth_message_hash_batch(buf, off, mode), want[mode])
    assert np.array_equal(eng.eth_message_hash_batch(buf, off, "eip191" if mode else "keccak256"), want[mode])
    for n in SIZES:                                                          # the last wavefront is partial
        assert np.array_equal(eng.eth_message_hash_batch(buf, off[:n + 1], mode), want[mode][:n]), n


def test_message_hash_device_form_at_an_odd_byte_offset(eng, ragged):
    import torch
    msgs, want = ragged
    buf, off = _pack(msgs)
    n, nbytes = len(msgs), int(off[-1])
    dev = torch.device(f"cuda:{eng.device_id}")
    for shift_in, shift_out in ((1, 3), (7, 0), (0, 5)):
        for mode in (S.KECCAK256, S.EIP191):
            dm = torch.full((nbytes + 64,), FILL, dtype=torch.uint8, device=dev)
            dm[shift_in:shift_in + nbytes] = torch.from_numpy(buf[:nbytes]).to(dev)
            out = torch.full((32 * n + 64,), FILL, dtype=torch.uint8, device=dev)
            doff = torch.from_numpy(off.view(np.int64)).to(dev)
            st = torch.cuda.Stream(dev)
            st.wait_stream(torch.cuda.current_stream(dev))
            eng.eth_message_hash_batch_device(n, dm[shift_in:], doff, nbytes, out[shift_out:], mode=mode, stream=st)
            st.synchronize()
            got = out.cpu().numpy()
            assert np.array_equal(got[shift_out:shift_out + 32 * n].reshape(n, 32), want[mode]), (shift_in, shift_out, mode)
            assert (got[:shift_out] == FILL).all() and (got[shift_out + 32 * n:] == FILL).all()
    # rejected offsets hash the empty message: item 3 (seven bytes) runs backwards -- its neighbour then starts one byte early -- and the last item reaches past msgs_bytes
    assert len(msgs[3]) == 7 and len(msgs[n - 1]) > 0
    bad = off.copy()
    bad[4] = bad[3] - 1
    dm = torch.from_numpy(buf[:nbytes]).to(dev)
    out = torch.full((n, 32), FILL, dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    eng.eth_message_hash_batch_device(n, dm, torch.from_numpy(bad.view(np.int64)).to(dev), nbytes - 1, out, mode="eip191", stream=st)
    st.synchronize()
    got = out.cpu().numpy()
    empty = np.frombuffer(S.message_hash(b"", S.EIP191), np.uint8)
    assert np.array_equal(got[3], empty) and np.array_equal(got[n - 1], empty)
    assert np.array_equal(got[:3], want[S.EIP191][:3]) and np.array_equal(got[5:n - 1], want[S.EIP191][5:n - 1])
    assert np.array_equal(got[4], np.frombuffer(S.message_hash(bytes(buf[int(bad[4]):int(bad[5])]), S.EIP191), np.uint8))


# ------------------------------------------------------------------------------------------------ signing
def _kat_arrays(kats, hedged):
    es = [e for e in kats["sign"] if (e["aux"] is not None) == hedged]
    arr = lambda key: np.frombuffer(b"".join(bytes.fromhex(e[key]) for e in es), np.uint8).reshape(len(es), 32).copy()  # noqa: E731
    return arr("sk"), arr("hash"), (arr("aux") if hedged else None), es


@pytest.fixture(scope="module")
def big(kats):
    """NBIG seeded items with the fixture's plain items planted from 960 on (across the wavefront boundary at 1024) and the three published vectors at 0, 63 and 64:
    (sk, hash, aux) and the restatement's answers without and with aux, computed once"""
    sk, h, aux = S.seeded(NBIG, 99)
    ksk, kh, _, _ = _kat_arrays(kats, False)
    sk[960:960 + len(ksk)], h[960:960 + len(kh)] = ksk, kh
    for pos, p in zip((0, 63, 64), kats["public"]):
        sk[pos], h[pos] = np.frombuffer(bytes.fromhex(p["sk"]), np.uint8), np.frombuffer(bytes.fromhex(p["hash"]), np.uint8)
    plain, hedged = S.sign_batch(h, sk, None, 0), S.sign_batch(h, sk, aux, 0)
    in_range = np.array([1 <= int.from_bytes(sk[i].tobytes(), "big") < E.N for i in range(NBIG)])
    for res in (plain, hedged):                                              # no valid item is left out, for these seeds
        assert np.array_equal(res[3] == S.OK, in_range) and (res[3][~in_range] == S.BAD_SCALAR).all()
    assert int((~in_range).sum()) == 4                                      # sk = 0, n, n + 1 and 2^256 - 1 of the planted fixture
    for pos, p in zip((0, 63, 64), kats["public"]):
        assert plain[0][pos].tobytes().hex() == p["r"] and plain[1][pos].tobytes().hex() == p["s"] and plain[2][pos] == p["v"]
    return dict(sk=sk, hash=h, aux=aux, plain=plain, hedged=hedged, in_range=in_range)


def _same(got, want, v27, what):
    r, s, v, st = want
    wv = np.where(st == S.OK, v + (27 if v27 else 0), 0).astype(np.uint8)
    assert np.array_equal(got[3], st), (what, "status")
    assert np.array_equal(got[0], r) and np.array_equal(got[1], s) and np.array_equal(got[2], wv), what


def _device(eng, n, h, sk, aux, v27=False, stream=None, shift=0):
    """one device-form call on the first n items into tensors pre-filled with FILL, every array `shift` bytes into its tensor"""
    import torch
    dev = torch.device(f"cuda:{eng.device_id}")

    def t(a):
        if a is None:
            return None
        x = torch.full((a[:n].size + 16,), FILL, dtype=torch.uint8, device=dev)
        x[shift:shift + a[:n].size] = torch.from_numpy(np.ascontiguousarray(a[:n]).reshape(-1)).to(dev)
        return x[shift:]
    o = [torch.full((w * n + 32,), FILL, dtype=torch.uint8, device=dev) for w in (32, 32, 1, 1)]
    st = stream or torch.cuda.Stream(dev)                                    # (never torch's default stream: its handle is NULL, which the library reads as "the context's own stream")
    dh, dsk, daux = t(h), t(sk), t(aux)
    st.wait_stream(torch.cuda.current_stream(dev))
    eng.ecdsa_sign_batch_device(n, dh, dsk, daux, o[0][shift:], o[1][shift:], o[2][shift:], o[3][shift:], v27=v27, stream=st)
    st.synchronize()
    out = []
    for x, w in zip(o, (32, 32, 1, 1)):
        g = x.cpu().numpy()
        assert (g[:shift] == FILL).all() and (g[shift + w * n:] == FILL).all()
        out.append(g[shift:shift + w * n].reshape((n, 32) if w == 32 else (n,)))
    return out


@pytest.mark.parametrize("hedged", [False, True])
def test_the_fixture_byte_exact_at_sizes_around_the_block(eng, kats, hedged):
    sk, h, aux, es = _kat_arrays(kats, hedged)
    want_st = np.array([e["status"] for e in es], np.uint8)
    r, s, v, st = eng.ecdsa_sign_batch(h, sk, aux)
    assert np.array_equal(st, want_st)
    assert r.tobytes().hex() == "".join(e["r"] for e in es) and s.tobytes().hex() == "".join(e["s"] for e in es) and list(v) == [e["v"] for e in es]
    # the same items tiled to the sizes around the block, host form and device form, both encodings of v
    reps = -(-257 // len(es))
    tsk, th = np.tile(sk, (reps, 1)), np.tile(h, (reps, 1))
    taux = None if aux is None else np.tile(aux, (reps, 1))
    want = tuple(np.tile(a, (reps, 1)) if a.ndim == 2 else np.tile(a, reps) for a in (r, s, v, st))
    for n, v27 in zip(SIZES, (False, True, False, True)):
        w = tuple(a[:n] for a in want)
        _same(eng.ecdsa_sign_batch(th[:n], tsk[:n], None if taux is None else taux[:n], v27=v27), w, v27, (n, "host form"))
        _same(_device(eng, n, th, tsk, taux, v27=v27, shift=n % 4), w, v27, (n, "device form"))
        _same(_device(eng, n, th, tsk, taux, v27=not v27, shift=0), w, not v27, (n, "device form, aligned"))


def test_2048_items_identical_at_the_three_uniform_levels(eng, big):
    b = big
    level0 = eng.sign_uniform()
    try:
        for level in (0, 1, 2):
            eng.set_sign_uniform(level)
            _same(eng.ecdsa_sign_batch(b["hash"], b["sk"], None), b["plain"], False, ("plain", level))
            _same(_device(eng, NBIG, b["hash"], b["sk"], b["aux"], v27=True), b["hedged"], True, ("hedged, device form", level))
    finally:
        eng.set_sign_uniform(level0)


def test_round_trip_through_recover_and_the_signers_own_pk(eng, big):
    from zk_nullifier_sig_amd.capi import pack_messages
    b = big
    ok = b["in_range"]
    r, s, v, st = eng.ecdsa_sign_batch(b["hash"], b["sk"], b["aux"], v27=True)
    assert np.array_equal(st == S.OK, ok)
    pk, address, status = eng.ecdsa_recover_batch(b["hash"], r, s, v, low_s=True)
    assert (status[ok] == E.MATCH).all() and (status[~ok] == E.INVALID).all()
    # the pk the PLUME signer reports for the same sk
    msgs, off = pack_messages([b"m"] * NBIG)
    sk_ok = b["sk"].copy()
    sk_ok[~ok] = b["sk"][ok][0]
    own = eng.sign_batch(2, msgs, off, sk_ok, sk_ok)["pk"].reshape(NBIG, 64)
    assert np.array_equal(pk[ok], own[ok])
    want_addr, _ = eng.eth_address_batch(own)
    assert np.array_equal(address[ok], want_addr[ok])


def test_personal_sign_and_personal_recover(eng, kats):
    import zk_nullifier_sig_amd as plume
    for e in kats["sign"][:3] + [x for x in kats["sign"] if x["name"] == "sk = 1"]:
        sk32 = bytes.fromhex(e["sk"])
        for msg in (b"", b"hello world", S.message_of(300, 5)):
            sig = plume.personal_sign(sk32, msg, engine=eng)
            assert sig == S.personal_sign(sk32, msg) and sig[64] in (27, 28)
            pk, addr = plume.personal_recover(msg, sig, engine=eng)
            own_addr, own_st = eng.eth_address_batch(np.frombuffer(E.pk_record(E.mul(int(e["sk"], 16)), "affine64"), np.uint8))
            assert addr == own_addr[0].tobytes() and own_st[0] == 1 and pk.to_bytes64() == E.pk_record(E.mul(int(e["sk"], 16)), "affine64")
            hedged = plume.personal_sign(plume.SecretKey.from_bytes(sk32), msg, aux=S.FIXED_AUX, engine=eng)
            assert hedged == S.personal_sign(sk32, msg, S.FIXED_AUX) and hedged != sig and plume.personal_recover(msg, hedged, engine=eng)[1] == addr
    r, s, v = plume.ecdsa_sign(bytes.fromhex(kats["public"][0]["sk"]), bytes.fromhex(kats["public"][0]["hash"]), engine=eng)
    assert (r.hex(), s.hex(), v) == (kats["public"][0]["r"], kats["public"][0]["s"], kats["public"][0]["v"])
    with pytest.raises(plume.SignatureError):
        plume.ecdsa_sign(bytes(32), bytes(32), engine=eng)


# ------------------------------------------------------------------------------------------------ the self-check
def test_selfcheck_outputs_stage_list_and_environment(eng, kats, big):
    sk, h, aux, es = _kat_arrays(kats, True)
    want = eng.ecdsa_sign_batch(h, sk, aux, v27=True)
    assert eng.sign_selfcheck() == 0
    eng.set_stage_timing(True)
    try:
        _device(eng, len(es), h, sk, aux)
        assert [k for k, _ in eng.last_stage_times()] == SIGN_STAGES
        eng.set_sign_selfcheck(1)
        got = eng.ecdsa_sign_batch(h, sk, aux, v27=True)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        assert S.BAD_SCALAR in got[3] and S.SELFCHECK_FAILED not in got[3]
        _same(_device(eng, NBIG, big["hash"], big["sk"], None, shift=1), big["plain"], False, "self-check, 2048, device form")
        assert [k for k, _ in eng.last_stage_times()] == SIGN_STAGES + RECOVER_STAGES + ["ecdsa_sign_release"]
        for level in (0, 2):
            eng.set_sign_uniform(level)
            _same(_device(eng, 257, big["hash"], big["sk"], big["aux"], v27=True), tuple(a[:257] for a in big["hedged"]), True, ("self-check", level))
    finally:
        eng.set_sign_uniform(1)
        eng.set_stage_timing(False)
        eng.set_sign_selfcheck(0)
    code = ("import numpy as np, zk_nullifier_sig_amd as p; e = p.Engine(0); print('mode', e.sign_selfcheck()); e.set_stage_timing(True);"
            "r = e.ecdsa_sign_batch(np.full(32, 7, np.uint8), np.full(32, 9, np.uint8)); print('status', int(r[3][0]), r[0].tobytes().hex()); e.close()")
    outs = {}
    for val in ("1", "0"):
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, PLUME_SIGN_SELFCHECK=val), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and f"mode {val}" in r.stdout and "status 0 " in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
        outs[val] = r.stdout.split("status 0 ")[1].split()[0]
    assert outs["1"] == outs["0"] == E.b32(S.sign(bytes([9]) * 32, bytes([7]) * 32)[0]).hex()


# ------------------------------------------------------------------------------------------------ routing
def test_sub_batches_chunks_shards_and_arguments(eng, big):
    import zk_nullifier_sig_amd as plume
    from zk_nullifier_sig_amd import capi
    b = big
    try:
        eng.set_sub_batches(2)
        _same(_device(eng, NBIG, b["hash"], b["sk"], b["aux"]), b["hedged"], False, "two sub-batches")
        eng.set_chunk(512)
        _same(eng.ecdsa_sign_batch(b["hash"], b["sk"], None, v27=True), b["plain"], True, "chunks of 512")
        buf, off = _pack([S.message_of(L % 300, L) for L in range(NBIG)])
        want = S.message_hash_batch(buf, off, S.EIP191)
        assert np.array_equal(eng.eth_message_hash_batch(buf, off, "eip191"), want)
        with pytest.raises(capi.PlumeHipError):
            _device(eng, NBIG, b["hash"], b["sk"], None)                     # the device form takes at most one chunk
    finally:
        eng.set_chunk(1 << 20)
        eng.set_sub_batches(1)
    multi = plume.Engine([eng.device_id, eng.device_id])
    try:
        _same(multi.ecdsa_sign_batch(b["hash"], b["sk"], b["aux"]), b["hedged"], False, "plume_init_multi([d, d])")
        assert np.array_equal(multi.eth_message_hash_batch(buf, off, "eip191"), want)
        multi.set_sign_selfcheck(1)
        _same(multi.ecdsa_sign_batch(b["hash"][:300], b["sk"][:300], None), tuple(a[:300] for a in b["plain"]), False, "plume_init_multi([d, d]), self-check")
    finally:
        multi.close()
    r, s, v, st = eng.ecdsa_sign_batch(np.zeros((0, 32), np.uint8), np.zeros((0, 32), np.uint8))
    assert r.shape == (0, 32) and st.shape == (0,)
    assert eng.eth_message_hash_batch(np.zeros(16, np.uint8), np.zeros(1, np.uint64)).shape == (0, 32)
    for flags in (2, 3, 0x100):
        with pytest.raises(capi.PlumeHipError):
            eng.ecdsa_sign_batch(b["hash"][:4], b["sk"][:4], flags=flags)
    for mode in (2, -1):
        with pytest.raises(capi.PlumeHipError):
            eng.eth_message_hash_batch(buf, off[:5], mode)


def test_cpp_facade(tmp_path, kats):
    import zk_nullifier_sig_amd as plume
    vectors = tmp_path / "vectors.txt"
    vectors.write_text("".join(f'{p["sk"]} {p["hash"]} {p["r"]} {p["s"]} {p["v"]}\n' for p in kats["public"]))
    exe = tmp_path / "ecdsa_sign_test"
    libdir = plume.library_path().parent
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"), str(ROOT / "tests" / "abi_cpp" / "ecdsa_sign_test.cpp"), "-L", str(libdir),
                    "-lplume_hip", f"-Wl,-rpath,{libdir}", "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe), str(vectors)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ecdsa_sign_test ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
