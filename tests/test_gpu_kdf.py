"""plume_pbkdf2_sha512_batch on the MI355X (include/plume_hip.h; kernels in csrc/plume_kdf_kernels.hip, lane bodies in csrc/plume_kdf.h and csrc/plume_sha512.h): byte
for byte against the restatement of tests/_kdf.py (hashlib.pbkdf2_hmac plus the status and zeroing rules).  The kernels run 256-lane workgroups of 64-lane wavefronts:
n = 1, 63, 64, 65 (a partial wavefront, a whole one, one lane over), 257 and 1025 (one lane over one and over four workgroups).  Every wavefront mixes the password
lengths 0, 1, 111, 112, 128, 129, 239, 240 and 300 (tests/_kdf.PLANTED): raw and hashed keys, one to three blocks of key hashing.  Iteration counts 1, 3 and 257 (no
slice, one short slice, one whole slice) for the shape sweep, 2048 at n = 65 and 1025; both flags, salts of 0 (NULL), 8, 100 and 256 bytes -- one, two and three blocks
of inner message.  Every comparison is bit-exact and leaves no item out."""
import json
from pathlib import Path

import numpy as np
import pytest

from tests import _kdf as D

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SALT_LEN = {0: 8, D.BIP39: 100, D.SHARED_SALT: 256, D.BIP39 | D.SHARED_SALT: 0}


@pytest.fixture(scope="module")
def eng():
    import zk_nullifier_sig_amd as plume
    e = plume.Engine(0)
    yield e
    e.close()


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _same(got, want, what):
    for g, w, name in zip(got, want, ("out", "status")):
        g = _np(g)
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))[:8])


def _call(eng, case, iterations, flags, device, dklen=64):
    buf, off, salt, out, status = case
    s = None if salt.shape[1] == 0 else salt[0].tobytes() if flags & D.SHARED_SALT else salt
    return eng.pbkdf2_sha512_batch((buf, off), s, iterations, dklen, bip39=bool(flags & D.BIP39), device=device)


@pytest.mark.parametrize("iterations", [1, 3, 257])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025])
def test_host_and_device_forms_against_the_restatement(eng, n, iterations):
    for flags, salt_len in SALT_LEN.items():
        case = D.planted_case(n, iterations, flags, salt_len)
        assert not case[4].any() and (n < 9 or len({int(b - a) for a, b in zip(case[1][:64], case[1][1:65])}) == min(n, len(D.PLANTED)))
        _same(_call(eng, case, iterations, flags, False), case[3:], (n, iterations, flags, "host form"))
        eng.set_stage_timing(True)
        try:
            _same(_call(eng, case, iterations, flags, True), case[3:], (n, iterations, flags, "device form"))
            assert [k for k, _ in eng.last_stage_times()] == D.stage_list(iterations)
        finally:
            eng.set_stage_timing(False)


@pytest.mark.parametrize("n,device", [(65, False), (1025, True)])
def test_2048_iterations(eng, n, device):
    flags = D.BIP39 | D.SHARED_SALT
    case = D.planted_case(n, 2048, flags, 6)
    eng.set_stage_timing(device)
    try:
        _same(_call(eng, case, 2048, flags, device), case[3:], (n, "2048 iterations"))
        if device:
            assert [k for k, _ in eng.last_stage_times()] == D.stage_list(2048) == ["kdf_key"] + ["kdf_iter"] * 8 + ["kdf_finish"]
    finally:
        eng.set_stage_timing(False)


@pytest.mark.parametrize("iterations,slices", [(1, 0), (2, 1), (256, 1), (257, 1), (258, 2)])
def test_stage_list(eng, iterations, slices):
    case = D.planted_case(9, iterations, D.SHARED_SALT, 4, 32)
    eng.set_stage_timing(True)
    try:
        _same(_call(eng, case, iterations, D.SHARED_SALT, True, 32), case[3:], iterations)
        assert [k for k, _ in eng.last_stage_times()] == ["kdf_key"] + ["kdf_iter"] * slices + ["kdf_finish"]
    finally:
        eng.set_stage_timing(False)


@pytest.mark.parametrize("dklen", [1, 31, 32, 63, 64])
def test_output_lengths(eng, dklen):
    case = D.planted_case(70, 2, 0, 17, dklen)
    _same(_call(eng, case, 2, 0, False, dklen), case[3:], (dklen, "host form"))
    _same(_call(eng, case, 2, 0, True, dklen), case[3:], (dklen, "device form"))


def _at(torch, dev, arr, shift, fill=0xAA):
    """the bytes of arr in device memory `shift` bytes behind a 16-byte boundary, between guard bytes; returns (buffer, view)"""
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    buf = torch.full((32 + 16 + raw.size + 32,), fill, dtype=torch.uint8, device=dev)
    view = buf[32 + shift:32 + shift + raw.size]
    view.copy_(torch.from_numpy(raw.copy()))
    return buf, view


@pytest.mark.parametrize("shift", [0, 1, 3])
def test_device_form_refuses_unsound_offsets_among_good_lanes(eng, shift):
    """items whose offsets decrease or reach past pw_bytes get status 128 and zero records, their neighbours are derived; every byte array `shift` bytes off its
    alignment between guard bytes that stay as they were, the password buffer ending with pw_bytes"""
    import torch
    dev = torch.device("cuda", eng.device_id)
    n, iterations, dklen, salt_len = 257, 3, 48, 12
    buf, off = D.planted_passwords(n, 128 + shift)
    off = off.copy()
    bad = [3, 64, 65, 130, 200, 256]
    off[4] = off[3] - 1                                     # item 3 runs backwards
    off[65] = len(buf) + 1                                  # item 64 reaches past the buffer, item 65 runs backwards from there
    off[131] = 2**63                                        # item 130 far past it; item 131 backwards
    bad.append(131)
    off[201] = off[200] - 1
    off[257] = len(buf) + 2**32                             # the last item: its end past the buffer by more than 32 bits hold
    salt = np.random.default_rng(9).integers(0, 256, (n, salt_len), dtype=np.uint8)
    want_out, want_st = D.pbkdf2_batch(buf, off, len(buf), salt, salt_len, iterations, dklen, D.BIP39)
    assert sorted(bad) == list(np.flatnonzero(want_st)) and (want_st[sorted(bad)] == D.BAD_INPUT).all() and not want_out[sorted(bad)].any()
    assert want_out[4].any() and want_out[63].any() and want_out[66].any() and want_out[255].any()
    pw_buf, pw = _at(torch, dev, buf, shift)
    salt_buf, salt_d = _at(torch, dev, salt, shift)
    out_buf, out = _at(torch, dev, np.zeros((n, dklen), np.uint8), shift)
    st_buf, st = _at(torch, dev, np.zeros(n, np.uint8), shift)
    out.fill_(0x55); st.fill_(0x55)
    off_d = torch.from_numpy(off.view(np.int64)).to(dev)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    eng.pbkdf2_sha512_batch_device(n, pw, off_d, len(buf), salt_d, salt_len, iterations, dklen, out, st, flags=D.BIP39, stream=stream)
    stream.synchronize()
    _same((out.reshape(n, dklen), st), (want_out, want_st), shift)
    for b, lo, size in ((out_buf, 32 + shift, n * dklen), (st_buf, 32 + shift, n), (pw_buf, 32 + shift, len(buf)), (salt_buf, 32 + shift, n * salt_len)):
        h = b.cpu().numpy()
        assert (h[:lo] == 0xAA).all() and (h[lo + size:] == 0xAA).all()
    assert np.array_equal(pw.cpu().numpy(), buf) and np.array_equal(salt_d.cpu().numpy().reshape(n, salt_len), salt)


def test_known_answers(eng):
    kats = json.loads((ROOT / "tests" / "golden" / "kdf_kats.json").read_text())["kats"]
    hd = json.loads((ROOT / "tests" / "golden" / "hd_kats.json").read_text())["known"]["hardhat"]
    by_name = {k["name"]: k for k in kats}
    assert by_name["bip39_trezor_vector_1"]["out"] == D.TREZOR_SEED and by_name["hardhat"]["out"] == hd["seed"]
    assert by_name["password_salt_1"]["out"] == D.RFC_STYLE[1] and by_name["password_salt_2"]["out"] == D.RFC_STYLE[2]
    for k in kats:
        for device in (False, True):
            out, status = eng.pbkdf2_sha512_batch([k["password"].encode()], k["salt"].encode(), k["iterations"], 64, bip39=k["bip39"], device=device)
            assert _np(out)[0].tobytes().hex() == k["out"] and int(_np(status)[0]) == 0, (k["name"], device)
    seed, status = eng.bip39_seed_batch([D.TREZOR_MNEMONIC, D.HARDHAT_MNEMONIC.encode()], "TREZOR")
    assert seed[0].tobytes().hex() == D.TREZOR_SEED and not status.any()
    assert eng.bip39_seed_batch([D.HARDHAT_MNEMONIC])[0][0].tobytes().hex() == hd["seed"]


def test_argument_errors_reach_python(eng):
    import zk_nullifier_sig_amd as plume
    for kw in (dict(iterations=0), dict(iterations=D.MAX_ITERATIONS + 1), dict(dklen=65), dict(salt=bytes(257))):
        with pytest.raises(plume.PlumeHipError):
            eng.pbkdf2_sha512_batch([b"pw"], **kw)
    off = np.array([0, 5, 3], np.uint64)                    # the host form refuses decreasing offsets as a whole
    with pytest.raises(plume.PlumeHipError, match="pw_off"):
        eng.pbkdf2_sha512_batch((np.zeros(8, np.uint8), off), b"s", 2)
    out, status = eng.pbkdf2_sha512_batch([], b"s", 2)
    assert out.shape == (0, 64) and status.shape == (0,)
