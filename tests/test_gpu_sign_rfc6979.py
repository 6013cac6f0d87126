"""The derived-nonce signer on the MI355X (include/plume_hip.h, plume_sign_batch_rfc6979*; kernel in csrc/plume_nonce_kernels.hip): every output byte-identical to
plume_sign_batch given the RFC 6979 nonces of the Python oracle (tests/_rfc6979.py), over V1 / V2, pk derived / supplied, aux absent / given, host form from pageable and
page-locked arrays and the device form on a torch stream, at uniform levels 0, 1 and 2; a 2^20-item call (repeatable, the same on a two-shard context, a sampled oracle
check, every signature verifies, no r_point repeats); domain separation; rejected offsets; the C++ façade."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import _rfc6979 as R

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
KEYS = ["pk", "nullifier", "c", "s", "r_point", "hashed_to_curve_r", "status"]


@pytest.fixture(scope="module")
def eng():
    import zk_nullifier_sig_amd as plume
    return plume.default_engine()


def _inputs(n, seed, maxlen=300):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, maxlen + 1, size=n)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    msgs = rng.integers(0, 256, size=int(off[-1]) + 16, dtype=np.uint8)
    sk = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    sk[:, 0] &= 0x7F                                               # < n
    sk[:, 31] |= 1                                                 # != 0
    aux = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    return msgs, off, sk, aux


def _oracle_r(version, msgs, off, sk, pk_in, aux):
    return np.frombuffer(R.plume_nonces(version, msgs, off, sk, pk_in, aux), dtype=np.uint8).reshape(-1, 32)


def _same(a, b, what):
    for k in KEYS:
        assert np.array_equal(np.asarray(a[k]).reshape(-1), np.asarray(b[k]).reshape(-1)), f"{what}: {k} differs"


@pytest.fixture(scope="module")
def batch(eng):
    n = 4096
    msgs, off, sk, aux = _inputs(n, 6979)
    pk = eng.sign_batch(1, msgs, off, sk, sk)["pk"]                 # the keys' public points, for the supplied-pk mode
    return msgs, off, sk, aux, pk


@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("hedged", [False, True])
def test_equals_sign_batch_with_the_oracle_nonces(eng, batch, version, mode, hedged):
    from zk_nullifier_sig_amd import capi
    msgs, off, sk, aux, pk = batch
    pk_in = pk if mode else None
    ax = aux if hedged else None
    r = _oracle_r(version, msgs, off, sk, pk_in, ax)
    for level in (0, 1, 2):
        eng.set_sign_uniform(level)
        try:
            want = eng.sign_batch(version, msgs, off, sk, r, pk_in=pk_in)
            got = eng.sign_batch_rfc6979(version, msgs, off, sk, aux=ax, pk_in=pk_in)
        finally:
            eng.set_sign_uniform(1)
        _same(got, want, f"level {level}")
        assert not got["status"].any()
    # page-locked caller arrays (the two-lane host pipeline)
    pm, poff, psk = capi.pinned_copy(msgs), capi.pinned_copy(off), capi.pinned_copy(sk)
    pax = None if ax is None else capi.pinned_copy(ax)
    ppk = None if pk_in is None else capi.pinned_copy(pk_in)
    out = {k: capi.pinned_empty((len(sk), w)) for k, w in [("pk", 64), ("nullifier", 64), ("c", 32), ("s", 32), ("r_point", 64), ("hashed_to_curve_r", 64)]}
    out["status"] = capi.pinned_empty(len(sk))
    _same(eng.sign_batch_rfc6979(version, pm, poff, psk, aux=pax, pk_in=ppk, out=out), want, "page-locked")


def test_device_form_on_a_torch_stream(eng, batch):
    import torch
    msgs, off, sk, aux, pk = batch
    n = len(sk)
    dev = torch.device(f"cuda:{eng.device_id}")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    for version, pk_in, ax in [(1, None, None), (2, pk, aux), (1, pk, None), (2, None, aux)]:
        want = eng.sign_batch(version, msgs, off, sk, _oracle_r(version, msgs, off, sk, pk_in, ax), pk_in=pk_in)
        o = {k: torch.zeros((n, w), dtype=torch.uint8, device=dev) for k, w in [("pk", 64), ("nullifier", 64), ("c", 32), ("s", 32), ("r_point", 64), ("hashed_to_curve_r", 64)]}
        o["status"] = torch.zeros(n, dtype=torch.uint8, device=dev)
        s = torch.cuda.Stream(dev)
        dm, doff, dsk = t(msgs), t(off.view(np.int64)), t(sk)
        dpk, dax = (None if pk_in is None else t(pk_in)), (None if ax is None else t(ax))
        s.wait_stream(torch.cuda.current_stream(dev))
        eng.sign_batch_rfc6979_device(version, n, dm, doff, len(msgs), dsk, dax, dpk, o["pk"], o["nullifier"], o["c"], o["s"], o["r_point"], o["hashed_to_curve_r"], o["status"],
                                      stream=s)
        s.synchronize()
        got = {k: v.cpu().numpy() for k, v in o.items()}
        _same(got, want, f"device v{version}")


def test_two_to_the_twenty(eng):
    import zk_nullifier_sig_amd as plume
    n = 1 << 20
    msgs, off, sk, _ = _inputs(n, 20, maxlen=64)
    a = eng.sign_batch_rfc6979(1, msgs, off, sk)
    b = eng.sign_batch_rfc6979(1, msgs, off, sk)
    _same(a, b, "repeat")
    assert not a["status"].any()
    multi = plume.Engine([eng.device_id, eng.device_id])
    try:
        _same(multi.sign_batch_rfc6979(1, msgs, off, sk), a, "plume_init_multi([0, 0])")
    finally:
        multi.close()
    idx = np.sort(np.random.default_rng(4096).choice(n, size=4096, replace=False))
    sub_off = np.concatenate([[0], np.cumsum((off[idx + 1] - off[idx]).astype(np.int64))]).astype(np.uint64)
    sub_msgs = np.concatenate([msgs[int(off[i]):int(off[i + 1])] for i in idx] + [np.zeros(16, np.uint8)])
    r = _oracle_r(1, sub_msgs, sub_off, sk[idx], None, None)
    want = eng.sign_batch(1, sub_msgs, sub_off, sk[idx], r)
    _same({k: a[k][idx] for k in KEYS}, want, "sampled oracle")
    ok = eng.verify_batch(1, msgs, off, a["pk"], a["nullifier"], a["c"], a["s"], a["r_point"], a["hashed_to_curve_r"])
    assert int(ok.sum()) == n
    rp = np.ascontiguousarray(a["r_point"]).view(np.dtype((np.void, 64))).reshape(-1)
    assert len(np.unique(rp)) == n


def test_domain_separation(eng):
    msgs, off, sk, aux = _inputs(1, 7)
    pk = eng.sign_batch(1, msgs, off, sk, sk)["pk"]
    rps = [eng.sign_batch_rfc6979(v, msgs, off, sk, aux=ax, pk_in=p)["r_point"][0].tobytes() for v in (1, 2) for p in (None, pk) for ax in (None, aux)]
    assert len(set(rps)) == len(rps)


def test_rejected_offsets_and_empty_calls(eng):
    import torch
    msgs, off, sk, _ = _inputs(8, 9, maxlen=40)
    dev = torch.device(f"cuda:{eng.device_id}")
    bad = off.copy().astype(np.int64)
    bad[3] = bad[2] - 1 if bad[2] > 0 else bad[4] + 1               # item 2 decreasing (or item 3: bad[3] > bad[4])
    bad[6] = int(off[-1]) + 10_000                                   # items 5 and 6 reach past the buffer
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    o = {k: torch.zeros((8, w), dtype=torch.uint8, device=dev) for k, w in [("pk", 64), ("nullifier", 64), ("c", 32), ("s", 32), ("r_point", 64), ("hashed_to_curve_r", 64)]}
    st = torch.zeros(8, dtype=torch.uint8, device=dev)
    mb = int(off[-1])
    eng.sign_batch_rfc6979_device(1, 8, t(msgs), t(bad), mb, t(sk), None, None, o["pk"], o["nullifier"], o["c"], o["s"], o["r_point"], o["hashed_to_curve_r"], st)
    torch.cuda.synchronize(dev)
    status = st.cpu().numpy()
    flagged = {i for i in range(8) if not (bad[i + 1] >= bad[i] and bad[i + 1] <= mb)}
    assert flagged and all(status[i] & 2 for i in flagged)
    assert all(status[i] == 0 for i in range(8) if i not in flagged)
    z = np.zeros(0, dtype=np.uint8)
    got = eng.sign_batch_rfc6979(1, z, np.zeros(1, dtype=np.uint64), np.zeros((0, 32), np.uint8))
    assert all(len(v) == 0 for v in got.values())


def test_python_facade(eng):
    import zk_nullifier_sig_amd as plume
    sk = plume.SecretKey.from_bytes(bytes.fromhex("519b423d715f8b581f4fa8ee59f4771a5b44c8130b4e3eacca54a56dda72b464"))
    for v1 in (True, False):
        s = plume.PlumeSigner(sk, v1, eng)
        a, b = s.sign_deterministic(b"An example app message string"), s.sign_deterministic(b"An example app message string")
        assert a.verify(eng) and a == b
        h = s.sign_deterministic(b"An example app message string", aux=bytes(range(32)))
        assert h.verify(eng) and h.s != a.s


def test_cpp_facade(tmp_path):
    import zk_nullifier_sig_amd as plume
    exe = tmp_path / "rfc6979_test"
    libdir = plume.library_path().parent
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"), str(ROOT / "tests" / "abi_cpp" / "rfc6979_test.cpp"), "-L", str(libdir),
                    "-lplume_hip", f"-Wl,-rpath,{libdir}", "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rfc6979_test ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
