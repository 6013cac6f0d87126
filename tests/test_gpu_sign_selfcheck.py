"""The signer's self-check on the MI355X (include/plume_hip.h, plume_set_sign_selfcheck; gate kernel in csrc/plume_selfcheck_kernels.hip).

Mode 1 must leave honest batches byte-identical to mode 0 (every sign entry point, V1 / V2, pk derived / supplied, uniform levels 0-2, host and device forms) and must
withhold -- all six records zero, status 8 -- exactly the items whose records do not verify.  The input that makes the check fire needs no fault: sign_with_r's shape takes
pk_in from the caller, and a pk_in that is on the curve but is not sk G gives status 0 and records no verifier accepts.  Which items those are comes from the C oracle
(sign with that pk_in, then verify_non_zk), never from the library."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import _oracle_c as OC
from tests import _rfc6979 as R

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
RECS = [("pk", 64), ("nullifier", 64), ("c", 32), ("s", 32), ("r_point", 64), ("hashed_to_curve_r", 64)]
KEYS = [k for k, _ in RECS] + ["status"]
SELFCHECK_FAILED = 8


@pytest.fixture(scope="module")
def eng():
    import zk_nullifier_sig_amd as plume
    e = plume.Engine(0)
    yield e
    e.close()


def _inputs(n, seed, maxlen=300):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, maxlen + 1, size=n)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    msgs = rng.integers(0, 256, size=int(off[-1]) + 16, dtype=np.uint8)
    sk = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    r = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    for a in (sk, r):
        a[:, 0] &= 0x7F                                            # < n
        a[:, 31] |= 1                                              # != 0
    aux = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    return msgs, off, sk, r, aux


def _same(a, b, what, keys=KEYS):
    for k in keys:
        assert np.array_equal(np.asarray(a[k]).reshape(-1), np.asarray(b[k]).reshape(-1)), f"{what}: {k} differs"


class _mode:
    def __init__(self, eng, mode):
        self.eng, self.mode = eng, mode

    def __enter__(self):
        self.eng.set_sign_selfcheck(self.mode)

    def __exit__(self, *a):
        self.eng.set_sign_selfcheck(0)


def _both(eng, call):
    """call() in mode 0 and in mode 1"""
    with _mode(eng, 0):
        a = call()
    with _mode(eng, 1):
        b = call()
    return a, b


@pytest.fixture(scope="module")
def batch(eng):
    n = 4096
    msgs, off, sk, r, aux = _inputs(n, 8)
    pk = OC.sign_batch(1, msgs, off, sk, r, nthreads=16)["pk"]
    rng = np.random.default_rng(88)
    planted = np.zeros(n, dtype=bool)
    planted[rng.choice(n, size=n // 16, replace=False)] = True
    planted[0] = planted[n - 1] = True
    wrong = pk.copy()
    wrong[planted] = np.roll(pk, -1, axis=0)[planted]              # the neighbour's public key: on the curve, not sk G
    return dict(n=n, msgs=msgs, off=off, sk=sk, r=r, aux=aux, pk=pk, wrong=wrong, planted=planted)


def _device_sign(eng, version, b, pk_in, P=64, stream=True, fill=0xAA, derived=False, off=None, want_pk=True):
    """one device-form sign call on a torch stream into arrays pre-filled with `fill`; P = 33: the SEC1 form"""
    import ctypes as C

    import torch
    dev = torch.device(f"cuda:{eng.device_id}")
    n = b["n"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    o = {k: torch.full((n, P if w == 64 else w), fill, dtype=torch.uint8, device=dev) for k, w in RECS}
    o["status"] = torch.full((n,), fill, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(dev) if stream else torch.cuda.current_stream(dev)
    dm, doff, dsk, dr = t(b["msgs"]), t((b["off"] if off is None else off).view(np.int64)), t(b["sk"]), t(b["r"])
    dpk = None if pk_in is None else t(pk_in)
    s.wait_stream(torch.cuda.current_stream(dev))
    mb = int(b["off"][-1])
    if derived:
        eng.sign_batch_rfc6979_device(version, n, dm, doff, mb, dsk, None, dpk, o["pk"], o["nullifier"], o["c"], o["s"], o["r_point"], o["hashed_to_curve_r"], o["status"], stream=s)
    elif P == 64:
        eng.sign_batch_device(version, n, dm, doff, mb, dsk, dr, dpk, o["pk"] if want_pk else None, o["nullifier"], o["c"], o["s"], o["r_point"], o["hashed_to_curve_r"], o["status"], stream=s)
    else:
        d = lambda x: C.c_void_p(0 if x is None else x.data_ptr())  # noqa: E731
        rc = eng._lib.plume_sign_batch_sec1_device(eng._ctx, version, n, d(dm), d(doff), mb, d(dsk), d(dr), d(dpk), d(o["pk"]), d(o["nullifier"]), d(o["c"]), d(o["s"]),
                                                   d(o["r_point"]), d(o["hashed_to_curve_r"]), d(o["status"]), C.c_void_p(s.cuda_stream))
        assert rc == 0
    s.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


# ---------------------------------------------------------------------------------------------------------- 1. honest batches
@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("supplied", [False, True])
def test_honest_batches_are_untouched(eng, batch, version, supplied):
    from zk_nullifier_sig_amd import capi
    b = batch
    pk_in = b["pk"] if supplied else None
    calls = {
        "sign_batch": lambda: eng.sign_batch(version, b["msgs"], b["off"], b["sk"], b["r"], pk_in=pk_in),
        "sign_batch_sec1": lambda: eng.sign_batch_sec1(version, b["msgs"], b["off"], b["sk"], b["r"], pk_in=pk_in),
        "sign_batch_rfc6979": lambda: eng.sign_batch_rfc6979(version, b["msgs"], b["off"], b["sk"], pk_in=pk_in),
        "sign_batch_rfc6979 hedged": lambda: eng.sign_batch_rfc6979(version, b["msgs"], b["off"], b["sk"], aux=b["aux"], pk_in=pk_in),
    }
    for level in (0, 1, 2):
        eng.set_sign_uniform(level)
        try:
            for name, call in calls.items():
                off_, on_ = _both(eng, call)
                _same(on_, off_, f"{name}, level {level}")
                assert not on_["status"].any(), (name, level)
        finally:
            eng.set_sign_uniform(1)
    want = eng.sign_batch(version, b["msgs"], b["off"], b["sk"], b["r"], pk_in=pk_in)
    # page-locked caller arrays (the two-lane host pipeline)
    pm, poff, psk, pr = (capi.pinned_copy(b[k]) for k in ("msgs", "off", "sk", "r"))
    ppk = None if pk_in is None else capi.pinned_copy(pk_in)
    out = {k: capi.pinned_empty((b["n"], w)) for k, w in RECS}
    out["status"] = capi.pinned_empty(b["n"])
    with _mode(eng, 1):
        _same(eng.sign_batch(version, pm, poff, psk, pr, pk_in=ppk, out=out), want, "page-locked")
        # the device form on a torch stream; and with no pk array
        _same(_device_sign(eng, version, b, pk_in), want, "device form")
        got = _device_sign(eng, version, b, pk_in, want_pk=False)
        _same(got, want, "device form, pk = NULL", [k for k in KEYS if k != "pk"])
        assert (got["pk"] == 0xAA).all()
        got33 = _device_sign(eng, version, b, pk_in, P=33)
    with _mode(eng, 0):
        _same(got33, _device_sign(eng, version, b, pk_in, P=33), "device form, SEC1")


# ---------------------------------------------------------------------------------------------------------- 2. mismatched keys
def _oracle_want(version, b, pk_in):
    o = OC.sign_batch(version, b["msgs"], b["off"], b["sk"], b["r"], pk_in=pk_in, nthreads=16)
    assert not o["status"].any()
    return OC.verify_non_zk_batch(version, b["msgs"], b["off"], o["pk"], o["nullifier"], o["s"], o["r_point"], o["hashed_to_curve_r"], o["c"], nthreads=16) == 1


def _check_withheld(got, ref, want, what):
    """got (mode 1) against ref (mode 0) and the oracle's flags: zeros and status 8 where want is false, ref's bytes elsewhere"""
    assert np.array_equal(got["status"], np.where(want, 0, SELFCHECK_FAILED).astype(np.uint8)), what
    for k, _ in RECS:
        assert not got[k][~want].any(), f"{what}: {k} of a withheld item is not all zero"
        assert np.array_equal(got[k][want], ref[k][want]), f"{what}: {k} of a released item differs from mode 0"


@pytest.mark.parametrize("version", [1, 2])
def test_mismatched_keys_are_withheld_and_only_they(eng, batch, version):
    b = batch
    want = _oracle_want(version, b, b["wrong"])
    assert np.array_equal(want, ~b["planted"])                     # the oracle agrees that exactly the planted keys break the signature
    calls = {
        "host, 64": lambda: eng.sign_batch(version, b["msgs"], b["off"], b["sk"], b["r"], pk_in=b["wrong"]),
        "host, 33": lambda: eng.sign_batch_sec1(version, b["msgs"], b["off"], b["sk"], b["r"], pk_in=b["wrong"]),
        "device, 64": lambda: _device_sign(eng, version, b, b["wrong"]),
        "device, 33": lambda: _device_sign(eng, version, b, b["wrong"], P=33),
    }
    for name, call in calls.items():
        ref, got = _both(eng, call)
        assert not ref["status"].any(), name                        # mode 0: the signer calls every item good ...
        _check_withheld(got, ref, want, f"v{version} {name}")
    ref = calls["host, 64"]()
    ok = eng.verify_batch(version, b["msgs"], b["off"], ref["pk"], ref["nullifier"], ref["c"], ref["s"], ref["r_point"], ref["hashed_to_curve_r"])
    assert np.array_equal(ok == 1, want)                           # ... and hands out records verify_batch rejects: the gap the check closes
    # derived nonces: r lives on the device only, so the flags are the same keys' and the released bytes are mode 0's
    ref, got = _both(eng, lambda: eng.sign_batch_rfc6979(version, b["msgs"], b["off"], b["sk"], pk_in=b["wrong"]))
    _check_withheld(got, ref, want, f"v{version} rfc6979")
    ref, got = _both(eng, lambda: _device_sign(eng, version, b, b["wrong"], derived=True))
    _check_withheld(got, ref, want, f"v{version} rfc6979 device")


# ---------------------------------------------------------------------------------------------------------- 3. items the signer rejects itself
def test_items_the_signer_rejects_come_out_as_before(eng):
    n = 64
    msgs, off, sk, r, _ = _inputs(n, 3, maxlen=40)
    pk = OC.sign_batch(1, msgs, off, sk, r, nthreads=4)["pk"]
    N = bytes.fromhex("FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141")
    sk[3] = 0
    r[5] = 0
    r[7] = np.frombuffer(N, dtype=np.uint8)
    r[9] = 0xFF
    bad_pk = pk.copy()
    bad_pk[11, 63] ^= 1                                            # off the curve
    b = dict(n=n, msgs=msgs, off=off, sk=sk, r=r)
    for version in (1, 2):
        for pk_in in (None, bad_pk):
            a0, a1 = _both(eng, lambda: eng.sign_batch(version, msgs, off, sk, r, pk_in=pk_in))
            _same(a1, a0, f"host v{version}")
            assert all(a0["status"][i] != 0 for i in (3, 5, 7, 9)) and (pk_in is None or a0["status"][11] != 0)
            s0, s1 = _both(eng, lambda: eng.sign_batch_sec1(version, msgs, off, sk, r, pk_in=pk_in))
            _same(s1, s0, f"host sec1 v{version}")
        bad = off.copy().astype(np.int64)
        bad[3] = bad[2] - 1 if bad[2] > 0 else bad[4] + 1           # decreasing
        bad[20] = int(off[-1]) + 10_000                              # reaches past the buffer
        d0, d1 = _both(eng, lambda: _device_sign(eng, version, b, bad_pk, off=bad.view(np.uint64)))
        _same(d1, d0, f"device v{version}")
        assert d0["status"][19] != 0 and d0["status"][20] != 0
        assert d0["status"][2] != 0 or d0["status"][3] != 0             # the decreasing offset


# ---------------------------------------------------------------------------------------------------------- 4. 2^20 items
def test_two_to_the_twenty(eng):
    import torch

    import zk_nullifier_sig_amd as plume
    n = 1 << 20
    msgs, off, sk, _, _ = _inputs(n, 20, maxlen=64)
    ref, got = _both(eng, lambda: eng.sign_batch_rfc6979(1, msgs, off, sk))
    _same(got, ref, "2^20 honest")
    assert not got["status"].any()
    planted = np.sort(np.random.default_rng(1024).choice(n, size=1024, replace=False))
    wrong = ref["pk"].copy()
    wrong[planted] = ref["pk"][(planted + 1) % n]
    ref, got = _both(eng, lambda: eng.sign_batch_rfc6979(1, msgs, off, sk, pk_in=wrong))
    flags = np.ones(n, dtype=bool)
    flags[planted] = False
    # the oracle on the planted items and as many others: sign with the nonce the library derived (RFC 6979 restated in tests/_rfc6979.py), then verify_non_zk
    idx = np.unique(np.concatenate([planted, np.random.default_rng(7).choice(n, size=1024, replace=False)]))
    sub_off = np.concatenate([[0], np.cumsum((off[idx + 1] - off[idx]).astype(np.int64))]).astype(np.uint64)
    sub_msgs = np.concatenate([msgs[int(off[i]):int(off[i + 1])] for i in idx] + [np.zeros(16, np.uint8)])
    sub_r = np.frombuffer(R.plume_nonces(1, sub_msgs, sub_off, sk[idx], wrong[idx], None), dtype=np.uint8).reshape(-1, 32)
    sub = dict(msgs=sub_msgs, off=sub_off, sk=np.ascontiguousarray(sk[idx]), r=sub_r)
    assert np.array_equal(_oracle_want(1, sub, np.ascontiguousarray(wrong[idx])), flags[idx])
    _check_withheld(got, ref, flags, "2^20 planted")
    with _mode(eng, 1):
        multi = plume.Engine([eng.device_id, eng.device_id])
        try:
            multi.set_sign_selfcheck(1)
            assert multi.sign_selfcheck() == 1
            _same(multi.sign_batch_rfc6979(1, msgs, off, sk, pk_in=wrong), got, "plume_init_multi([d, d])")
        finally:
            multi.close()
        # two batches in flight on two streams
        dev = torch.device(f"cuda:{eng.device_id}")
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        dm, doff, dsk, dpk = t(msgs), t(off.view(np.int64)), t(sk), t(wrong)
        eng.set_in_flight(2)
        try:
            outs, streams = [], [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
            for s in streams:
                s.wait_stream(torch.cuda.current_stream(dev))
                o = {k: torch.full((n, w), 0xAA, dtype=torch.uint8, device=dev) for k, w in RECS}
                o["status"] = torch.full((n,), 0xAA, dtype=torch.uint8, device=dev)
                eng.sign_batch_rfc6979_device(1, n, dm, doff, int(off[-1]), dsk, None, dpk, o["pk"], o["nullifier"], o["c"], o["s"], o["r_point"], o["hashed_to_curve_r"],
                                              o["status"], stream=s)
                outs.append(o)
            for s, o in zip(streams, outs):
                s.synchronize()
                _same({k: v.cpu().numpy() for k, v in o.items()}, got, "two in flight")
        finally:
            eng.set_in_flight(1)


# ---------------------------------------------------------------------------------------------------------- 5. the switch itself
def test_switch_stage_list_and_environment(eng, batch):
    from zk_nullifier_sig_amd import capi
    b = batch
    assert eng.sign_selfcheck() == 0
    eng.set_sign_selfcheck(1)
    assert eng.sign_selfcheck() == 1
    with pytest.raises(capi.PlumeHipError):
        eng.set_sign_selfcheck(2)
    assert eng.sign_selfcheck() == 1
    eng.set_stage_timing(True)
    try:
        _device_sign(eng, 1, b, None, stream=False)
        names = [k for k, _ in eng.last_stage_times()]
    finally:
        eng.set_stage_timing(False)
        eng.set_sign_selfcheck(0)
    assert names[-1] == "sign_release", names
    assert names.index("sign_final") < names.index("verify_msm") < names.index("verify_finalize") < len(names) - 1, names
    code = "import zk_nullifier_sig_amd as p; e = p.Engine(0); print('mode', e.sign_selfcheck()); e.close()"
    for val, want in (("1", "mode 1"), ("0", "mode 0")):
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, PLUME_SIGN_SELFCHECK=val), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and want in r.stdout, (r.stdout[-500:], r.stderr[-2000:])


# ---------------------------------------------------------------------------------------------------------- 6. façades
def test_python_facade(eng):
    import zk_nullifier_sig_amd as plume
    G = plume.AffinePoint.generator()
    sk, r = 0x519b423d715f8b581f4fa8ee59f4771a5b44c8130b4e3eacca54a56dda72b464, 0x93b9323b629f251b8f3fc2dd11f4672c5544e8230d493eceea98a90bda789808
    right = plume.PlumeSigner(plume.SecretKey(sk), True, eng).sign_deterministic(b"m").pk
    assert right != G
    for version in (plume.PlumeVersion.V1, plume.PlumeVersion.V2):
        sig = plume.sign_with_r((G, sk), b"message", r, version, eng)                 # G is on the curve and is not sk G
        assert not plume.verify_non_zk(sig, G, b"message", version, eng)
        with _mode(eng, 1):
            with pytest.raises(plume.PlumeSelfCheckError):
                plume.sign_with_r((G, sk), b"message", r, version, eng)
            good = plume.sign_with_r((right, sk), b"message", r, version, eng)
        assert plume.verify_non_zk(good, right, b"message", version, eng)


def test_cpp_facade(tmp_path):
    import zk_nullifier_sig_amd as plume
    exe = tmp_path / "selfcheck_test"
    libdir = plume.library_path().parent
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"), str(ROOT / "tests" / "abi_cpp" / "selfcheck_test.cpp"), "-L", str(libdir),
                    "-lplume_hip", f"-Wl,-rpath,{libdir}", "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "selfcheck_test ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
