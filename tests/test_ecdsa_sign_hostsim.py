"""plume_ecdsa_sign_batch* and plume_eth_message_hash_batch* on the host side (csrc/plume_ecdsa_sign_capi.hip, csrc/plume_eth_hash_capi.hip) under the sanitizers, on the CPU
(tests/_hostsim.py): the two ABI translation units, the self-check's switch
(csrc/plume_selfcheck_capi.hip, tests/hostsim/selfcheck_launch.cpp), the recover stages' launchers (tests/hostsim/ecdsa_launch.cpp: the self-check runs them), the new kernels as host loops (tests/hostsim/ecdsa_sign_launch.cpp) and a driver
(tests/hostsim/ecdsa_sign_driver.cpp) that pins every output to vectors this test writes from the restatement (tests/_ecdsa_sign.py) over the whole fixture: the host form
with chunks of 1, 7 and n, pageable and page-locked arrays, the device form on a caller stream (nothing runs before the caller synchronises), the three uniform levels,
sub-batches, the self-check on (same bytes, the stage list of the header), plume_init_multi contexts over three and eight mock devices, argument errors, every allocation
of a call failing in turn.  ASan + UBSan and TSan, lazy, random and eager schedulers.  One mutant of a launcher, which drops its stream argument, must fail the driver."""
import struct

import numpy as np
import pytest

from tests import _ecdsa_sign as S
from tests import _hostsim as H

UNITS = dict(driver="ecdsa_sign_driver", capi=["plume_ecdsa_sign_capi.hip", "plume_ecdsa_capi.hip", "plume_eth_hash_capi.hip", "plume_selfcheck_capi.hip"],
             launch=["selfcheck_launch.cpp", "ecdsa_launch.cpp", "ecdsa_sign_launch.cpp"])


@pytest.fixture(scope="module")
def vectors(tmp_path_factory):
    """every item of the fixture (its own aux dropped: a call hedges all of its items or none) and what the restatement says of it without and with aux, once; the
    fixture's messages of both modes and their digests in both modes"""
    kats = S.load_kats()
    H = b"".join(bytes.fromhex(e["hash"]) for e in kats["sign"])
    SK = b"".join(bytes.fromhex(e["sk"]) for e in kats["sign"])
    n = len(kats["sign"])
    AUX = np.random.default_rng(5).bytes(32 * n)
    blob = struct.pack("<I", n) + H + SK + AUX
    for aux in (None, AUX):
        r, s, v, st = S.sign_batch(H, SK, aux, 0)
        assert S.BAD_SCALAR in st and int((st == S.OK).sum()) > n - 12
        blob += r.tobytes() + s.tobytes() + v.tobytes() + st.tobytes()
    msgs = [bytes.fromhex(e["msg"]) for e in kats["hash"]]
    off = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint64)
    buf = b"".join(msgs)
    blob += struct.pack("<I", len(msgs)) + off.tobytes() + buf + S.message_hash_batch(buf, off, S.KECCAK256).tobytes() + S.message_hash_batch(buf, off, S.EIP191).tobytes()
    path = tmp_path_factory.mktemp("ecdsa_sign_vectors") / "vectors.bin"
    path.write_bytes(blob)
    return path


@pytest.mark.parametrize("san,runs", H.RUNS)
def test_ecdsa_sign_host_side_under_sanitizers(tmp_path, vectors, san, runs):
    exe = H.build(tmp_path / "b", san, **UNITS)
    for seed, sched in runs:
        H.ok(H.run(exe, vectors, seed, sched=sched), "ecdsa_sign_driver", seed)


def test_the_driver_fails_when_a_launcher_drops_its_stream(tmp_path, vectors):
    r = H.run(H.build(tmp_path / "b", "", **UNITS, defs={"ecdsa_sign_launch.cpp": ["-DECDSA_SIGN_MUTANT_DROPS_STREAM"]}), vectors, 1)
    assert r.returncode != 0 and "ecdsa_sign_driver:" in r.stderr and "one device, host form" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])
