"""plume_eth_tx_sign_batch* on the host side (csrc/plume_eth_tx_sign_capi.hip) under the sanitizers, on the CPU (tests/_hostsim.py):
the ABI's translation unit, the self-check's switch (csrc/plume_selfcheck_capi.hip, tests/hostsim/selfcheck_launch.cpp), the launchers of the sign and recover stages (tests/hostsim/ecdsa_sign_launch.cpp,
ecdsa_launch.cpp), the two new kernels as host loops
(tests/hostsim/eth_tx_sign_launch.cpp) and a driver (tests/hostsim/eth_tx_sign_driver.cpp) that pins every output to vectors this test writes from the restatement
(tests/_eth_tx_sign.py): the host form with chunks that cut the batch into 1, 2 and many pieces and on sub-ranges, the assembled out compared whole; the device form on a
caller stream; sub-batches; the self-check and the stage lists; plume_init_multi contexts over two and eight mock devices; argument errors; every allocation of a call
failing in turn; the staged sk and aux wiped on success and on failure.  ASan + UBSan and TSan, lazy, random and eager schedulers: stand-alone programs, nothing is
loaded into Python.  One mutant of the launcher, an assemble that writes one byte past out_len, must fail the driver."""
import struct

import numpy as np
import pytest

from tests import _eth_tx as T
from tests import _eth_tx_sign as X
from tests import _hostsim as H
from tests import _keccak as K

UNITS = dict(driver="eth_tx_sign_driver", capi=["plume_eth_tx_sign_capi.hip", "plume_ecdsa_sign_capi.hip", "plume_ecdsa_capi.hip", "plume_selfcheck_capi.hip"],
             launch=["ecdsa_launch.cpp", "ecdsa_sign_launch.cpp", "eth_tx_sign_launch.cpp", "selfcheck_launch.cpp"])


@pytest.fixture(scope="module")
def vectors(tmp_path_factory):
    """the first 72 short items of both fixtures as one batch (framed and unframed items alternate; keys out of range and the refused v among the new vectors are added) and what
    the restatement says of them without and with aux, once"""
    items, keys = X.fixture_batch()
    short = [(it, sk) for it, sk in zip(items, keys) if len(it) < 1000]
    extra = [(bytes.fromhex(e["unsigned"]), bytes.fromhex(e["sk"])) for e in X.load_kats()["items"] if e["status"] in (X.BAD_SCALAR, X.IDENTITY)]
    picked = short[:72] + extra
    items, keys = [p[0] for p in picked], [p[1] for p in picked]
    n = len(items)
    txs, off = T.pack(items)
    sk = b"".join(keys)
    aux = b"".join(K.keccak256(b"hostsim aux %d" % j) for j in range(n))
    blob = struct.pack("<I", n) + off.tobytes() + txs.tobytes() + sk + aux
    for a in (None, aux):
        w = X.sign_batch(txs, off, sk, a)
        assert (w["status"] == 0).sum() >= 20 and (w["status"] == X.BAD_TX).sum() >= 20 and (w["status"] == X.BAD_SCALAR).sum() == 3
        blob += b"".join(np.ascontiguousarray(w[k]).tobytes() for k in ("out", "out_len", "status", "hash", "r", "s", "v", "chain_id", "tx_type"))
    path = tmp_path_factory.mktemp("eth_tx_sign_vectors") / "vectors.bin"
    path.write_bytes(blob)
    return path


@pytest.mark.parametrize("san,runs", H.RUNS)
def test_eth_tx_sign_host_side_under_sanitizers(tmp_path, vectors, san, runs):
    exe = H.build(tmp_path / "b", san, **UNITS)
    for seed, sched in runs:
        H.ok(H.run(exe, vectors, seed, sched=sched), "eth_tx_sign_driver", seed)


def test_the_driver_fails_when_the_assemble_writes_past_out_len(tmp_path, vectors):
    r = H.run(H.build(tmp_path / "b", "", **UNITS, defs={"eth_tx_sign_launch.cpp": ["-DETH_TX_SIGN_MUTANT_WRITES_PAST"]}), vectors, 1)
    assert r.returncode != 0 and "eth_tx_sign_driver:" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])
