"""plume_eth_tx_parse_batch* and plume_eth_tx_sender_batch* on the host side (csrc/plume_eth_tx_capi.hip) under the sanitizers, on the CPU
(tests/_hostsim.py): the ABI's translation unit, the recover stages' launchers (tests/hostsim/ecdsa_launch.cpp), k_eth_tx_parse as a host loop
(tests/hostsim/eth_tx_launch.cpp) and a driver (tests/hostsim/eth_tx_driver.cpp) that pins every output to vectors this test writes from the restatements
(tests/_eth_tx.py, tests/_ecdsa.py) over the committed fixture: the host form with chunks of 1, 7 and n, the device form on a caller stream (nothing runs before the caller
synchronises), sub-batches, the stage lists, plume_init_multi contexts over three and eight mock devices, argument errors, every allocation of a call failing in turn, no
table built by a context that only parses.  ASan + UBSan and TSan, lazy, random and eager schedulers: stand-alone programs, nothing is loaded into Python.  One mutant of
the launcher, which drops its stream argument, must fail the driver."""
import struct

import pytest

from tests import _ecdsa as E
from tests import _eth_tx as T
from tests import _hostsim as H

UNITS = dict(driver="eth_tx_driver", capi=["plume_eth_tx_capi.hip", "plume_ecdsa_capi.hip"], launch=["ecdsa_launch.cpp", "eth_tx_launch.cpp"])


@pytest.fixture(scope="module")
def vectors(tmp_path_factory):
    """the fixture's items (the two long ones left out: the recover stages of a CPU are slow enough) and what the restatements say of them, once"""
    raws = [bytes.fromhex(e["raw"]) for e in T.load_kats()["items"] if len(e["raw"]) < 4000]
    txs, off = T.pack(raws)
    p = T.parse_batch(txs, off)
    pk, addr, st = E.recover_batch(p["hash"], p["r"], p["s"], p["v"], None, "affine64", "raw20", E.LOW_S)
    assert (st[p["status"] == T.INVALID] == 3).all() and int((st == 1).sum()) > 100 and int(((st == 3) & (p["status"] == T.OK)).sum()) >= 5
    blob = struct.pack("<I", len(raws)) + off.tobytes() + txs.tobytes() + b"".join(p[k].tobytes() for k in ("hash", "r", "s", "v", "tx_type", "status", "chain_id"))
    blob += pk.tobytes() + addr.tobytes() + st.tobytes()
    path = tmp_path_factory.mktemp("eth_tx_vectors") / "vectors.bin"
    path.write_bytes(blob)
    return path


@pytest.mark.parametrize("san,runs", H.RUNS)
def test_eth_tx_host_side_under_sanitizers(tmp_path, vectors, san, runs):
    exe = H.build(tmp_path / "b", san, **UNITS)
    for seed, sched in runs:
        H.ok(H.run(exe, vectors, seed, sched=sched), "eth_tx_driver", seed)


def test_the_driver_fails_when_the_launcher_drops_its_stream(tmp_path, vectors):
    r = H.run(H.build(tmp_path / "b", "", **UNITS, defs={"eth_tx_launch.cpp": ["-DETH_TX_MUTANT_DROPS_STREAM"]}), vectors, 1)
    assert r.returncode != 0 and "eth_tx_driver:" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])
