"""plume_eth_address_batch* on the host side (csrc/plume_eth_capi.hip) under the sanitizers, on the CPU (tests/_hostsim.py): the ABI's
translation unit, k_eth_address as a host loop (tests/hostsim/eth_launch.cpp) and a driver (tests/hostsim/eth_driver.cpp) that pins every
output to vectors this test writes from the Python restatement (tests/_keccak.py): the host form with chunks smaller than n, plume_init_multi contexts over three and
eight mock devices, the device form on a caller stream (nothing runs before the caller synchronises), two calls back to back on one stream, every allocation of a call
failing in turn, no table built.  ASan + UBSan and TSan, lazy, random and eager schedulers.  One mutant of the launcher, which drops its stream argument, must fail the
driver."""
import struct

import pytest

from tests import _hostsim as H
from tests import _keccak as K

UNITS = dict(driver="eth_driver", capi=["plume_eth_capi.hip"], launch=["eth_launch.cpp"])


@pytest.fixture(scope="module")
def vectors(tmp_path_factory):
    """per key format: 64 keys with every invalid kind planted (first, last and in between), status, raw address, EIP-55 record -- from the restatement, once"""
    blob = b""
    for fmt in ("affine64", "sec1"):
        bad = [rec for _, rec in K.invalid_keys(fmt)]
        keys = [k.tobytes() for k in K.sample_keys(64 - len(bad), 21 if fmt == "sec1" else 20, fmt)]
        for j, rec in enumerate(bad):
            keys.insert(0 if j == 0 else len(keys) if j == 1 else 9 * j, rec)
        raw, st = K.eth_address_batch(b"".join(keys), None, fmt, "raw20")
        eip, st2 = K.eth_address_batch(b"".join(keys), None, fmt, "eip55")
        assert list(st) == list(st2) and int((st == K.INVALID).sum()) == len(bad) and st[0] == st[-1] == K.INVALID
        blob += struct.pack("<I", len(keys)) + b"".join(keys) + st.tobytes() + raw.tobytes() + eip.tobytes()
    path = tmp_path_factory.mktemp("eth_vectors") / "vectors.bin"
    path.write_bytes(blob)
    return path


@pytest.mark.parametrize("san,runs", H.RUNS)
def test_eth_address_host_side_under_sanitizers(tmp_path, vectors, san, runs):
    exe = H.build(tmp_path / "b", san, **UNITS)
    for seed, sched in runs:
        H.ok(H.run(exe, vectors, seed, sched=sched), "eth_driver", seed)


def test_the_driver_fails_when_the_launcher_drops_its_stream(tmp_path, vectors):
    r = H.run(H.build(tmp_path / "b", "", **UNITS, defs={"eth_launch.cpp": ["-DETH_MUTANT_DROPS_STREAM"]}), vectors, 1)
    assert r.returncode != 0 and "eth_driver:" in r.stderr and "one device, host form" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])
