"""plume_hd_*_batch* on the host side (csrc/plume_hd_capi.hip) under the sanitizers, on the CPU (tests/_hostsim.py): the ABI's translation
unit, the new kernels as host loops (tests/hostsim/hd_launch.cpp) and a driver (tests/hostsim/hd_driver.cpp) that pins every output to vectors this test writes from the
restatement (tests/_hd.py): the host form with chunks that cut the batch into 1, 2 and many pieces and on sub-ranges; both SHARED flags -- a whole-call input that was
advanced, or a shared secret parent that was wiped behind the first piece and not uploaded again, gives wrong bytes --; NULL optional outputs; the device form on a caller
stream; the uniform levels, sub-batches and the stage lists; plume_init_multi contexts over two and eight mock devices; argument errors; every allocation of a call failing
in turn; and after every call, failed ones included, no device allocation but the caller's own holding a key or a chain code of the batch.  ASan + UBSan and TSan, lazy,
random and eager schedulers: stand-alone programs, nothing is loaded into Python.  One mutant of the launcher, a finish that leaves a byte of a failed item's chain code,
must fail the driver."""
import struct

import numpy as np
import pytest

from tests import _hd as H
from tests import _hostsim as S
from tests import _keccak as K

UNITS = dict(driver="hd_driver", capi=["plume_hd_capi.hip"], launch=["hd_launch.cpp"])


@pytest.fixture(scope="module")
def vectors(tmp_path_factory):
    """37 seeded parents with invalid ones planted, depth-3 paths with hardened and plain indices, and what the restatement says of every recorded call, once"""
    n, depth, seed_len = 37, 3, 33
    sk, chain = H.seeded_nodes(n, 4242)
    for j, v in enumerate((0, H.N, 2**256 - 1)):
        sk[6 + 9 * j] = np.frombuffer(H.b32(v), np.uint8)
    path = H.seeded_paths(n, depth, 4243)
    ppath = path & np.uint32(0x7FFFFFFF)
    ppath[5, 1] = H.H + 1
    ppath[19, 2] = 2**32 - 1
    pk = H.pk_of(np.where((sk == 0).all(axis=1, keepdims=True) | (sk[:, :1] >= 0x80), np.uint8(1), sk))
    for j, (_, rec) in enumerate(K.invalid_keys("affine64")[:4]):
        pk[2 + 7 * j] = np.frombuffer(rec, np.uint8)
    seeds = np.random.default_rng(4244).integers(0, 256, (n, seed_len), dtype=np.uint8)
    blob = struct.pack("<3I", n, depth, seed_len) + sk.tobytes() + chain.tobytes() + path.tobytes() + pk.tobytes() + ppath.tobytes() + seeds.tobytes()
    cat = lambda arrays: b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)  # noqa: E731
    priv = H.derive_priv_batch(sk, chain, path, depth)
    pub = H.derive_pub_batch(pk, chain, ppath, depth)
    assert (priv[4] == H.BAD_SCALAR).sum() == 3 and (pub[3] == H.BAD_SCALAR).sum() == 4 and (pub[3] == H.HARDENED_PUB).sum() == 2 and priv[4][0] == 0 and pub[3][0] == 0
    blob += cat(priv) + cat(pub)
    blob += cat(H.derive_priv_batch(sk[:1], chain[:1], path, depth, H.SHARED_PARENT))
    blob += cat(H.derive_priv_batch(sk, chain, path[:1], depth, H.SHARED_PATH))
    blob += cat(H.derive_pub_batch(pk[:1], chain[:1], ppath[:1], depth, H.SHARED_PARENT | H.SHARED_PATH, n=n))
    blob += cat(H.master_batch(seeds, seed_len))
    p = tmp_path_factory.mktemp("hd_vectors") / "vectors.bin"
    p.write_bytes(blob)
    return p


@pytest.mark.parametrize("san,runs", S.RUNS)
def test_hd_host_side_under_sanitizers(tmp_path, vectors, san, runs):
    exe = S.build(tmp_path / "b", san, **UNITS)
    for seed, sched in runs:
        S.ok(S.run(exe, vectors, seed, sched=sched), "hd_driver", seed)


def test_the_driver_fails_when_a_failed_item_is_not_zeroed(tmp_path, vectors):
    r = S.run(S.build(tmp_path / "b", "", **UNITS, defs={"hd_launch.cpp": ["-DHD_MUTANT_KEEPS_FAILED"]}), vectors, 1)
    assert r.returncode != 0 and "hd_driver:" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])
