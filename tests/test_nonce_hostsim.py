"""The derived-nonce signer's host side (csrc/plume_nonce_capi.hip and the nonce hook of plume_capi.hip) under the sanitizers, on the CPU (tests/_hostsim.py): the ABI's translation unit,
k_sign_nonce as a host loop (tests/hostsim/nonce_launch.cpp) and a driver (tests/hostsim/nonce_driver.cpp) that checks every output against the C oracle's sign given the
lane body's nonces and, after every call, that no device allocation still holds a derived nonce or a staged secret: host and device forms, one device and eight, pieces of
5-64 items, pageable and page-locked arrays, an allocation failure at every allocation of a call, argument errors.  ASan + UBSan and TSan, random and eager schedulers; a
mutant that drops the nonce buffer's wipe must fail."""
import shutil

import pytest

from tests import _hostsim as H
from tests._hostsim import CSRC, ROOT

UNITS = dict(driver="nonce_driver", capi=["plume_nonce_capi.hip"], launch=["nonce_launch.cpp"])
WIPE = "    if (nonce_fn) HIPCHK(hipMemsetAsync(ctx->nonce.p, 0, 32 * n, st));"


@pytest.mark.parametrize("san,runs", H.RUNS)
def test_nonce_host_side_under_sanitizers(tmp_path, san, runs):
    exe = H.build(tmp_path / "b", san, **UNITS)
    for seed, sched in runs:
        H.ok(H.run(exe, seed, sched=sched), "nonce_driver", seed)


def test_the_driver_fails_when_the_nonce_buffer_is_not_wiped(tmp_path):
    """mutant: sign_device no longer wipes the workspace nonce buffer -- the driver's scan of device memory must find a nonce"""
    src = (CSRC / "plume_capi.hip").read_text()
    assert src.count(WIPE) == 1
    csrc = tmp_path / "pkg" / "csrc"                              # ../../include from csrc, as in the tree
    shutil.copytree(CSRC, csrc, ignore=shutil.ignore_patterns("*.o", "*.so"))
    (tmp_path / "include").mkdir()
    shutil.copy(ROOT / "include" / "plume_hip.h", tmp_path / "include" / "plume_hip.h")
    (csrc / "plume_capi.hip").write_text(src.replace(WIPE, ""))
    r = H.run(H.build(tmp_path / "b", "", **UNITS, csrc=csrc), 1)
    assert r.returncode != 0 and "!sec.count(r)" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])
