"""The signer's self-check on the host side (the gate in csrc/plume_capi.hip's sign_device, csrc/plume_selfcheck_capi.hip) under the sanitizers, on the CPU
(tests/_hostsim.py): the ABI's translation unit and the derived-nonce one, k_sign_release as a host loop (tests/hostsim/selfcheck_launch.cpp) and a driver (tests/hostsim/selfcheck_driver.cpp) that checks every output against the
C oracle's sign + verify_non_zk on batches with planted wrong keys and, after every call, that no device allocation holds the c or s of a withheld item.  ASan + UBSan and
TSan, lazy, random and eager schedulers.  Three mutants must each fail the driver: a release launcher that ignores the verdict, the staging wipe removed, and the sign
kernels pointed at the caller's arrays instead of the staging (caught with a release launcher that writes nothing: the caller's arrays must still hold their pre-fill)."""
import shutil

import pytest

from tests import _hostsim as H
from tests._hostsim import CSRC, ROOT

UNITS = dict(driver="selfcheck_driver", capi=["plume_selfcheck_capi.hip", "plume_nonce_capi.hip"], launch=["selfcheck_launch.cpp", "nonce_launch.cpp"])
WIPE = "        HIPCHK(hipMemsetAsync(ctx->scstage.p, 0, kStageBytes * n, st));"
REDIRECT = "    if (selfcheck) { pk = g_pk; nul = g_nul; c = g_c; s = g_s; rpt = g_rpt; hr = g_hr; status = g_status; out33 = false; }"


@pytest.mark.parametrize("san,runs", H.RUNS)
def test_selfcheck_host_side_under_sanitizers(tmp_path, san, runs):
    exe = H.build(tmp_path / "b", san, **UNITS)
    for seed, sched in runs:
        H.ok(H.run(exe, seed, sched=sched), "selfcheck_driver", seed)


def _mutated_csrc(tmp_path, old, new):
    src = (CSRC / "plume_capi.hip").read_text()
    assert src.count(old) == 1, "the mutant's text is no longer in plume_capi.hip -- update the mutant"
    csrc = tmp_path / "pkg" / "csrc"                              # ../../include from csrc, as in the tree
    shutil.copytree(CSRC, csrc, ignore=shutil.ignore_patterns("*.o", "*.so"))
    (tmp_path / "include").mkdir()
    shutil.copy(ROOT / "include" / "plume_hip.h", tmp_path / "include" / "plume_hip.h")
    (csrc / "plume_capi.hip").write_text(src.replace(old, new))
    return csrc


def test_the_driver_fails_when_the_release_ignores_the_verdict(tmp_path):
    r = H.run(H.build(tmp_path / "b", "", **UNITS, defs={"selfcheck_launch.cpp": ["-DSELFCHECK_MUTANT_IGNORES_VERDICT"]}), 1)
    assert r.returncode != 0 and "selfcheck_driver:" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])


def test_the_driver_fails_when_the_staging_is_not_wiped(tmp_path):
    r = H.run(H.build(tmp_path / "b", "", **UNITS, csrc=_mutated_csrc(tmp_path, WIPE, "")), 1)
    assert r.returncode != 0 and "!sec.count(r)" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])


def test_the_driver_fails_when_the_sign_kernels_write_the_callers_arrays(tmp_path):
    """with a release launcher that writes nothing the caller's arrays keep their pre-fill -- unless the sign kernels were pointed at them"""
    nothing = {"selfcheck_launch.cpp": ["-DSELFCHECK_RELEASE_NOTHING"]}
    H.ok(H.run(H.build(tmp_path / "good", "", **UNITS, defs=nothing), 1, "prefill"), "selfcheck_driver", 1)
    r = H.run(H.build(tmp_path / "b", "", **UNITS, csrc=_mutated_csrc(tmp_path, REDIRECT, ""), defs=nothing), 1, "prefill")
    assert r.returncode != 0 and "all_fill" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])
