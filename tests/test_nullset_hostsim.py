"""The persistent nullifier set's host side (csrc/plume_nullset_capi.hip) under the sanitizers, on the CPU (tests/_hostsim.py; no oracle): the set's
translation unit, its kernels as host loops (tests/hostsim/nullset_launch.cpp) and a driver (tests/hostsim/nullset_driver.cpp) that checks every answer against a std::set: host and device forms, two caller streams,
a multi-device context, a set outliving its context, destroy with work queued, an allocation failure at every allocation of a growing insert, argument errors.  Run under
ASan + UBSan and under TSan with the mock's random stream scheduler; one mutant shows the harness notices a missing ordering."""
import shutil

import pytest

from tests import _hostsim as H
from tests._hostsim import CSRC, ROOT

UNITS = dict(driver="nullset_driver", capi=["plume_nullset_capi.hip"], launch=["nullset_launch.cpp"], oracle=False)


@pytest.mark.parametrize("san,runs", [("address,undefined", [(1, None), (2, "random:2"), (3, "random:3"), (4, "random:4"), (5, "eager")]),
                                      ("thread", [(6, "random:6"), (7, "random:7")])])
def test_nullset_host_side_under_sanitizers(tmp_path, san, runs):
    exe = H.build(tmp_path / "b", san, **UNITS)
    for seed, sched in runs:
        H.ok(H.run(exe, seed, sched=sched), "nullset_driver", seed)


def test_the_driver_fails_when_an_operation_does_not_wait_for_the_previous_one(tmp_path):
    """mutant: operations on different streams no longer wait for the set's last one -- the random scheduler must turn that into a wrong answer"""
    src = (CSRC / "plume_nullset_capi.hip").read_text()
    old = "if (s->last_stream != st) NSCHK(hipStreamWaitEvent(st, s->last, 0));"
    assert src.count(old) == 1
    pkg = tmp_path / "pkg" / "csrc"
    pkg.mkdir(parents=True)
    (tmp_path / "pkg" / "include").mkdir()
    shutil.copy(ROOT / "include" / "plume_hip.h", tmp_path / "pkg" / "include" / "plume_hip.h")
    (pkg / "plume_nullset_capi.hip").write_text(src.replace(old, ""))
    exe = H.build(tmp_path / "b", "", **UNITS, sources={"plume_nullset_capi.hip": pkg / "plume_nullset_capi.hip"})
    results = [H.run(exe, seed, sched=f"random:{seed}") for seed in (1, 2, 3)]
    assert any(r.returncode != 0 for r in results), [r.stdout[-300:] for r in results]
