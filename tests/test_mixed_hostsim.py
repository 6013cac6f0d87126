"""Every call family on ONE mock context under the sanitizers (tests/_hostsim.py; driver: tests/hostsim/mixed_driver.cpp): all thirteen family translation units of csrc
and every launcher file of tests/hostsim linked into one stand-alone program.  The families' own drivers each see one family per context; here a context's workspace is
dirty with other families' bytes, counters and flags, and every output byte of every call must equal what a context that has done nothing else gives: every ordered pair
of different families, large then small within a family, a seeded walk of 300 calls over forms, streams and settings, and that walk on two mock devices, with two
batches in flight and with host calls of three or more pieces.  ASan + UBSan under the lazy, random and eager schedulers, TSan under the random one.

Three mutants of csrc, CPU only, show that this tier sees what it is for -- each must make the driver name a call, not crash:
  - verify_device no longer clears the flag it owns (the redo list is the verifier's again): plume_last_redo_tasks keeps refusing behind a verify call that follows an
    ECDSA-family call.  The verify family's own driver (recover_driver) cannot notice: its contexts never see an ECDSA call;
  - sign_device places its staged status array by the ECDSA signer's 195-byte stride instead of its own: the self-checked signer's staged records are overwritten;
  - the SEC1 decompression stage keeps a reject flag it finds set instead of writing every item's flag: dirty (0xA5) memory is cleared, so a context that has done nothing
    else answers right, and only a call behind a larger SEC1 call -- whose planted items sit elsewhere -- rejects items it should accept."""
import shutil

import pytest

from tests import _hostsim as H

ROOT = H.ROOT
UNITS = dict(driver="mixed_driver",
             capi=["plume_eth_capi.hip", "plume_eth_hash_capi.hip", "plume_ecdsa_capi.hip", "plume_eth_tx_capi.hip", "plume_merkle_capi.hip", "plume_ecdsa_sign_capi.hip",
                   "plume_eth_tx_sign_capi.hip", "plume_hd_capi.hip", "plume_kdf_capi.hip", "plume_recover_capi.hip", "plume_nonce_capi.hip", "plume_selfcheck_capi.hip",
                   "plume_nullset_capi.hip"],
             launch=["eth_launch.cpp", "ecdsa_launch.cpp", "eth_tx_launch.cpp", "merkle_launch.cpp", "ecdsa_sign_launch.cpp", "eth_tx_sign_launch.cpp", "hd_launch.cpp",
                     "kdf_launch.cpp", "recover_launch.cpp", "nonce_launch.cpp", "selfcheck_launch.cpp", "nullset_launch.cpp"])
RECOVER = dict(driver="recover_driver", capi=["plume_recover_capi.hip"], launch=["recover_launch.cpp"])

REARM = "if (k == 0) { ctx->redo_counters.clear(); ctx->redo_foreign = false; }"
STATUS = "*const g_status = stg + 320 * n,"
PREFLAG = "a.preflags[i] = ok ? 0 : 1;"
DIFFERS = "differs from the result of a context that has done nothing else"
MUTANTS = {     # name -> (file of csrc, text, its replacement, what the driver must say, the family's own driver where that must still pass)
    "verify no longer clears the flag it owns": ("plume_capi.hip", REARM, "if (k == 0) ctx->redo_counters.clear();", "plume_last_redo_tasks gave", RECOVER),
    "the signer's staged status at the ECDSA signer's stride": ("plume_capi.hip", STATUS, "*const g_status = stg + 195 * n,", DIFFERS, None),
    "the decompression keeps a reject flag it finds": ("plume_stages.h", PREFLAG, "a.preflags[i] = (!ok || a.preflags[i] == 1) ? 1 : 0;", "verify_sec1[9] (", None),
}


def test_every_family_unit_and_launcher_is_linked():
    """the list above is the tree's: a new family file must join the mixed program"""
    capi = sorted(p.name for p in H.CSRC.glob("plume_*_capi.hip"))
    launch = sorted(p.name for p in H.HOSTSIM.glob("*_launch.cpp") if p.name != "host_launch.cpp")       # (host_launch.cpp is the base object launch.o)
    assert sorted(UNITS["capi"]) == capi and sorted(UNITS["launch"]) == launch


@pytest.mark.parametrize("san,runs", H.RUNS)
def test_all_families_on_one_context_under_sanitizers(tmp_path, san, runs):
    exe = H.build(tmp_path / "b", san, **UNITS)
    for seed, sched in runs:
        H.ok(H.run(exe, seed, sched=sched), "mixed_driver", seed)


def _mutated_csrc(tmp_path, name, old, new):
    src = (H.CSRC / name).read_text()
    assert src.count(old) == 1, old
    csrc = tmp_path / "pkg" / "csrc"                              # ../../include from csrc, as in the tree
    shutil.copytree(H.CSRC, csrc, ignore=shutil.ignore_patterns("*.o", "*.so"))
    (tmp_path / "include").mkdir()
    shutil.copy(ROOT / "include" / "plume_hip.h", tmp_path / "include" / "plume_hip.h")
    (csrc / name).write_text(src.replace(old, new))
    return csrc


@pytest.mark.parametrize("name", list(MUTANTS))
def test_the_mixed_driver_names_a_call_on_a_mutant(tmp_path, name):
    unit, old, new, says, own = MUTANTS[name]
    csrc = _mutated_csrc(tmp_path, unit, old, new)
    r = H.run(H.build(tmp_path / "b", "", **UNITS, csrc=csrc), 1)
    assert r.returncode == 2 and "mixed_driver: seed 1, call " in r.stderr and says in r.stderr and " after " in r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-1500:])
    if own is not None:                                              # what the old tests did not see: the family's own driver passes on the same mutant
        H.ok(H.run(H.build(tmp_path / "own", "", **own, csrc=csrc), 1), own["driver"], 1)
