"""plume_pbkdf2_sha512_batch* on the host side (csrc/plume_kdf_capi.hip) under the sanitizers, on the CPU (tests/_hostsim.py): the ABI's translation unit, the new kernels
as host loops (tests/hostsim/kdf_launch.cpp) and a driver (tests/hostsim/kdf_driver.cpp) that pins every output to vectors this test writes from the restatement
(tests/_kdf.py): the host form with chunks that cut the batch into 1, 2 and many pieces and on sub-ranges; the shared salt -- a whole-call input that was advanced, or a
secret one that was wiped behind the first piece and not uploaded again, gives wrong bytes --; the NULL salt; the device form on a caller stream, with unsound offsets
planted among sound ones; the stage lists with the slice count for 1, 256, 257 and 2048 iterations; plume_init_multi contexts over two and eight mock devices; every
argument error; decreasing offsets; every allocation of a call failing in turn; and after every call, failed ones included, no device allocation but the caller's own
holding eight bytes in a row of a password, a salt, an ist / ost midstate, a U or T, or an output.  A small iteration count but for one 2048 run.  ASan + UBSan and TSan,
lazy, random and eager schedulers: stand-alone programs, nothing is loaded into Python.  One mutant, KDF_MUTANT_SKIPS_WIPE -- the workspace left as it was behind the last
kernel --, must fail the driver."""
import struct

import numpy as np
import pytest

from tests import _hostsim as S
from tests import _kdf as D

UNITS = dict(driver="kdf_driver", capi=["plume_kdf_capi.hip"], launch=["kdf_launch.cpp"], oracle=False)
WIPE = "~StageWipe() { (void)hipMemsetAsync(ctx->kdfws.p, 0, ws, st); }"


@pytest.fixture(scope="module")
def vectors(tmp_path_factory):
    """37 seeded passwords of the planted lengths, their salts, and what the restatement says of every recorded call, once"""
    n, salt_len, iterations, dklen, n_long = 37, 21, 3, 40, 5
    buf, off = D.planted_passwords(n, 3700)
    salt = np.random.default_rng(3701).integers(0, 256, (n, salt_len), dtype=np.uint8)
    blob = struct.pack("<5IQ", n, salt_len, iterations, dklen, n_long, len(buf)) + off.tobytes() + buf.tobytes() + salt.tobytes()
    for flags, s, sl in ((0, salt, salt_len), (D.BIP39 | D.SHARED_SALT, salt[:1], salt_len), (D.BIP39, None, 0)):
        out, status = D.pbkdf2_batch(buf, off, len(buf), s, sl, iterations, dklen, flags)
        assert not status.any()
        blob += out.tobytes()
    blob += D.pbkdf2_batch(buf, off[:n_long + 1], len(buf), salt[:1], salt_len, 2048, 64, D.BIP39 | D.SHARED_SALT)[0].tobytes()
    bad = off.copy()
    bad[5] = bad[4] - 1                                    # item 4 runs backwards
    bad[20] = len(buf) + 3                                 # item 19 reaches past the buffer, item 20 runs backwards from there
    bad[37] = 2**40                                        # item 36 far past it
    out, status = D.pbkdf2_batch(buf, bad, len(buf), salt, salt_len, iterations, dklen, 0)
    assert list(np.flatnonzero(status)) == [4, 19, 20, 36] and not out[status != 0].any() and out[5].any()
    blob += bad.tobytes() + out.tobytes() + status.tobytes()
    p = tmp_path_factory.mktemp("kdf_vectors") / "vectors.bin"
    p.write_bytes(blob)
    return p


@pytest.mark.parametrize("san,runs", S.RUNS)
def test_kdf_host_side_under_sanitizers(tmp_path, vectors, san, runs):
    exe = S.build(tmp_path / "b", san, **UNITS)
    for seed, sched in runs:
        S.ok(S.run(exe, vectors, seed, sched=sched), "kdf_driver", seed)


def test_the_driver_fails_when_the_workspace_is_not_wiped(tmp_path, vectors):
    """mutant: built with -DKDF_MUTANT_SKIPS_WIPE the call leaves ctx->kdfws as the kernels left it; the midstates, U and T of the batch are then found in it"""
    src = (S.CSRC / "plume_kdf_capi.hip").read_text()
    assert src.count(WIPE) == 1
    pkg = tmp_path / "pkg" / "csrc"
    pkg.mkdir(parents=True)
    (tmp_path / "pkg" / "include").mkdir()
    (tmp_path / "pkg" / "include" / "plume_hip.h").write_text((S.ROOT / "include" / "plume_hip.h").read_text())
    (pkg / "plume_kdf_capi.hip").write_text(src.replace(WIPE, "\n#if defined(KDF_MUTANT_SKIPS_WIPE)\n        ~StageWipe() {}\n#else\n        " + WIPE + "\n#endif\n"))
    unit = {"plume_kdf_capi.hip": pkg / "plume_kdf_capi.hip"}
    r = S.run(S.build(tmp_path / "b", "", **UNITS, sources=unit, defs={"plume_kdf_capi.hip": ["-DKDF_MUTANT_SKIPS_WIPE"]}), vectors, 1)
    assert r.returncode != 0 and "kdf_driver:" in r.stderr and "g_words" in r.stderr, (r.stdout[-500:], r.stderr[-1000:])
    S.ok(S.run(S.build(tmp_path / "c", "", **UNITS, sources=unit), vectors, 1), "kdf_driver", 1)     # the same patched unit without the flag passes
