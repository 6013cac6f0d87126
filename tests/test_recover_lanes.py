"""k_recover_finalize's lane body (zk-nullifier-sig_amd/csrc/plume_recover.h) on the host: tests/recover/recover_lanes.cpp compiled with g++ under AddressSanitizer +
UBSan and -Werror, against the restatement below (the definition in include/plume_hip.h: records in the three formats, the version's hash, status 0 / 1 / 3).  All three
formats x both versions x status 0 / 1 / 3 x identity and non-identity results x odd / even y x an identity H, pk, nullifier x every subset of NULL outputs x all sixteen
destination offsets from a 16-byte boundary (so the aligned 16-byte path, the byte + quad + byte path of every lead and the 33-byte records all run) x batch sizes that
end inside a quad; the bytes around every array stay at their pre-fill.
First of all the restatement the other recover tests share (tests/_recover.py) is checked here against the reference's vector and the golden sign records."""
import hashlib
import itertools
import json
import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import plume_oracle as O
from tests import _oracle_c as OC
from tests import _recover as R

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "zk-nullifier-sig_amd" / "csrc"
GOLD = json.loads((ROOT / "tests" / "golden" / "golden_batches.json").read_text())
KATS = json.loads((ROOT / "tests" / "golden" / "reference_kats.json").read_text())


# ------------------------------------------------------------------------------------------------ the restatement itself
def _vector(ver):
    v = KATS["plume_vector"]
    pt = lambda k: bytes.fromhex(v[k + "_x"]) + bytes.fromhex(v[k + "_y"])  # noqa: E731
    return dict(msg=v["msg_utf8"].encode(), pk=pt("pk"), nul=pt("nullifier"), c=bytes.fromhex(v[f"c_v{ver}"]), s=bytes.fromhex(v[f"s_v{ver}"]), r=pt("g_r"), hr=pt("h_r"), h=pt("h"))


@pytest.mark.parametrize("ver", [1, 2])
def test_restatement_reproduces_the_reference_vector(ver):
    v = _vector(ver)
    assert R.recover_item(ver, v["msg"], v["pk"], v["nul"], v["c"], v["s"]) == (v["r"], v["hr"], v["h"], R.MATCH)
    mb, off = OC.pack_msgs([v["msg"]])
    col = lambda b: np.frombuffer(b, np.uint8).reshape(1, -1).copy()  # noqa: E731
    got = R.recover_batch(ver, mb, off, col(v["pk"]), col(v["nul"]), col(v["c"]), col(v["s"]))
    assert (got["r_point"].tobytes(), got["hashed_to_curve_r"].tobytes(), got["hashed_to_curve"].tobytes(), int(got["status"][0])) == (v["r"], v["hr"], v["h"], R.MATCH)
    # the other version's hash does not match this version's c
    assert R.recover_item(3 - ver, v["msg"], v["pk"], v["nul"], v["c"], v["s"]) == (v["r"], v["hr"], v["h"], R.MISMATCH)


@pytest.mark.parametrize("ver", [1, 2])
def test_restatement_reproduces_the_golden_sign_records(ver):
    items = GOLD[f"sign_v{ver}"]
    mb, off = OC.pack_msgs([bytes.fromhex(it["msg"]) for it in items])
    got = R.recover_batch(ver, mb, off, OC.arr(items, "pk", 64), OC.arr(items, "nullifier", 64), OC.arr(items, "c", 32), OC.arr(items, "s", 32))
    assert np.array_equal(got["r_point"], OC.arr(items, "r_point", 64))
    assert np.array_equal(got["hashed_to_curve_r"], OC.arr(items, "hashed_to_curve_r", 64))
    assert np.array_equal(got["hashed_to_curve"], OC.arr(items, "h", 64))
    assert (got["status"] == R.MATCH).all()
    for it in items[:2]:                                             # the array form and the Python-only form are one definition
        b = lambda k: bytes.fromhex(it[k])  # noqa: E731
        assert R.recover_item(ver, b("msg"), b("pk"), b("nullifier"), b("c"), b("s")) == (b("r_point"), b("hashed_to_curve_r"), b("h"), R.MATCH)


def test_restatement_rejects_what_the_reference_types_cannot_hold():
    v = _vector(2)
    zero = (bytes(64), bytes(64), bytes(64), R.INVALID)
    n, p = O.N.to_bytes(32, "big"), O.P.to_bytes(32, "big")
    assert R.recover_item(2, v["msg"], v["pk"], v["nul"], bytes(32), v["s"]) == zero
    assert R.recover_item(2, v["msg"], v["pk"], v["nul"], v["c"], n) == zero
    assert R.recover_item(2, v["msg"], v["pk"][:63] + bytes([v["pk"][63] ^ 1]), v["nul"], v["c"], v["s"]) == zero
    assert R.recover_item(2, v["msg"], v["pk"], p + v["nul"][32:], v["c"], v["s"]) == zero
    r, hr, h, st = R.recover_item(2, v["msg"], bytes(64), v["nul"], v["c"], v["s"])          # an identity pk is a value: accepted, R = s G
    assert st == R.MISMATCH and r == OC.point_mul(v["s"], R.G_BYTES) and h == O.pt_bytes(O.hash_to_curve(v["msg"], None))
    assert np.array_equal(R.registers_of(np.frombuffer(v["r"], np.uint8))[0].view("<u8"),
                          [int.from_bytes(v["r"][24 - 8 * j + 32 * k:32 - 8 * j + 32 * k], "big") for k in range(2) for j in range(4)])
    assert R.sec1_of(np.frombuffer(v["r"], np.uint8))[0].tobytes() == OC.sec1_compress(v["r"]) and not R.sec1_of(np.zeros(64, np.uint8)).any()


# ------------------------------------------------------------------------------------------------ the lane body
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("recover_lanes") / "recover_lanes"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}",
                    str(ROOT / "tests" / "recover" / "recover_lanes.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True, timeout=600)
    return exe


def _enc(rec):
    return b"\x00" if rec == bytes(64) else bytes([2 + (rec[63] & 1)]) + rec[:32]


def _hash(ver, pk, h, nul, r, hr):
    pts = [R.G_BYTES, pk, h, nul, r, hr] if ver == 1 else [nul, r, hr]
    return (int.from_bytes(hashlib.sha256(b"".join(_enc(x) for x in pts)).digest(), "big") % O.N).to_bytes(32, "big")


def _items(rng, n, ver, kinds):
    """n items; item i is of kind kinds[i % len(kinds)] = (status, R identity, Hr identity, y parity, which of H / pk / nullifier is the identity)"""
    pt = lambda par: rng.integers(0, 255, 31, dtype=np.uint8).tobytes() + b"\x01" + rng.integers(0, 255, 31, dtype=np.uint8).tobytes() + bytes([(int(rng.integers(0, 128)) << 1) | par])  # noqa: E731
    out = []
    for i in range(n):
        status, rinf, hrinf, par, ident = kinds[i % len(kinds)]
        r, hr, h, pk, nul = (bytes(64) if rinf else pt(par)), (bytes(64) if hrinf else pt(1 - par)), pt(par), pt(par), pt(1 - par)
        if ident == 1:
            h = bytes(64)
        elif ident == 2:
            pk = bytes(64)
        elif ident == 3:
            nul = bytes(64)
        c = _hash(ver, pk, h, nul, r, hr)
        if status != 1:
            c = c[:7] + bytes([c[7] ^ 0x10]) + c[8:]
        out.append(dict(flag=1 if status == 3 else 0, pk=pk, nul=nul, c=c, r=r, hr=hr, h=h, status=status))
    return out


def expected(items, fmt):
    """the four caller arrays"""
    cols = [[], [], [], []]
    for it in items:
        dead = it["status"] == 3
        for k, key in enumerate(("r", "hr", "h")):
            rec = np.frombuffer(bytes(64) if dead else it[key], np.uint8)
            cols[k].append(R.as_format(rec.reshape(1, 64), fmt).tobytes())
        cols[3].append(bytes([it["status"]]))
    return [b"".join(c) for c in cols]


def _run(harness, tmp_path, items, ver, fmt, mis, present):
    n = len(items)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<5I", n, ver, fmt, mis, present) + b"".join(bytes([it["flag"]]) + it["pk"] + it["nul"] + it["c"] + it["r"] + it["hr"] + it["h"] for it in items))
    r = subprocess.run([str(harness), str(fin), str(fout)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "recover_lanes ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    got, want = fout.read_bytes(), expected(items, fmt)
    pos = 0
    for k in range(4):
        if not present & (1 << k):
            continue                                               # (the harness itself checked that nothing was written anywhere)
        seg = got[pos:pos + 64 + len(want[k])]
        pos += len(seg)
        assert seg[:32] == b"\xAA" * 32 and seg[-32:] == b"\xAA" * 32, f"output {k}: bytes outside the array were written"
        assert seg[32:-32] == want[k], f"output {k} (n={n}, version={ver}, format={fmt}, misalign={mis}, present={present:04b})"
    assert pos == len(got)


KINDS = [(st, ri, hi, par, 0) for st, ri, hi, par in itertools.product((0, 1, 3), (0, 1), (0, 1), (0, 1))] + [(st, 0, 0, 1, ident) for st in (0, 1) for ident in (1, 2, 3)]


def test_every_format_status_identity_parity_and_alignment(harness, tmp_path):
    rng = np.random.default_rng(7)
    for ver, fmt, mis in itertools.product((1, 2), (0, 1, 2), range(16)):
        _run(harness, tmp_path, _items(rng, len(KINDS), ver, KINDS), ver, fmt, mis, 0b1111)


def test_every_subset_of_null_outputs(harness, tmp_path):
    rng = np.random.default_rng(8)
    for fmt, present in itertools.product((0, 1, 2), range(1, 16)):
        _run(harness, tmp_path, _items(rng, len(KINDS), 1 + (present & 1), KINDS), 1 + (present & 1), fmt, (5 * present) & 15, present)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 7, 16, 17, 255])
def test_batch_sizes_that_end_inside_a_quad(harness, tmp_path, n):
    rng = np.random.default_rng(n)
    for fmt, mis in itertools.product((0, 1, 2), (0, 4, 9)):
        _run(harness, tmp_path, _items(rng, n, 2 - (n & 1), KINDS[n % 5:] + KINDS[:n % 5]), 2 - (n & 1), fmt, mis, 0b1111)
