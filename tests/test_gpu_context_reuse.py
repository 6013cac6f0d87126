"""No call's result may depend on what its context ran before.  The call families share one workspace per context (csrc/plume_capi_ctx.h: bases, jobflags, itemflags,
tab, tabscr, res, resinf, res2, redo, digs, eq1fall, eq1k, nonce, scstage, and the host forms' staging slots) and lay it out differently -- 3 or 4 table jobs per item,
2, or 1; digit rows of two heights; a redo list at 2 lo + k or at lo + k; two staging layouts in scstage.  Here sequences of ordinary calls of different families and
sizes run on one engine, and every output byte of every call is compared with the CPU restatements' answer for that call alone (tests/_reuse.py: the table, computed once
per module).  Sizes are 321 and 65 items: a stale tail then lies both inside the last wavefront and in whole wavefronts behind it, and the planted invalid items of the
two sizes sit at different positions, so a flag or status byte another call left behind is a wrong one.  plume_last_redo_tasks is read after every call whose context's
redo list is known: 0 behind a verify call (these inputs hold none of the crafted items of tests/test_gpu_round6.py), an error behind an ECDSA-family call."""
import itertools

import pytest

from tests import _reuse as U

pytestmark = pytest.mark.gpu

# (A, settings, B, settings): family pairs that between them meet on every shared buffer (what each pair shares is listed beside it)
STREAM_PAIRS = [
    ("verify_v1", {"eq1_short": 3}, "ecdsa_recover", {}),            # bases jobflags itemflags tab tabscr res resinf redo digs eq1k (u1) eq1fall: J = 4 against one job per item
    ("sign", {"selfcheck": 0}, "verify_v2", {}),                     # bases jobflags itemflags tab tabscr res resinf res2 pkaff: PLUME_SIGN_K = 2 against J = 3
    ("sign_rfc6979", {"selfcheck": 1}, "ecdsa_sign", {}),            # nonce, res, scstage in its two layouts (322 and 195 B / item), the checks' verify and recover stages
    ("hd", {}, "ecdsa_sign", {"selfcheck": 0}),                      # res resinf hdws
    ("verify_non_zk", {"eq1_short": 1}, "aggregate", {}),            # bases jobflags itemflags, as verify_ingest_h2c leaves them
    ("eth_tx_sender", {}, "recover", {}),                            # redo digs txstage, the ECDSA list against the verifier's
    ("eth_tx_sign", {"selfcheck": 1}, "eth_tx_sender", {}),          # txsign txstage scstage
    ("kdf", {}, "merkle", {}),                                       # buffers of their own (kdfws, mrksort): the workspace chain alone
    ("dedup", {}, "eth_address", {}),                                # dslots .. dblockcnt
    ("verify_sec1", {}, "sign_sec1", {}),                            # dec[0..3] preflags in front of the verifier's buffers; the signer's 33-byte outputs (host form)
]


@pytest.fixture(scope="module")
def table():
    return U.table()


@pytest.fixture(scope="module")
def streams():
    import torch
    dev = torch.device("cuda", 0)
    return torch.cuda.Stream(dev), torch.cuda.Stream(dev)


def _engine(kind="plain"):
    import zk_nullifier_sig_amd as plume
    e = plume.Engine([0, 0] if kind == "two shards" else 0)
    if kind == "in flight":
        e.set_in_flight(2)
    return e


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.close()


def _reset(e):
    e.set_sign_selfcheck(0); e.set_eq1_short(1); e.set_sign_uniform(1); e.set_stage_timing(False)


def test_every_family_after_every_other(eng, table, streams):
    _reset(eng)
    steps = []
    for a, b in itertools.combinations(table, 2):
        for x, y in ((a, b), (b, a)):
            steps += [U.Step(table[x][U.LARGE], True, streams[0]), U.Step(table[y][U.SMALL], True, streams[0])]
    assert U.run_steps(eng, steps) == 4 * len(table) * (len(table) - 1) // 2


def test_small_after_large_within_a_family(eng, table, streams):
    _reset(eng)
    steps = [U.Step(table[f][n], device, streams[1] if device else None) for f in table for device in (False, True) for n in (U.LARGE, U.SMALL, U.LARGE)]
    U.run_steps(eng, steps)


@pytest.mark.parametrize("kind", ["plain", "in flight", "two shards"])
def test_seeded_walk(table, streams, kind):
    """200 calls: entry, form, stream (two caller streams or the context's own), self-check, the form of equation 1, the signer's schedule and stage timing drawn before
    each.  A two-shard context has host forms only"""
    seed = {"plain": 20261, "in flight": 20262, "two shards": 20263}[kind]
    e = _engine(kind)
    try:
        steps = U.walk(table, seed, 200, streams=(None, streams[0], streams[1]), forms=(False,) if kind == "two shards" else (False, True))
        U.run_steps(e, steps, seed=seed, lanes=kind == "in flight")
    finally:
        e.close()


def test_two_streams_without_a_host_sync(eng, table, streams):
    """A on one caller stream and B on the other, back to back: nothing but the library's workspace chain orders B's use of the scratch behind A's.  One synchronise at
    the end, then both compared"""
    import torch
    _reset(eng)
    for a, sa, b, sb in STREAM_PAIRS:
        for (x, sx, y, sy) in ((a, sa, b, sb), (b, sb, a, sa)):
            ex, ey = table[x][U.LARGE], table[y][U.SMALL]
            for k, v in sx.items():
                getattr(eng, U.SETTERS[k])(v)
            px = ex.enqueue(eng, True, streams[0])
            for k, v in sy.items():
                getattr(eng, U.SETTERS[k])(v)
            py = ey.enqueue(eng, True, streams[1])
            torch.cuda.synchronize()
            gx, gy = px.collect(sync=False), py.collect(sync=False)
            assert not U.differences(ex, gx, True), (ex.name, "in front of", ey.name, U.describe(ex, gx, True))
            assert not U.differences(ey, gy, True), (ey.name, "behind", ex.name, U.describe(ey, gy, True))
    _reset(eng)


@pytest.fixture(scope="module")
def long_verify():
    """a V2 verify of 2^14 + 65 items: above msm_pair_max, the long multi-scalar kernel"""
    return U.fam_verify((1 << 14) + 65, 2)


def test_layout_switches(table, streams, long_verify):
    e = _engine()
    try:
        s = streams[0]
        v1 = {n: table["verify_v1"][n] for n in (U.LARGE, U.SMALL)}
        steps = [U.Step(v1[U.LARGE], True, s, {"eq1_short": 3}),                      # J = 4, k_verify_msm_s
                 U.Step(table["verify_v2"][U.SMALL], True, s),                        # J = 3, the pair kernel
                 U.Step(table["ecdsa_recover"][U.LARGE], True, s),                    # one job per item, digit rows of PLUME_NPOS, eq1k as u1, redo at lo + k
                 U.Step(v1[U.LARGE], True, s),
                 U.Step(v1[U.SMALL], False, None, {"eq1_short": 1}),                  # the long form again, through the staging slots
                 U.Step(long_verify, True, s),                                        # every buffer grows; k_verify_msm
                 U.Step(table["verify_v2"][U.SMALL], True, s),
                 U.Step(v1[U.SMALL], True, s, {"eq1_short": 3})]
        U.run_steps(e, steps)
        kernels = []
        for mode, entry in ((3, v1[U.LARGE]), (1, table["verify_v2"][U.SMALL]), (1, long_verify)):
            e.set_eq1_short(mode)
            assert not U.differences(entry, entry.run(e, True, s), True), entry.name
            kernels.append(e.last_msm_kernel())
        assert kernels == ["k_verify_msm_s", "k_verify_msm_pair", "k_verify_msm"]   # the three layouts were the ones the sequence is about
    finally:
        e.close()


def test_growth_between_calls(table, streams):
    """65, then 321 -- every buffer of the workspace is reallocated -- then 65, on a fresh engine per pair; the 321 call of family B is issued while family A's
    device-form result on the other stream has not been synchronised"""
    import torch
    for a, sa, b, sb in STREAM_PAIRS:
        e = _engine()
        try:
            for k, v in {**sa, **sb}.items():
                getattr(e, U.SETTERS[k])(v)
            ea, eb = table[a][U.SMALL], table[b][U.LARGE]
            pa = ea.enqueue(e, True, streams[0])
            pb = eb.enqueue(e, True, streams[1])
            torch.cuda.synchronize()
            ga, gb = pa.collect(sync=False), pb.collect(sync=False)
            assert not U.differences(ea, ga, True), (ea.name, "in front of a growing", eb.name, U.describe(ea, ga, True))
            assert not U.differences(eb, gb, True), (eb.name, "growing behind", ea.name, U.describe(eb, gb, True))
            U.run_steps(e, [U.Step(ea, True, streams[0]), U.Step(table[b][U.SMALL], True, streams[1]), U.Step(table[a][U.LARGE], False, None)], check_redo=False)
        finally:
            e.close()


def test_the_redo_hook_refuses_another_familys_list(eng, table, streams):
    """read directly: a count behind a verify, an error that says why behind an ECDSA recovery, a count again behind the next verify"""
    import zk_nullifier_sig_amd as plume
    _reset(eng)
    table["verify_v2"][U.SMALL].run(eng, True, streams[0])
    assert eng.last_redo_tasks() == 0
    table["ecdsa_recover"][U.SMALL].run(eng, True, streams[0])
    with pytest.raises(plume.PlumeHipError, match="another family"):
        eng.last_redo_tasks()
    table["kdf"][U.SMALL].run(eng, True, streams[0])
    with pytest.raises(plume.PlumeHipError, match="another family"):
        eng.last_redo_tasks()
    table["recover"][U.SMALL].run(eng, False, None)
    assert eng.last_redo_tasks() == 0
