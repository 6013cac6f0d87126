"""The runner of tests/_reuse.py against two fake engines that answer from the table's expected arrays: an honest one, which every sequence must pass, and one that
leaks -- past the current n rounded down to a wavefront (64 items) and in every status byte it hands back what the previous call wrote there.  The runner must name the
first leaking call.  No GPU: what is under test is the harness the GPU tests (tests/test_gpu_context_reuse.py) rely on.  The table is built on a few quick families."""
import numpy as np
import pytest

from tests import _reuse as U

FAMILIES = ("verify_v1", "verify_v2", "sign", "kdf", "dedup", "aggregate")


@pytest.fixture(scope="module")
def table():
    return U.table(FAMILIES)


class Honest:
    def __init__(self):
        self.calls = 0

    def answer(self, entry, device):
        self.calls += 1
        return {k: v.copy() for k, v in entry.want(device).items()}

    def set_sign_selfcheck(self, v): pass
    def set_eq1_short(self, v): pass
    def set_sign_uniform(self, v): pass
    def set_stage_timing(self, v): pass


class Leaky(Honest):
    """per-item arrays: the items from (n // 64) * 64 on hold the previous call's bytes where that call had such items; status arrays: every byte the previous call's"""

    def __init__(self):
        super().__init__()
        self.last = {}                                     # array position in the call's outputs -> what the previous call returned there

    def answer(self, entry, device):
        out = super().answer(entry, device)
        n, tail = entry.n, (entry.n // 64) * 64
        for slot, (k, a) in enumerate(out.items()):
            prev = self.last.get(slot)
            if prev is None or a.ndim == 0 or len(a) != n or prev.dtype != a.dtype or prev.shape[1:] != a.shape[1:]:
                continue
            lo = 0 if k in entry.status else tail
            hi = min(n, len(prev))
            if hi > lo:
                a[lo:hi] = prev[lo:hi]
        self.last = {slot: a.copy() for slot, (k, a) in enumerate(out.items())}
        return out


def _pairs(table):
    steps = []
    for a in table:
        for b in table:
            if a != b:
                steps += [U.Step(table[a][U.LARGE]), U.Step(table[b][U.SMALL])]
    return steps


def test_planted_positions_of_the_two_sizes_never_meet():
    big, small = set(U.bad_positions(U.LARGE).tolist()), set(U.bad_positions(U.SMALL).tolist())
    assert big and small and not big & small and min(small) < 64 == max(small) and max(big) == 320


def test_the_runner_passes_an_honest_engine(table):
    eng = Honest()
    steps = _pairs(table) + U.walk(table, 5, 300, streams=(None, "s0", "s1"))
    assert U.run_steps(eng, steps) == len(steps) == eng.calls


def test_the_runner_names_the_first_call_of_a_leaky_engine(table):
    """verify 321 then verify 65 of the other version: the small call's verdicts are the large call's -- the planted positions differ, so they are wrong"""
    steps = [U.Step(table["kdf"][U.SMALL]), U.Step(table["verify_v1"][U.LARGE]), U.Step(table["verify_v2"][U.SMALL], device=True), U.Step(table["sign"][U.SMALL])]
    with pytest.raises(U.Leak) as e:
        U.run_steps(Leaky(), steps, seed=77)
    assert e.value.index == 2 and e.value.step is steps[2] and e.value.previous is steps[1]
    msg = str(e.value)
    assert "seed 77" in msg and "call 2" in msg and "verify_v2[65] (device form" in msg and "after verify_v1[321] (host form" in msg and "ok:" in msg


def test_a_leak_in_the_last_wavefront_alone_is_seen(table):
    """sign 321 then sign 65 on an engine that leaks only past item 64: one item of one call differs"""
    class TailOnly(Leaky):
        def answer(self, entry, device):
            out = Honest.answer(self, entry, device)
            for slot, (k, a) in enumerate(out.items()):
                prev = self.last.get(slot)
                if prev is not None and len(a) == entry.n and prev.shape[1:] == a.shape[1:] and len(prev) > 64 and entry.n > 64:
                    a[64:entry.n] = prev[64:entry.n]
            self.last = {slot: a.copy() for slot, (k, a) in enumerate(out.items())}
            return out
    steps = [U.Step(table["sign"][U.LARGE]), U.Step(table["sign"][U.SMALL]), U.Step(table["sign"][U.LARGE])]
    with pytest.raises(U.Leak) as e:
        U.run_steps(TailOnly(), steps)
    assert e.value.index == 1


def test_every_leaky_pair_is_caught(table):
    """large then small of two different families, each pair on a leaky engine of its own: whenever the engine changed a byte the runner stops at the second call"""
    seen = 0
    for a in table:
        for b in table:
            if a == b:
                continue
            eng = Leaky()
            first = eng.answer(table[a][U.LARGE], False)
            second = eng.answer(table[b][U.SMALL], False)
            changed = bool(U.differences(table[b][U.SMALL], second, False))
            assert not U.differences(table[a][U.LARGE], first, False)
            eng2 = Leaky()
            steps = [U.Step(table[a][U.LARGE]), U.Step(table[b][U.SMALL])]
            if changed:
                seen += 1
                with pytest.raises(U.Leak) as e:
                    U.run_steps(eng2, steps)
                assert e.value.index == 1
            else:
                U.run_steps(eng2, steps)
    assert seen >= 6                                       # (families whose arrays have nothing in common leak nothing into each other here)


def test_the_redo_hook_is_checked_behind_verify_and_ecdsa_calls(table):
    class Counts(Honest):
        def __init__(self, count):
            super().__init__()
            self.count = count

        def last_redo_tasks(self):
            return self.count
    U.run_steps(Counts(0), [U.Step(table["verify_v1"][U.SMALL])])
    with pytest.raises(U.Leak, match="plume_last_redo_tasks gave 7"):
        U.run_steps(Counts(7), [U.Step(table["kdf"][U.SMALL]), U.Step(table["verify_v1"][U.SMALL])])
    fake = U.Entry("ecdsa_like", 1, None, {"x": np.zeros(1, np.uint8)}, None, redo=U.ECDSA)
    with pytest.raises(U.Leak, match="an error expected"):
        U.run_steps(Counts(0), [U.Step(fake)])
