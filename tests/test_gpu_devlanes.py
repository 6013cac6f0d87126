"""The field, scalar, group-law, recoding, SHA-256, half-GCD, hash-to-curve-map and nonce-loop unit tests on the GPU's own code: the lane bodies of tests/devsim/lane_ops.h built for gfx950
(tests/devgpu/devgpu.hip, one lane per element, the op a template parameter of the kernel) under the same checks as the host build (tests/_lane_cases.py) -- the
DEVICE branch of every product in plume_fe_mul.inc, the device forms of mad_i64 / sel32 / opaque_*, the GPU's doubles in plume_eis.h.  The reference is Python integers,
pow, hashlib and the oracles; never the host build of the header (one count below compares the two builds, and asserts nothing).
Every batch goes to the GPU in a seeded shuffled order (LC.Placed): no wavefront is all edge cases or all random ones.  Device code has no assertions, so the group-law
check also holds every returned point to the group law over Python integers.
The last two tests reach the wave-wide vote of the multi-scalar loop (msm_all_inf: __all) through the C ABI, with scalars of every length mixed inside each wavefront."""
import random

import numpy as np
import pytest

from oracle import plume_oracle as O
from tests import _devgpu as G
from tests import _devsim as D
from tests import _lane_cases as LC
from tests import _oracle_c as OC
from tests import _recover as R

pytestmark = pytest.mark.gpu


@pytest.fixture()
def B(request):
    """the GPU backend, its batches in a shuffled order seeded by the test's name"""
    return LC.Placed(G.GPU, sum(request.node.name.encode()))


def test_fe_arith(B):
    LC.check_fe_arith(B)


def test_products_at_their_operand_bounds_come_back_tight(B):
    LC.check_products_at_bounds(B)


def test_group_law_compositions_stay_tight_and_give_the_group_laws_points(B):
    LC.check_group_law_compositions(B, values=True)


def test_fe_inv_pow(B):
    LC.check_fe_inv_pow(B)


def test_inversion_by_divsteps_matches_fermat_and_python(B):
    LC.check_inversion_by_divsteps(B)


def test_sc_arith(B):
    LC.check_sc_arith(B)


def test_glv_and_booth(B):
    LC.check_glv_and_booth(B)


def test_eisenstein_digit_entries(B):
    LC.check_eisd_entries(B)


def test_sha256_generic(B):
    LC.check_sha256_generic(B)


def test_batch_sizes_around_a_wavefront():
    """1, 63, 64, 65 lanes and 4133 (65 workgroups, the last one ragged), in the caller's order"""
    LC.check_counts(G.GPU)


def test_one_wavefront_of_64_different_edge_pairs():
    LC.check_one_wave_of_edge_pairs(G.GPU)


def test_eis_half_gcd_on_the_gpus_doubles(B):
    """the host test's 20 000 challenges: the relation, tau != 0, ok and the 66-bit bound for every item, whatever quotients the GPU's fma / division / rint estimate.
    The pairs need not be the host build's (g++ with -ffp-contract=off): how many differ is printed, not asserted.  Measured on an MI355X (ROCm 7.2): see LABNOTES.md,
    "Unit tests on the device branch"."""
    pairs = LC.check_eis_half_gcd(B)
    host = D.eis_half_gcd(LC.half_gcd_cases())
    differ = sum(1 for a, b in zip(pairs, host) if a != b)
    print(f"\nhalf-GCD pairs that differ between the gfx950 build and the host build: {differ} of {len(host)}")


def test_eis_pair_is_checked_before_it_is_used(B):
    LC.check_eis_pair_is_checked(B)


# ------------------------------------------------------------------------------------------------------- the map behind hash_to_curve, the nonce's retry loop
# Through the C ABI u0 and u1 are SHA-256 outputs and the modulus is n: the tangent and identity branches of the addition on E', SSWU's tv2 == 0 exception and the retry
# loop's body run here only.  Every check asserts, from the reference and the order the GPU gets, that each full wavefront mixes these lanes with ordinary ones
# (tests/_lane_cases.py) before it compares anything; batches are shuffled inside their 64-lane groups.
def test_sswu_on_chosen_field_elements(B):
    LC.check_sswu(B)


def test_addition_on_the_isogenous_curve_takes_its_tangent_and_identity_branches(B):
    LC.check_eprime_add(B)


def test_isogeny_on_fractions(B):
    LC.check_iso3(B)


def test_map2_on_chosen_pairs_and_the_two_role_form(B):
    """also 1, 63, 64, 65 and 4133 lanes through map2_to_curve_jac"""
    LC.check_map2(B)


def test_forty_eight_byte_reduction_at_the_multiples_of_p(B):
    LC.check_be48(B)


def test_nonce_retry_loop_keeps_every_lanes_k_while_other_lanes_retry(B):
    """the loop runs while ANY lane of the wavefront needs a candidate (__any): with q = 2^255 + 1 half of all candidates are rejected, with q = 2^256 - 2^250 about one
    lane of 64 retries while the others must keep their k; 4133 lanes per instantiation, and 1, 63, 64, 65"""
    LC.check_nonce_retries(B)


# ------------------------------------------------------------------------------------------------------- wavefronts that mix scalar lengths, through the C ABI
_NITEMS = 192          # three wavefronts


def _top_position(k):
    """where a chain over k's Eisenstein digits leaves the identity: the bit length of the longer GLV half"""
    k1, k2 = LC.glv_split(k)
    return max(abs(k1).bit_length(), abs(k2).bit_length())


def _mixed_items(seed):
    """192 items whose c and s are drawn independently from the scalars where a length or a carry changes (plus random ones), so that the two chains of neighbouring lanes
    leave the identity at different positions; pk among G, -G, 2G and random points.  plume_recover_batch admits c, s in [1, n-1] (tests/_recover.py): the smallest
    admitted value, 1, stands in for c = 0."""
    rng = random.Random(seed)
    n, lam = O.N, LC.LAM
    special = [1, 2, 3] + [pow(2, k, n) for k in (16, 64, 127, 128, 129, 192, 255)] + [lam, lam + 1, n - lam, n - 1, n - 2, (n - 1) // 2, (n + 1) // 2]

    def draw():
        return rng.choice(special) if rng.random() < 0.75 else rng.randrange(1, n)
    mul_g = lambda k: OC.point_mul(k.to_bytes(32, "big"), R.G_BYTES)  # noqa: E731  (64-byte records)
    fixed = [R.G_BYTES, O.pt_bytes(O.pt_neg(O.G)), mul_g(2)]
    cs, ss, pks, nuls, msgs = [], [], [], [], []
    for i in range(_NITEMS):
        while True:
            c, s = draw(), draw()
            if i % 8 == 0:
                c = 1
            top = (max(_top_position(s), _top_position(c)))
            if not cs or top != max(_top_position(ss[-1]), _top_position(cs[-1])):
                break
        cs.append(c); ss.append(s)
        pks.append((fixed + [mul_g(rng.randrange(1, n))])[rng.randrange(4)])
        nuls.append(mul_g(rng.randrange(1, n)))
        msgs.append(bytes(rng.getrandbits(8) for _ in range(rng.randrange(0, 40))))
    assert all(1 <= x < n for x in cs + ss) and {1, n - 1, lam} <= set(cs) | set(ss)
    return dict(c=cs, s=ss, pk=pks, nul=nuls, msgs=msgs)


def _arrays(items, order):
    col = lambda vals, w: np.frombuffer(b"".join(vals), dtype=np.uint8).reshape(-1, w).copy()  # noqa: E731
    mb, off = OC.pack_msgs([items["msgs"][i] for i in order])
    return dict(msgs=mb, off=off, pk=col([items["pk"][i] for i in order], 64), nullifier=col([items["nul"][i] for i in order], 64),
                c=col([items["c"][i].to_bytes(32, "big") for i in order], 32), s=col([items["s"][i].to_bytes(32, "big") for i in order], 32))


@pytest.fixture(scope="module")
def eng():
    """a context of its own: it has run no large verify"""
    import zk_nullifier_sig_amd as plume
    e = plume.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def mixed():
    items = _mixed_items(20261017)
    ident = list(range(_NITEMS))
    v = _arrays(items, ident)
    want = {ver: R.recover_batch(ver, v["msgs"], v["off"], v["pk"], v["nullifier"], v["c"], v["s"], nthreads=16) for ver in (1, 2)}
    return items, v, want


_KEYS = ("r_point", "hashed_to_curve_r", "hashed_to_curve", "status")


@pytest.mark.parametrize("ver", [1, 2])
def test_wavefronts_that_mix_scalar_lengths_recover_the_oracles_points(eng, mixed, ver):
    """r_point = s G - c pk and hashed_to_curve_r = s H - c nullifier of 192 items, byte for byte the definition's (tests/_recover.py: the oracles' point arithmetic)"""
    _, v, want = mixed
    got = eng.recover_batch(ver, v["msgs"], v["off"], v["pk"], v["nullifier"], v["c"], v["s"])
    assert (want[ver]["status"] != R.INVALID).all()
    for k in _KEYS:
        assert np.array_equal(np.asarray(got[k]).reshape(_NITEMS, -1), want[ver][k].reshape(_NITEMS, -1)), k


@pytest.mark.parametrize("ver", [1, 2])
def test_an_items_result_does_not_depend_on_its_neighbours(eng, mixed, ver):
    """the same 192 items in another seeded order: every item's records are the ones the definition gives it, wherever in a wavefront it sits"""
    items, _, want = mixed
    order = list(range(_NITEMS))
    random.Random(77).shuffle(order)
    assert sum(1 for k, i in enumerate(order) if i // 64 != k // 64) > 64
    v = _arrays(items, order)
    got = eng.recover_batch(ver, v["msgs"], v["off"], v["pk"], v["nullifier"], v["c"], v["s"])
    for k in _KEYS:
        assert np.array_equal(np.asarray(got[k]).reshape(_NITEMS, -1), want[ver][k].reshape(_NITEMS, -1)[order]), k
