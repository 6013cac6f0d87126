"""Case generators and checks of the field, scalar, group-law, recoding, SHA-256, half-GCD, hash-to-curve-map and nonce-loop unit tests, as functions of a BACKEND: a
tests/_devsim.Lanes -- the host build of tests/devsim/lane_ops.h (tests/test_devsim.py) or its gfx950 build (tests/test_gpu_devlanes.py).  The reference in every check
is Python integers, pow, hashlib, hmac (tests/_rfc6979.py) and oracle.plume_oracle -- never the other build of the header."""
import functools
import hashlib
import random
import re
from collections import namedtuple
from pathlib import Path

from oracle import plume_oracle as O
from tests import _devsim
from tests import _rfc6979 as RF

ROOT = Path(__file__).resolve().parent.parent
P, N = O.P, O.N
PC = 2**32 + 977
LAM = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE
EDGE_FE = [0, 1, 2, PC - 1, PC, PC + 1, P - 2, P - 1, P, P + 1, P + PC - 1, 2**256 - PC, 2**256 - PC + 1, 2**256 - 2, 2**256 - 1,
           2**255, 2**128, 2**128 - 1, (1 << 224) - 1, 0xFFFFFFFF, 0xFFFFFFFF00000000, int("f" * 56 + "0" * 8, 16)]
T, T8 = 2**29 + 2**19, 2**24 + 2**10                              # plume_field.h "tight": limbs 0..7, limb 8
BIG = int(((2**64 - 2**50) // 9) ** 0.5) - 1                      # both operands of a product at the square root of its column bound (~1.33 * 2^30)
P_LIMBS = [0x1FFFFC2F, 0x1FFFFFF7] + [0x1FFFFFFF] * 6 + [0x00FFFFFF]


def val(L):
    return sum(x << (29 * i) for i, x in enumerate(L))


def tight(L):
    return all(x <= T for x in L[:8]) and L[8] <= T8


def fe_cases(rng, nrand=300):
    vals = list(EDGE_FE) + [rng.randrange(2**256) for _ in range(nrand)] + [rng.randrange(P) for _ in range(nrand)]
    a, b = [], []
    for x in EDGE_FE:
        for y in EDGE_FE:
            a.append(x); b.append(y)
    for _ in range(nrand * 2):
        a.append(rng.choice(vals)); b.append(rng.choice(vals))
    return a, b


class Placed:
    """A backend whose batches are NOT sorted into uniform wavefronts: every call's elements go to the backend in a seeded random order (edge cases and random cases
    interleaved, another order per call) and come back in the caller's.  On the GPU an element's position is its lane."""

    def __init__(self, backend, seed):
        self._b, self._rng = backend, random.Random(seed)

    def _perm(self, n):
        perm = list(range(n))
        self._rng.shuffle(perm)
        return perm

    def _perm_in_groups(self, n, group=64):
        """shuffled inside every run of 64 elements: what shares a wavefront in the caller's order still does, in other lanes"""
        perm = []
        for g0 in range(0, n, group):
            blk = list(range(g0, min(n, g0 + group)))
            self._rng.shuffle(blk)
            perm += blk
        return perm

    def _run(self, fn, cols, fixed=(), perm=None, placed=None):
        n = len(cols[0])
        perm = self._perm(n) if perm is None else perm
        if placed is not None:
            placed(perm)                                   # the order the backend gets: the coverage conditions of a check are asserted on THIS order
        out = fn(*fixed, *[None if c is None else [c[i] for i in perm] for c in cols])
        back = [None] * n
        for k, i in enumerate(perm):
            back[i] = out[k]
        return back

    def fe_op(self, op, a, b=None):
        return self._run(self._b.fe_op, [a, b], (op,))

    def fe_raw(self, op, a, b=None, c=None, e=None):
        return self._run(self._b.fe_raw, [a, b, c, e], (op,))

    def group_raw(self, op, px, py, pz, qx, qy):
        return self._run(self._b.group_raw, [px, py, pz, qx, qy], (op,))

    def sc_op(self, op, a, b=None):
        return self._run(self._b.sc_op, [a, b], (op,))

    def glv(self, ks):
        return self._run(self._b.glv, [ks])

    def eis_half_gcd(self, cs):
        return self._run(self._b.eis_half_gcd, [cs])

    def eis_consistent(self, cs, which=0):
        return self._run(lambda c: list(self._b.eis_consistent(c, which)), [cs])

    def h2c_op(self, op, *cols, placed=None):
        return self._run(self._b.h2c_op, list(cols), (op,), self._perm_in_groups(len(cols[0])), placed)

    def rfc6979(self, cap, q, x, h1, aux=None, placed=None):
        return self._run(self._b.rfc6979, [q, x, h1, aux], (cap,), self._perm_in_groups(len(q)), placed)

    def sha256(self, data):
        return self._b.sha256(data)

    def eisd_entries(self):
        return self._b.eisd_entries()


# ------------------------------------------------------------------------------------------------------------------------------- field
def check_fe_arith(B):
    rng = random.Random(1)
    a, b = fe_cases(rng)
    for op, fn in [(0, lambda x, y: x * y), (2, lambda x, y: x + y), (3, lambda x, y: x - y)]:
        got = B.fe_op(op, a, b)
        for x, y, g in zip(a, b, got):
            assert g < 2**256 and g % P == fn(x, y) % P, (op, hex(x), hex(y), hex(g))
    got = B.fe_op(1, a)
    assert all(g % P == x * x % P for x, g in zip(a, got))
    got = B.fe_op(4, a)
    assert all(g % P == (-x) % P for x, g in zip(a, got))
    got = B.fe_op(7, a)
    assert all(g == x % P for x, g in zip(a, got))
    ks = [1, 2, 3, 4, 8, 11, 1771, 65535, 2**20 - 1]
    for k in ks:
        got = B.fe_op(8, a, [k] * len(a))
        assert all(g % P == x * k % P for x, g in zip(a, got)), k
    assert [g for g in B.fe_op(9, a)] == [int(x % P == 0) for x in a]
    assert [g for g in B.fe_op(10, a, b)] == [int((x - y) % P == 0) for x, y in zip(a, b)]
    assert [g for g in B.fe_op(11, a)] == [(x % P) & 1 for x in a]
    # round 3: products with a subtraction riding in their fold (plume_fe_mul.inc fe_mul_sub / fe_sqr_sub / fe_sqr_sub2) and the doubling's two-product Y'
    for op, fn in [(16, lambda x, y: x * y - x), (17, lambda x, y: x * x - 2 * y - x), (18, lambda x, y: x * x - 2 * y), (19, lambda x, y: x * (y - x) - 2 * y * y),
                   (20, lambda x, y: (x - y) * (x + y) - y)]:
        got = B.fe_op(op, a, b)
        for x, y, g in zip(a, b, got):
            assert g == fn(x, y) % P, (op, hex(x), hex(y), hex(g))
    # the lazy forms and the word round trip (canonical out)
    for op, fn in [(12, lambda x, y: (x + y) * (x - y)), (13, lambda x, y: (x - 2 * y) ** 2), (14, lambda x, y: x)]:
        got = B.fe_op(op, a, b)
        for x, y, g in zip(a, b, got):
            assert g == fn(x, y) % P, (op, hex(x), hex(y), hex(g))
    # fe_mul_small with the LITERAL constants of the product's call sites (the compiler sees the constant: the strength-reduction miscompile of x * 11 was of this kind)
    for op, fn in [(21, lambda x: 3 * x), (22, lambda x: 11 * x), (23, lambda x: 1771 * x), (24, lambda x: -11 * x)]:
        got = B.fe_op(op, a)
        for x, g in zip(a, got):
            assert g == fn(x) % P, (op, hex(x), hex(g))
    got = B.fe_op(25, a, b)                                                # hash_to_field's 512-bit value: lo + hi 2^256
    for x, y, g in zip(a, b, got):
        assert g == (x + (y << 256)) % P, (hex(x), hex(y), hex(g))
    got = B.fe_op(26, a, b)                                                # fe_cmov, the flag another one in every lane
    for x, y, g in zip(a, b, got):
        assert g == (y if x & 1 else x) % P, (hex(x), hex(y), hex(g))
    assert any(x & 1 for x in a) and not all(x & 1 for x in a)
    assert B.fe_op(27, a) == [int(x < P) for x in a]


def check_products_at_bounds(B):
    """Round 4: the product's top columns run first (gen_fe_mul.py), so the excess over 2^256 is folded into limbs 0..2 before they are formed and limb 8 takes a
    remainder at the end.  Drive the column sums to the contract's bounds (plume_field.h: tight = limbs <= 2^29 + 2^19, limb 8 <= 2^24 + 2^10; multiplication inputs up
    to 9 * max(a) * max(b) < 2^64 - 2^50 with limb 8 <= 2^26) and check value and tightness of every form; the host build asserts the intermediate bounds."""
    rng = random.Random(44)
    big = BIG
    shapes = [([T] * 8 + [2**24 + 2**10], [T] * 8 + [2**24 + 2**10]), ([big] * 8 + [2**26], [big] * 8 + [2**26]), ([2**31 - 1] * 8 + [2**26], [T] * 8 + [2**26]),
              ([0] * 9, [big] * 8 + [2**26]), ([big] * 8 + [0], [0] * 8 + [2**26])]
    for _ in range(200):
        m = rng.choice([T, big, 2**29 - 1])
        shapes.append(([rng.randrange(m + 1) for _ in range(8)] + [rng.randrange(2**26 + 1)], [rng.randrange(m + 1) for _ in range(8)] + [rng.randrange(2**26 + 1)]))
    a, b = [s[0] for s in shapes], [s[1] for s in shapes]
    for got, x, y in zip(B.fe_raw(0, a, b), a, b):
        assert tight(got) and val(got) % P == val(x) * val(y) % P
    sq = [x for x in a if max(x[:8]) <= big]
    for got, x in zip(B.fe_raw(1, sq), sq):
        assert tight(got) and val(got) % P == val(x) ** 2 % P
    # tight operands for the scaled squarings; subtrahends up to 2p / 4p limbwise for the fused forms
    ta = [x for x in a if tight(x)] + [[rng.randrange(T + 1) for _ in range(8)] + [rng.randrange(2**24 + 2**10 + 1)] for _ in range(100)]
    for op, f in [(6, 3), (7, 2)]:
        for got, x in zip(B.fe_raw(op, ta), ta):
            assert tight(got) and val(got) % P == f * val(x) ** 2 % P
    p_l = P_LIMBS
    sub2 = [[rng.choice([0, 2 * q, rng.randrange(2 * q + 1)]) for q in p_l] for _ in a]
    sub4 = [[rng.choice([0, 4 * q, rng.randrange(4 * q + 1)]) for q in p_l] for _ in a]
    for got, x, y, s in zip(B.fe_raw(3, a, b, sub2), a, b, sub2):
        assert tight(got) and val(got) % P == (val(x) * val(y) - val(s)) % P
    for got, x, s in zip(B.fe_raw(4, sq, None, sub4[:len(sq)]), sq, sub4):
        assert tight(got) and val(got) % P == (val(x) ** 2 - val(s)) % P
    for got, x, s in zip(B.fe_raw(5, sq, None, sub2[:len(sq)]), sq, sub2):
        assert tight(got) and val(got) % P == (val(x) ** 2 - 2 * val(s)) % P
    # two products, one fold: the doubling's Y' at its bound (E * (D - X') + (-B) * 2B: 2^29 * 3 * 2^29 + 2^30 * 2^30 per column term)
    e1, e2, e3, e4 = [T] * 8 + [2**24], [3 * 2**29 + 2**19] * 8 + [2**26], [2**30 - 2000] * 8 + [2**25], [2**30 + 2**20] * 8 + [2**25]
    qa = [e1] + [[rng.randrange(v + 1) for v in e1] for _ in range(100)]
    qb = [e2] + [[rng.randrange(v + 1) for v in e2] for _ in range(100)]
    qc = [e3] + [[rng.randrange(v + 1) for v in e3] for _ in range(100)]
    qe = [e4] + [[rng.randrange(v + 1) for v in e4] for _ in range(100)]
    for got, x, y, z, w in zip(B.fe_raw(2, qa, qb, qc, qe), qa, qb, qc, qe):
        assert tight(got) and val(got) % P == (val(x) * val(y) + val(z) * val(w)) % P
    # the squarings that hand back the doubled operand (the doubling's Z' = (2Y) Z): the square as above, the double limb for limb.  Operands as the group law's: tight
    # (a doubled limb must fit 32 bits), the ends of the range first
    for op, f in [(8, 1), (9, 2)]:
        for got, x in zip(B.fe_raw(op, ta), ta):
            assert tight(got[:9]) and val(got[:9]) % P == f * val(x) ** 2 % P, op
            assert got[9:] == [2 * v for v in x], op
    # a constant operand held in scalar registers: beta (the table passes) and the largest limbs a canonical constant can have
    for op, k in [(10, BETA), (11, 2**256 - 1)]:
        for got, x in zip(B.fe_raw(op, a), a):
            assert tight(got) and val(got) % P == k * val(x) % P, op
    # the aliasing forms: "r may alias a or b" (plume_fe_mul.inc) -- on the device that is a matter of the asm statements' constraints
    for got, x, y in zip(B.fe_raw(12, a, b), a, b):
        assert tight(got) and val(got) % P == val(x) * val(y) % P                                  # fe_mul(x, x, y)
    for got, x, y in zip(B.fe_raw(13, a, b), a, b):
        assert tight(got) and val(got) % P == val(x) * val(y) % P                                  # fe_mul(y, x, y)
    for got, x in zip(B.fe_raw(14, sq), sq):
        assert tight(got) and val(got) % P == val(x) ** 2 % P                                      # fe_mul(x, x, x)
    for got, x in zip(B.fe_raw(15, sq), sq):
        assert tight(got) and val(got) % P == val(x) ** 2 % P                                      # fe_sqr(x, x)
    tb = [y for x, y in zip(a, b) if tight(x)] + [[rng.randrange(BIG + 1) for _ in range(8)] + [rng.randrange(2**26 + 1)] for _ in range(100)]
    assert len(tb) == len(ta)
    for got, x, y in zip(B.fe_raw(16, ta, tb), ta, tb):                                            # fe_mul_sub<2>(x, x, y, x): the subtrahend (tight: <= 2p limbwise) is the result too
        assert tight(got) and val(got) % P == (val(x) * val(y) - val(x)) % P
    ha = [x for x, y in zip(a, b) if 2 * max(x[:8]) * max(y[:8]) < (2**64 - 2**50) // 9]          # fe_muladd(x, x, y, x, y) = 2xy: both products in one column sum
    hb = [y for x, y in zip(a, b) if 2 * max(x[:8]) * max(y[:8]) < (2**64 - 2**50) // 9]
    ha += [[T] * 8 + [2**26]]; hb += [[T] * 8 + [2**26]]
    assert len(ha) > 100
    for got, x, y in zip(B.fe_raw(17, ha, hb), ha, hb):
        assert tight(got) and val(got) % P == 2 * val(x) * val(y) % P


# ------------------------------------------------------------------------------------------------------------------------------- group law
def group_law(op, X, Y, Z, qx, qy):
    """The formula sequences of plume_ec.h over Python integers mod p -- (X', Y', Z') of jac_dbl (0), jac_dbl_neg (1), jac_madd<false> (2), jac_madd<true> (3),
    jac_madd<false> with the row's y negated (4), jac_add with q = (qx, qy, Z) (5).  Polynomial identities in the five inputs: the inputs need not be curve points.
    Where a checked addition meets H = 0 it doubles (r = 0 too) or sets the identity flag and leaves the coordinates as they were."""
    def dbl(neg):
        E, Bv = 3 * X * X, 2 * Y * Y
        D = X * 2 * Bv
        Xn = E * E - 2 * D
        Yn = E * (Xn - D) + Bv * 2 * Bv if neg else E * (D - Xn) - Bv * 2 * Bv
        return Xn % P, Yn % P, 2 * Y * Z % P
    if op in (0, 1):
        return dbl(op == 1)
    if op == 4:
        qy = -qy
    z1z1 = Z * Z
    if op == 5:
        u1, s1, zz = X * z1z1, Z * z1z1 * Y, Z * Z
    else:
        u1, s1, zz = X, Y, Z
    h = qx * z1z1 - u1
    r = Z * z1z1 * qy - s1
    if op in (3, 5) and h % P == 0:
        return dbl(False) if r % P == 0 else (X % P, Y % P, Z % P)
    hh, hhh = h * h, h * h * h
    v = u1 * hh
    Xn = r * r - 2 * v - hhh
    return Xn % P, (r * (v - Xn) - s1 * hhh) % P, zz * h % P


def _check_group_values(op, rows, X, Y, Z, qx, qy):
    for k, row in enumerate(rows):
        got = (val(row[0:9]) % P, val(row[9:18]) % P, val(row[18:27]) % P)
        want = group_law(op, val(X[k]), val(Y[k]), val(Z[k]), val(qx[k]), val(qy[k]))
        assert got == want, (op, k)
        if want[2]:                                       # the point the coordinates stand for: X / Z^2, Y / Z^3
            zi, wi = pow(got[2], -1, P), pow(want[2], -1, P)
            assert (got[0] * zi * zi % P, got[1] * zi**3 % P) == (want[0] * wi * wi % P, want[1] * wi**3 % P), (op, k)


def check_group_law_compositions(B, values=True):
    """the product's limb-8 precondition (<= 2^26, since round 4's top-columns-first fold) is asserted in host builds only -- on whatever values a test happens to
    carry.  Here the group law's lazy sums and differences meet operands at the ENDS of the tight range (every limb 0 or its maximum, 2^29 + 2^19 and 2^24 + 2^10 on top, in
    every combination that matters plus random ones): each fe_mul / fe_sqr / fe_muladd inside jac_dbl, jac_dbl_neg, jac_madd (row y negated or not) and jac_add is checked by
    fe_mul_inputs_ok (the process aborts on a violation), and what comes back must be tight again, so that the operations compose.
    values: every returned point is also held against the group law over Python integers (group_law) -- device code has no assertions, there the VALUE does the policing."""
    rng = random.Random(99)
    hi, lo = [T] * 8 + [T8], [0] * 9

    def pick():
        r = rng.random()
        if r < 0.3:
            return list(hi)
        if r < 0.45:
            return list(lo)
        if r < 0.8:
            return [rng.choice([0, T]) for _ in range(8)] + [rng.choice([0, T8])]
        return [rng.randrange(T + 1) for _ in range(8)] + [rng.randrange(T8 + 1)]
    n = 600
    ops = [[pick() for _ in range(n)] for _ in range(5)]
    for k in range(5):                                   # the all-maximum and the all-but-one-maximum combinations first
        for j in range(5):
            ops[j][k] = list(hi if j != k else lo)
    ops[0][5], ops[1][5], ops[2][5], ops[3][5], ops[4][5] = list(hi), list(hi), list(hi), list(hi), list(hi)
    for op in range(6):
        rows = B.group_raw(op, *ops)
        for row in rows:
            assert tight(row[0:9]) and tight(row[9:18]) and tight(row[18:27]), op
        if values:
            _check_group_values(op, rows, *ops)
    # ... and composed: the outputs of one operation are the inputs of the next, twelve deep, every order
    cur = [ops[0], ops[1], ops[2]]
    for step in range(12):
        op = rng.choice([0, 1, 2, 4, 5])
        out = B.group_raw(op, cur[0], cur[1], cur[2], ops[3], ops[4])
        if values:
            _check_group_values(op, out, cur[0], cur[1], cur[2], ops[3], ops[4])
        cur = [[r[0:9] for r in out], [r[9:18] for r in out], [r[18:27] for r in out]]
        assert all(tight(a) and tight(b) and tight(c) for a, b, c in zip(*cur)), (step, op)


def check_fe_inv_pow(B):
    rng = random.Random(2)
    a = [1, 2, P - 1, P + 1, 2**256 - 1, PC] + [rng.randrange(1, 2**256) for _ in range(40)]
    a = [x for x in a if x % P]
    assert [g % P for g in B.fe_op(5, a)] == [pow(x, P - 2, P) for x in a]
    assert [g % P for g in B.fe_op(6, a)] == [pow(x, (P - 3) // 4, P) for x in a]
    assert B.fe_op(5, [0, P])[0] % P == 0


def check_inversion_by_divsteps(B):
    """fe_inv (Bernstein-Yang divsteps, 20 x 30 steps) against pow(x, -1, p), and against the Fermat chain it replaced; 0 and p give 0"""
    rng = random.Random(2024)
    vals = [1, 2, 3, P - 1, P - 2, P + 1, 2**255, 2**256 - 1, 977, 2**32 + 977, 2**128, 2**30, 2**30 - 1, 2**60, (P + 1) // 2]
    vals += [rng.getrandbits(256) for _ in range(3000)] + [rng.getrandbits(k) | 1 for k in (1, 8, 29, 30, 31, 58, 60, 61, 200, 255) for _ in range(20)]
    vals = [v for v in vals if v % P]
    got = B.fe_op(15, vals)
    assert got == [pow(v % P, -1, P) for v in vals]
    assert [g % P for g in B.fe_op(5, vals)] == got
    assert B.fe_op(15, [0, P]) == [0, 0]


# ------------------------------------------------------------------------------------------------------------------------------- scalars, recoding, SHA-256
def check_sc_arith(B):
    rng = random.Random(3)
    edge = [0, 1, 2, N - 1, N - 2, (N - 1) // 2, 2**128, 2**255 % N, 2**256 - N]
    a = edge * len(edge) + [rng.randrange(N) for _ in range(300)]
    b = [y for y in edge for _ in edge] + [rng.randrange(N) for _ in range(300)]
    assert B.sc_op(0, a, b) == [x * y % N for x, y in zip(a, b)]
    assert B.sc_op(1, a, b) == [(x + y) % N for x, y in zip(a, b)]
    assert B.sc_op(2, a) == [(-x) % N for x in a]
    wide_lo = [rng.randrange(2**256) for _ in range(200)] + [2**256 - 1, 0, 2**256 - 1]
    wide_hi = [rng.randrange(2**256) for _ in range(200)] + [2**256 - 1, 2**256 - 1, 0]
    assert B.sc_op(3, wide_lo, wide_hi) == [(lo + (hi << 256)) % N for lo, hi in zip(wide_lo, wide_hi)]


GLV_G1 = 0x3086D221A7D46BCDE86C90E49284EB153DAA8A1471E8CA7FE893209A45DBB031
GLV_G2 = 0xE4437ED6010E88286F547FA90ABFE4C4221208AC9DF506C61571B4AE8AC47F71
GLV_A1, GLV_MB1, GLV_A2 = 0x3086D221A7D46BCDE86C90E49284EB15, 0xE4437ED6010E88286F547FA90ABFE4C3, 0x114CA50F7A8E2F3F657C1108D9D44CFD8


def glv_split(k):
    """(k1, k2) of plume_ec.h glv_split, as integers: k1 = k - c1 a1 - c2 a2, k2 = c1 (-b1) - c2 b2 with c_i = round(k g_i / 2^384)"""
    c1, c2 = (k * GLV_G1 + (1 << 383)) >> 384, (k * GLV_G2 + (1 << 383)) >> 384
    return k - c1 * GLV_A1 - c2 * GLV_A2, c1 * GLV_MB1 - c2 * GLV_A1


def check_glv_and_booth(B):
    rng = random.Random(4)
    lam = LAM
    ks = [0, 1, 2, N - 1, N - 2, lam, lam + 1, N - lam, (N - 1) // 2, (N + 1) // 2, 2**128, 2**128 - 1, 2**255 % N] + [rng.randrange(N) for _ in range(2000)]
    # round 4: the split is exact integer arithmetic on 29-bit limbs (plume_ec.h glv_split): k1 = k - c1 a1 - c2 a2, k2 = c1 (-b1) - c2 b2 with c_i = round(k g_i / 2^384)
    g1, g2 = GLV_G1, GLV_G2
    ks += [N - lam, 2**255, 2**256 % N, (1 << 174) - 1, 1 << 174, (1 << 174) + 1, (1 << 145) - 1, g1 % N, g2 % N] + [rng.randrange(N) for _ in range(6000)]
    nonzero = total = 0
    for k, (m1, n1, m2, n2, codes) in zip(ks, B.glv(ks)):
        assert m1 < 2**128 and m2 < 2**128
        k1 = -m1 if n1 else m1
        k2 = -m2 if n2 else m2
        assert (k1 + k2 * lam) % N == k
        assert (k1, k2) == glv_split(k), hex(k)
        # round 5: ONE Eisenstein digit per position (plume_ec.h eisd_store): k1 + k2 w = sum d_i 4^i, d_i in {0, units, associates of 1 - w, associates of 2}
        assert len(codes) == _devsim.NPOS and all(0 <= c <= 18 for c in codes)
        va = vb = 0
        for c in reversed(codes):
            da, db = _devsim.eis_digit(c)
            va, vb = 4 * va + da, 4 * vb + db
        assert (va, vb) == (k1, k2), hex(k)
        nonzero += sum(1 for c in codes[:64] if c)
        total += 64
    assert 0.92 < nonzero / total < 0.95                       # fifteen of the sixteen residues mod 4 are non-zero digits


def eisenstein_digit_table():
    """the 64-entry table behind eisd_entry (plume_ec.h), regenerated from its definition: for t = (ta, tb), |t| <= 4, the digit is the representative of t mod 4 among
    0, the units, the associates of theta = 1 - w and of 2 that leaves a carry (t - d) / 4 in {-1, 0, 1}^2; and the header carries exactly this table"""
    digits = {c: _devsim.eis_digit(c) for c in range(1, 19)}
    assert len(set(digits.values())) == 18 and all(max(abs(a), abs(b)) <= 2 for a, b in digits.values())
    assert {(a % 4, b % 4) for a, b in digits.values()} | {(0, 0)} == {(a, b) for a in range(4) for b in range(4)}      # a complete residue system of Z[w] / 4
    tab = []
    for idx in range(64):
        ca, cb, na, nb = (idx >> 2) & 3, idx & 3, (idx >> 4) & 1, (idx >> 5) & 1
        ta_s = [t for t in range(-4, 5) if t % 4 == ca and (t < 0) == bool(na)]
        tb_s = [t for t in range(-4, 5) if t % 4 == cb and (t < 0) == bool(nb)]
        if not ta_s or not tb_s:
            tab.append(0)
            continue
        if (ca, cb) == (0, 0):
            tab.append(0 | (2 << 5) | (2 << 8))
            continue
        best = None
        for code, d in digits.items():
            if (d[0] % 4, d[1] % 4) != (ca, cb):
                continue
            worst = max([abs((t - d[0]) // 4) for t in ta_s] + [abs((t - d[1]) // 4) for t in tb_s])
            if best is None or worst < best[0]:
                best = (worst, code, d)
        assert best and best[0] <= 1, idx
        tab.append(best[1] | ((best[2][0] + 2) << 5) | ((best[2][1] + 2) << 8))
    src = (ROOT / "zk-nullifier-sig_amd" / "csrc" / "plume_ec.h").read_text()
    body = src[src.index("static const uint16_t T[64] = {"):]
    body = body[:body.index("};")]
    assert [int(x, 16) for x in re.findall(r"0x[0-9A-Fa-f]{3}", body)] == tab
    return tab


def check_eisd_entries(B, tab=None):
    """... and the register-resident packing the kernels run (eisd_entry) is this table for every t the recoding can meet"""
    tab = tab or eisenstein_digit_table()
    out = B.eisd_entries()
    assert len(out) == 81
    k = 0
    for ta in range(-4, 5):
        for tb in range(-4, 5):
            idx = ((ta & 3) << 2) | (tb & 3) | (16 if ta < 0 else 0) | (32 if tb < 0 else 0)
            assert out[k] == (tab[idx], tab[idx]), (ta, tb)
            k += 1


def check_sha256_generic(B):
    for n in (0, 1, 3, 55, 56, 57, 63, 64, 65, 119, 120, 121, 198, 99, 500):
        d = bytes((i * 13 + n) & 0xFF for i in range(n))
        assert B.sha256(d) == hashlib.sha256(d).digest(), n


# ------------------------------------------------------------------------------------------------------------------------------- half-GCD in Z[w]
def eis_cases(rng, nrand):
    n = O.N
    a1, b1 = 0x3086D221A7D46BCDE86C90E49284EB15, 0xE4437ED6010E88286F547FA90ABFE4C3
    cs = [0, 1, 2, 3, n - 1, n - 2, LAM, LAM + 1, LAM * LAM % n, 2**128, 2**64, 2**64 + 1, 2**65, 2**96, 2**127, 2**192, (n - 1) // 2, (n + 1) // 2, a1, b1, n - a1, n - b1]
    cs += [(x + y * LAM) % n for x in (1, 2**63, 2**64, 2**65, 2**66, -2**64, 3 * 2**62) for y in (0, 1, -1, 2**63, 2**64, -2**65)]      # short on the gamma side already
    cs += [pow(rng.randrange(2, 2**70), -1, n) for _ in range(100)]                                                                       # tau short, upsilon = 1
    cs += [rng.randrange(1, 2**66) * pow(rng.randrange(1, 2**66), -1, n) % n for _ in range(100)]                                      # both short: the answer is (nearly) unique
    cs += [rng.getrandbits(k) % n for k in (8, 16, 32, 64, 96, 127, 129, 160, 200) for _ in range(10)]
    cs += [rng.randrange(1, n) for _ in range(nrand)]
    return [c % n for c in cs]


def half_gcd_cases():
    return eis_cases(random.Random(20261002), 20000)


def check_eis_half_gcd(B):
    """tau gamma = upsilon (mod pi) for every c -- i.e. (t0 + t1 lambda) c = u0 + u1 lambda (mod n) --, tau != 0, every coefficient below 2^67 (in fact <= 65 bits: the chain
    has seventeen 4-bit windows), no fallback; random and crafted challenges, c = 0 included (verify_non_zk admits it).  The quotients are double-precision estimates: the
    RELATION holds whatever they are, the BOUND (<= 66 bits: plume_eis.h's contract, thirty-four digit positions) is what this check holds the estimates to.
    Returns the pairs."""
    cs = half_gcd_cases()
    pairs = B.eis_half_gcd(cs)
    worst = 0
    for c, (tm1, t1, u0, u1, tau, ok) in zip(cs, pairs):
        t0 = tm1 + 1
        assert tau == (t0 + t1 * LAM) % O.N and tau != 0
        assert (tau * c - (u0 + u1 * LAM)) % O.N == 0, hex(c)
        assert ok, hex(c)
        worst = max(worst, abs(tm1), abs(t1), abs(u0), abs(u1))
    assert worst.bit_length() <= 66, worst.bit_length()
    return pairs


def check_eis_pair_is_checked(B):
    """the scalar stage re-derives tau c == upsilon (mod n) from the pair it is about to use (eis_consistent) and falls back to the long form when it does not hold: true for
    every honest pair, crafted challenges included; false after any single tamper -- a coefficient's bit, a sign, tau itself, the pair of a neighbouring challenge"""
    rng = random.Random(99)
    cs = eis_cases(rng, 4000)
    assert all(B.eis_consistent(cs))
    pairs = B.eis_half_gcd(cs)
    for which in (1, 2, 3, 4):
        got = list(B.eis_consistent(cs, which))
        for c, g, (_, _, _, u1, _, _) in zip(cs, got, pairs):
            if g:       # a tamper that changes nothing: the sign of a ZERO coefficient (upsilon = u0 for small c and for c near n); tau + 1 for c = 0 (both sides stay 0)
                assert (which == 2 and u1 == 0) or (which == 3 and c == 0), (which, hex(c))
        assert sum(got) < len(cs) // 20, (which, int(sum(got)))


# ------------------------------------------------------------------------------------------------------------------------------- lane placement
def check_counts(B, counts=(1, 63, 64, 65, 4096 + 37)):
    """batches of one lane, one short of a wavefront, a wavefront, one more, and many workgroups with a ragged last one: the same mix of edge and random operands at every
    count (cut or repeated to length), through a field product, the doubling's two-product form, a raw product, a scalar product and the recoding"""
    rng = random.Random(7)
    a0, b0 = fe_cases(rng, 40)
    mix = list(zip(a0, b0))
    rng.shuffle(mix)
    raw = [([T] * 8 + [T8], [T] * 8 + [T8]), ([BIG] * 8 + [2**26], [BIG] * 8 + [2**26]), ([0] * 9, [BIG] * 8 + [2**26])]
    raw += [([rng.randrange(BIG + 1) for _ in range(8)] + [rng.randrange(2**26 + 1)], [rng.randrange(BIG + 1) for _ in range(8)] + [rng.randrange(2**26 + 1)]) for _ in range(61)]
    for n in counts:
        a, b = [mix[i % len(mix)][0] for i in range(n)], [mix[i % len(mix)][1] for i in range(n)]
        assert B.fe_op(0, a, b) == [x * y % P for x, y in zip(a, b)], n
        assert B.fe_op(19, a, b) == [(x * (y - x) - 2 * y * y) % P for x, y in zip(a, b)], n
        ra, rb = [raw[(i * 7) % len(raw)][0] for i in range(n)], [raw[(i * 7) % len(raw)][1] for i in range(n)]
        for got, x, y in zip(B.fe_raw(0, ra, rb), ra, rb):
            assert tight(got) and val(got) % P == val(x) * val(y) % P, n
        sa, sb = [x % N for x in a], [y % N for y in b]
        assert B.sc_op(0, sa, sb) == [x * y % N for x, y in zip(sa, sb)], n
        for k, (m1, n1, m2, n2, _) in zip(sa, B.glv(sa)):
            assert ((-m1 if n1 else m1), (-m2 if n2 else m2)) == glv_split(k), n


def check_one_wave_of_edge_pairs(B):
    """ONE wavefront whose 64 lanes hold 64 different pairs of edge operands, the all-maximum pair in lane 0 and in lane 63 (tight maximum | the products' input maximum):
    a value that the compiler wrongly held wave-uniform (a scalar register where a vector register is due) shows as a wrong lane"""
    hi, lo = [T] * 8 + [T8], [0] * 9
    alt = [T, 0] * 4
    v = [hi, lo, [2**29 - 1] * 8 + [2**24 - 1], alt + [T8], alt[::-1] + [0], [0] * 8 + [2**26], [BIG] * 8 + [0], [BIG] * 8 + [2**26]]       # v[0]: tight maximum, v[7]: input maximum
    a, b = [v[i // 8] for i in range(64)], [v[i % 8] for i in range(64)]
    assert len({(tuple(x), tuple(y)) for x, y in zip(a, b)}) == 64 and a[0] == b[0] == hi and a[63] == b[63] == v[7]
    for op in (0, 12, 13):
        for got, x, y in zip(B.fe_raw(op, a, b), a, b):
            assert tight(got) and val(got) % P == val(x) * val(y) % P, op
    for op in (1, 14, 15):
        for got, x in zip(B.fe_raw(op, b), b):
            assert tight(got) and val(got) % P == val(x) ** 2 % P, op
    sub = [[2 * q if (i + k) % 3 == 0 else 0 if (i + k) % 3 == 1 else q for k, q in enumerate(P_LIMBS)] for i in range(64)]
    for got, x, y, s in zip(B.fe_raw(3, a, b, sub), a, b, sub):
        assert tight(got) and val(got) % P == (val(x) * val(y) - val(s)) % P
    for got, x in zip(B.fe_raw(10, a), a):
        assert tight(got) and val(got) % P == BETA * val(x) % P
    # the tight ends for the forms whose operands must be tight: eight vectors again, the maximum first and last
    t = [hi, lo, [2**29 - 1] * 8 + [2**24 - 1], alt + [T8], alt[::-1] + [0], [0] * 8 + [T8], [T] * 8 + [0], hi]
    ta, tb = [t[i // 8] for i in range(64)], [t[i % 8] for i in range(64)]
    for got, x, y in zip(B.fe_raw(2, ta, tb, tb, ta), ta, tb):
        assert tight(got) and val(got) % P == 2 * val(x) * val(y) % P
    for got, x, y in zip(B.fe_raw(17, ta, tb), ta, tb):
        assert tight(got) and val(got) % P == 2 * val(x) * val(y) % P
    for got, x, y in zip(B.fe_raw(16, ta, tb), ta, tb):
        assert tight(got) and val(got) % P == (val(x) * val(y) - val(x)) % P
    for op, f in [(8, 1), (9, 2)]:
        for got, x in zip(B.fe_raw(op, tb), tb):
            assert tight(got[:9]) and val(got[:9]) % P == f * val(x) ** 2 % P and got[9:] == [2 * w for w in x], op
    for op in range(6):                                   # p = (t_i, t_j, t_i), q = (t_j, t_i)
        rows = B.group_raw(op, ta, tb, ta, tb, ta)
        for row in rows:
            assert tight(row[0:9]) and tight(row[9:18]) and tight(row[18:27]), op
        _check_group_values(op, rows, ta, tb, ta, tb, ta)
    # canonical words: every pair of the field's edge values that a wavefront holds
    ea = [EDGE_FE[(5 * i) % len(EDGE_FE)] for i in range(64)]
    eb = [EDGE_FE[(7 * i + 3) % len(EDGE_FE)] for i in range(64)]
    ea[0] = eb[0] = ea[63] = eb[63] = 2**256 - 1
    assert B.fe_op(0, ea, eb) == [x * y % P for x, y in zip(ea, eb)]
    assert B.fe_op(15, ea) == [pow(x % P, -1, P) if x % P else 0 for x in ea]
    assert B.fe_op(26, ea, eb) == [(y if x & 1 else x) % P for x, y in zip(ea, eb)]
    assert B.fe_op(22, ea) == [11 * x % P for x in ea]


# ------------------------------------------------------------------------------------------------------------------------------- the map behind hash_to_curve
ISO_A, ISO_B, SSWU_Z = O.ISO_A, O.ISO_B, O.Z
SQRT11 = pow(11, (P + 1) // 4, P)                                 # plume_h2c.h fe_sqrt_neg_z
assert SQRT11 * SQRT11 % P == 11
U_EXC = (pow(SQRT11, -1, P), P - pow(SQRT11, -1, P))              # Z u^2 = -1: tv2 = tv1 (tv1 + 1) = 0 with u != 0
SswuRef = namedtuple("SswuRef", "pt tv1 tv2_zero gx1 is_sq flip")


def _inv(x):
    return pow(x, -1, P)


def on_eprime(pt):
    return (pt[1] * pt[1] - pt[0] ** 3 - ISO_A * pt[0] - ISO_B) % P == 0


def eprime_add(p, q):
    """affine addition on E': y^2 = x^3 + A' x + B' over Python integers; None is the identity"""
    if p is None or q is None:
        return q if p is None else p
    (x0, y0), (x1, y1) = p, q
    if x0 == x1:
        if (y0 + y1) % P == 0:
            return None
        lam = (3 * x0 * x0 + ISO_A) * _inv(2 * y0) % P
    else:
        lam = (y1 - y0) * _inv(x1 - x0) % P
    x3 = (lam * lam - x0 - x1) % P
    return x3, (lam * (x0 - x3) - y0) % P


def pair_kind(p, q):
    """which branch of eprime_add_frac the points take"""
    if p[0] != q[0]:
        return "chord"
    return "identity" if (p[1] + q[1]) % P == 0 else "tangent"


@functools.lru_cache(maxsize=None)
def sswu_ref(u):
    """the oracle's simplified SWU of u and what classifies it: tv1 = Z u^2, whether tv2 = tv1 (tv1 + 1) is zero, gx1 = g(x1), Euler's criterion on it, and whether the
    last step negates y (sgn0(u) != sgn0(y) before it; y before it from the oracle's sqrt_ratio)"""
    tv1 = SSWU_Z * u * u % P
    tv2 = (tv1 * tv1 + tv1) % P
    tv3 = ISO_B * (tv2 + 1) % P
    tv4 = ISO_A * (SSWU_Z if tv2 == 0 else -tv2) % P
    x1 = tv3 * _inv(tv4) % P
    gx1 = (x1 ** 3 + ISO_A * x1 + ISO_B) % P
    is_sq = pow(gx1, (P - 1) // 2, P) == 1
    _, y1 = O.sqrt_ratio_3mod4((tv3 ** 3 + ISO_A * tv3 * tv4 * tv4 + ISO_B * tv4 ** 3) % P, pow(tv4, 3, P))
    y_pre = y1 if is_sq else tv1 * u % P * y1 % P
    pt = O.map_to_curve_sswu(u)
    assert on_eprime(pt) and gx1 != 0 and pt[1] in (y_pre, P - y_pre)
    return SswuRef(pt, tv1, tv2 == 0, gx1, is_sq, (u & 1) != (y_pre & 1))


@functools.lru_cache(maxsize=None)
def map2_ref(u0, u1):
    """(iso(sswu(u0)) + iso(sswu(u1)) on secp256k1, the branch the sum on E' takes)"""
    p0, p1 = sswu_ref(u0).pt, sswu_ref(u1).pt
    return O.pt_add(O.iso_map(p0), O.iso_map(p1)), pair_kind(p0, p1)


def _full_waves(order, wave=64):
    return [order[w:w + wave] for w in range(0, len(order) - wave + 1, wave)]


def _scaled(rng, v):
    """v as a fraction with a random nonzero denominator"""
    s = rng.randrange(1, P)
    return v * s % P, s


def _jac_affine(X, Y, Z):
    zi = _inv(Z)
    return X * zi * zi % P, Y * zi ** 3 % P


def check_sswu(B, groups=8):
    """sswu_frac (op 0) and its intermediates against the oracle's map, every full wavefront holding a tv2 == 0 lane and lanes of both is_sq values"""
    rng = random.Random(61)
    edge = [0, 1, 2, P - 1, P - 2, U_EXC[0], U_EXC[1]]
    us = []
    for _ in range(groups):
        us += edge + [rng.randrange(P) for _ in range(64 - len(edge))]
    us += [rng.randrange(P) for _ in range(37)]                    # a ragged last wavefront
    ref = [sswu_ref(u) for u in us]
    assert {0, 1, 2, P - 1, P - 2, U_EXC[0], U_EXC[1]} <= set(us) and all(SSWU_Z * u * u % P == P - 1 for u in U_EXC)
    assert {u for u, r in zip(us, ref) if r.tv2_zero} == {0, U_EXC[0], U_EXC[1]}
    for sq in (False, True):
        for flip in (False, True):
            assert sum(1 for r in set(ref) if (r.is_sq, r.flip) == (sq, flip)) >= 20, (sq, flip)

    def placed(order):
        waves = _full_waves(order)
        assert len(waves) >= groups
        for w in waves:
            assert any(ref[i].tv2_zero for i in w) and {ref[i].is_sq for i in w} == {False, True}
    got = B.h2c_op(0, us, placed=placed)
    for u, r, ((xn, xd, y, tv1, root), is_sq) in zip(us, ref, got):
        assert xd != 0, hex(u)
        assert (xn * _inv(xd) % P, y) == r.pt, hex(u)
        assert tv1 == (-11 * u * u) % P == r.tv1, hex(u)
        assert is_sq == int(r.is_sq), hex(u)
        assert root * root % P == (r.gx1 if r.is_sq else SSWU_Z * r.gx1 % P), hex(u)


def _eprime_points(rng, count):
    return [sswu_ref(rng.randrange(P)).pt for _ in range(count)]


def check_eprime_add(B, groups=6):
    """eprime_add_frac (op 3) against the affine addition on E' over Python integers: equal points arrive as DIFFERENT fractions (independent random denominators), every
    full wavefront holds tangent, identity and chord lanes"""
    rng = random.Random(62)
    pts = _eprime_points(rng, 48)
    neg = lambda p: (p[0], (-p[1]) % P)  # noqa: E731
    pairs = []
    for g in range(groups):
        pairs += [(p, p) for p in rng.sample(pts, 5)] + [(p, neg(p)) for p in rng.sample(pts, 5)]
        pairs += [tuple(rng.sample(pts, 2)) for _ in range(10)]                                            # distinct points
        pairs += [(rng.choice(pts), rng.choice([neg, lambda p: p])(rng.choice(pts))) for _ in range(44)]   # random pairs, whatever they are
    pairs += [tuple(rng.sample(pts, 2)) for _ in range(29)]
    kinds = [pair_kind(p, q) for p, q in pairs]
    cols = [[], [], [], [], [], []]
    for p, q in pairs:
        a, b = _scaled(rng, p[0])
        c, d = _scaled(rng, q[0])
        for col, v in zip(cols, (a, b, p[1], c, d, q[1])):
            col.append(v)
    assert all(b != d for b, d in zip(cols[1], cols[4]))

    def placed(order):
        waves = _full_waves(order)
        assert len(waves) >= groups
        for w in waves:
            assert {kinds[i] for i in w} == {"tangent", "identity", "chord"}
    got = B.h2c_op(3, *cols, placed=placed)
    for (p, q), kind, ((xn, xd, yn, yd), flag) in zip(pairs, kinds, got):
        want = eprime_add(p, q)
        assert (want is None) == (kind == "identity")
        assert flag == int(want is not None), (kind, p, q)
        if want is not None:
            assert xd != 0 and yd != 0, (kind, p, q)
            assert (xn * _inv(xd) % P, yn * _inv(yd) % P) == want, (kind, p, q)


def check_iso3(B, count=300):
    """iso3_frac_to_jac with y affine (op 4) and y a fraction (op 5): the affine value of the Jacobian output is the oracle's iso_map, a point of secp256k1"""
    rng = random.Random(63)
    pts = _eprime_points(rng, count - 3) + [sswu_ref(u).pt for u in (0, U_EXC[0], U_EXC[1])]
    fx = [_scaled(rng, p[0]) for p in pts]
    fy = [_scaled(rng, p[1]) for p in pts]
    xn, xd, yn, yd = [f[0] for f in fx], [f[1] for f in fx], [f[0] for f in fy], [f[1] for f in fy]
    for got in (B.h2c_op(4, xn, xd, [p[1] for p in pts]), B.h2c_op(5, xn, xd, yn, yd)):
        for p, ((X, Y, Z), inf) in zip(pts, got):
            assert inf == 0 and Z != 0, p
            q = _jac_affine(X, Y, Z)
            assert q == O.iso_map(p) and O.is_on_curve(q), p


def map2_pairs(groups):
    """pairs (u0, u1) in 64-lane groups that each hold the pairs the chord cannot take -- (u, u), (u, -u), (0, 0), and the u whose tv2 is zero among themselves: 0 and
    +-1/sqrt(11) share ONE x on E', so (0, +-1/sqrt(11)) are a tangent and an identity pair of DIFFERENT u -- among random pairs"""
    rng = random.Random(64)
    e0, e1 = U_EXC
    pairs = []
    for _ in range(groups):
        us = [rng.randrange(P) for _ in range(3)] + [1, 2, P - 1]
        grp = [(u, u) for u in us[:4]] + [(u, P - u) for u in us[:4]] + [(0, 0), (0, e0), (0, e1), (e0, 0), (e0, e1), (e1, e0), (e0, e0), (e1, e1)]
        grp += [(rng.randrange(P), rng.randrange(P)) for _ in range(64 - len(grp))]
        pairs += grp
    return pairs


def check_map2(B, groups=6, counts=(1, 63, 64, 65, 4096 + 37)):
    """map2_to_curve_jac (op 1) against iso(sswu(u0)) + iso(sswu(u1)) of the oracle, inf exactly for the opposite pairs; the same Jacobian words from the two maps run
    apart and maps_to_curve_jac (op 2: the two-role ingest kernel's form); then op 1 at the batch sizes around a wavefront"""
    pairs = map2_pairs(groups)
    assert {(0, 0), (0, U_EXC[0]), (0, U_EXC[1]), (U_EXC[0], U_EXC[1])} <= set(pairs) and any(a == b for a, b in pairs) and any(a and a == P - b for a, b in pairs)
    assert {map2_ref(0, U_EXC[0])[1], map2_ref(0, U_EXC[1])[1]} == {"tangent", "identity"}

    def run(op, prs):
        ref = [map2_ref(*pr) for pr in prs]

        def placed(order):
            for w in _full_waves(order):
                assert {ref[i][1] for i in w} == {"tangent", "identity", "chord"}
        got = B.h2c_op(op, [pr[0] for pr in prs], [pr[1] for pr in prs], placed=placed)
        for pr, (want, kind), ((X, Y, Z), inf) in zip(prs, ref, got):
            assert (want is None) == (kind == "identity")
            assert inf == int(kind == "identity"), (op, kind, pr)
            if not inf:
                assert Z != 0 and _jac_affine(X, Y, Z) == want, (op, kind, pr)
        return got
    assert len(_full_waves(pairs)) == groups
    assert run(2, pairs) == run(1, pairs)
    for n in counts:
        run(1, [pairs[i % len(pairs)] for i in range(n)])


def check_be48(B):
    """fe_from_be48_words (op 6): OS2IP of 48 bytes mod p, at the multiples of p, the word boundaries and both ends"""
    rng = random.Random(65)
    top = (2**384 // P) * P
    vals = [0, 1, P - 1, P, P + 1, 2 * P, 2**256 - 1, 2**256, 2**256 + 1, 2**384 - 1, top - 1, top, top + 1]
    vals += [2**(32 * k) + d for k in range(1, 12) for d in (-1, 1)]
    vals += [rng.getrandbits(384) for _ in range(300)] + [rng.randrange(2**128) * P + rng.choice([-1, 0, 1]) for _ in range(40)]
    assert all(0 <= v < 2**384 for v in vals) and top + P >= 2**384
    got = B.h2c_op(6, vals)
    assert [g[0][0] for g in got] == [v % P for v in vals]


# ------------------------------------------------------------------------------------------------------------------------------- RFC 6979's retry loop
Q_N, Q_HALF, Q_64TH = N, 2**255 + 1, 2**256 - 2**250             # a retry with probability 2^-128 | about 1/2 | 1/64: about one lane of a wavefront
NONCE_LANES = 4096 + 37
NONCE_SEED = 6979


@functools.lru_cache(maxsize=None)
def nonce_reference():
    """seeded x, h1 and aux of NONCE_LANES lanes and tests/_rfc6979.py's (k, used) for every modulus, with and without aux: computed once per process, never changed"""
    rng = random.Random(NONCE_SEED)
    x = [rng.getrandbits(256) for _ in range(NONCE_LANES)]
    h1 = [rng.getrandbits(256) for _ in range(NONCE_LANES)]
    aux = [rng.getrandbits(256) for _ in range(NONCE_LANES)]
    edge_h = [0, 1, 2**255, Q_HALF - 1, Q_HALF, Q_HALF + 1, Q_64TH - 1, Q_64TH, Q_64TH + 1, N - 1, N, N + 1, 2**256 - 1]     # bits2octets: h1 around every modulus
    edge_x = [0, 1, 2**256 - 1]
    h1[3:3 + len(edge_h)] = edge_h
    x[20:20 + len(edge_x)] = edge_x
    b = lambda v: v.to_bytes(32, "big")  # noqa: E731
    ref = {(q, with_aux): [RF.rfc6979_k(q, b(xi), b(hi), b(ai) if with_aux else None) for xi, hi, ai in zip(x, h1, aux)]
           for q in (Q_N, Q_HALF, Q_64TH) for with_aux in (False, True)}
    return x, h1, aux, ref


def nonce_want(q, with_aux, cap, n=NONCE_LANES):
    """the reference under a cap: k = 0, used = 0 where the first `cap` candidates were all out of range"""
    return [(k, used) if used <= cap else (0, 0) for k, used in nonce_reference()[3][(q, with_aux)][:n]]


def check_nonce_retries(B, counts=(1, 63, 64, 65)):
    """rfc6979_k_core for three moduli x CAP 16 | 4 x aux off | on against tests/_rfc6979.py, k and used of every lane.  What the reference must show, per wavefront of
    the order the backend gets, before anything is compared: q = n: every lane 1; q = 2^255 + 1: at least three distinct counts in every full wavefront, and under CAP 4
    both an exhausted lane (0) and one that took the last candidate (4); q = 2^256 - 2^250: at least half the wavefronts with one to three retrying lanes among lanes
    that must keep their k"""
    x, h1, aux, _ = nonce_reference()
    for q in (Q_N, Q_HALF, Q_64TH):
        for with_aux in (False, True):
            for cap in (16, 4):
                for n in ((NONCE_LANES,) + tuple(counts) if q == Q_HALF else (NONCE_LANES,)):
                    want = nonce_want(q, with_aux, cap, n)

                    def placed(order):
                        waves = _full_waves(order)
                        assert len(waves) == n // 64
                        if q == Q_N:
                            assert all(used == 1 for _, used in want)
                        elif q == Q_HALF:
                            assert all(len({want[i][1] for i in w}) >= 3 for w in waves)
                            if cap == 4 and n == NONCE_LANES:
                                assert {0, 4} <= {used for _, used in want}
                        else:
                            few = sum(1 for w in waves if 1 <= sum(1 for i in w if want[i][1] != 1) <= 3)
                            assert 2 * few >= len(waves) > 0, (few, len(waves))
                    got = B.rfc6979(cap, [q] * n, x[:n], h1[:n], aux[:n] if with_aux else None, placed=placed)
                    assert all((k == 0) == (used == 0) and k < q and used <= cap for k, used in want)
                    bad = [i for i in range(n) if got[i] != want[i]]
                    assert not bad, (hex(q), with_aux, cap, n, bad[:8], [got[i] for i in bad[:3]], [want[i] for i in bad[:3]])
