// Per-element bodies of the field, scalar, group-law, hash-to-curve-map and nonce unit tests -- TEST INFRASTRUCTURE ONLY (never linked into the product library).
// One set of bodies, two builds: tests/devsim/devsim.cpp loops over them on the host (g++, the plain-C branch of every product, PLUME_FE_CHECK's assertions), and
// tests/devgpu/devgpu.hip runs one lane per element on gfx950 (the inline-asm branch of every product, the device forms of mad_i64 / sel32 / opaque_*, the GPU's doubles).
// The OP is a template parameter everywhere: each op is compiled the way a production kernel sees it, with its constants visible -- never a runtime switch in a kernel.
// Every function takes pointers to ONE element's words.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <type_traits>

#include "plume_eis.h"        // -> plume_ec.h -> plume_field.h
#include "plume_sha256.h"
#include "plume_h2c.h"
#include "plume_nonce.h"      // -> plume_stages.h

namespace plume_lanes {
using namespace plume;

constexpr int kFeOps = 28, kFeRawOps = 18, kGroupRawOps = 6, kScOps = 4, kEisTampers = 5;
constexpr int kFeRawOutWords = 18;      // r, then the second output of the forms that have one (zeros otherwise)
constexpr int kH2cOps = 7;
constexpr int kH2cInWords = 48, kH2cOutWords = 49;      // six field elements in; six out (zeros where an op has fewer), then one word of flag

// host side: the runtime op number -> f(std::integral_constant<int, OP>); false if there is no such op
template <int N, class F>
inline bool dispatch(int op, F&& f) {
    if constexpr (N == 0) { (void)op; (void)f; return false; }
    else {
        if (op == N - 1) { f(std::integral_constant<int, N - 1>{}); return true; }
        return dispatch<N - 1>(op, f);
    }
}

// op: 0 mul, 1 sqr, 2 add, 3 sub, 4 neg, 5 inv, 6 pow_c1, 7 normalize, 8 mul_small(b[0]), 9 is_zero->out[0], 10 eq->out[0], 11 is_odd->out[0],
//     12 (a+b)*(a+2p-b) on unreduced operands, 13 (a+4p-2b)^2 through fe_carry, 14 words round trip, 15 inversion by divsteps,
//     16..20 the fused multiply-subtract forms of the group law (round 3): xy - x, x^2 - (2y + x), x^2 - 2y, x(y - x) - 2y^2, (x - y)(x + y) - y
//     21..24 fe_mul_small with the LITERAL constants of the product's call sites, in their shapes: 21 r = 3 x (plume_h2c.h: fe_mul_small(Ln, a2, 3)), 22 x = 11 x in place
//     (plume_h2c.h: tv1), 23 x = 1771 x in place (plume_h2c.h: tv3), 24 -(11 x): in place, then negated into another element (plume_stages.h: gx2_sqrt)
//     25 fe_from_words16(a | b) = a + b 2^256, 26 fe_cmov(a, b, a odd): the flag differs from lane to lane, 27 words_lt_p(a)->out[0]
// operands/outputs: 256-bit integers as 8 little-endian 32-bit words (outputs canonical)
template <int OP>
PLUME_HD void fe_op(const uint32_t* a, const uint32_t* b, uint32_t* out) {
    fe x, y, r = fe_zero();
    bool flag = false;
    fe_from_words(x, a);       // any 256-bit integer, also >= p
    fe_from_words(y, b);
    switch (OP) {
        case 0: fe_mul(r, x, y); break;
        case 1: fe_sqr(r, x); break;
        case 2: fe_add(r, x, y); break;
        case 3: fe_sub(r, x, y); break;
        case 4: fe_neg(r, x); break;
        case 5: fe_inv_fermat(r, x); break;
        case 6: fe_pow_c1(r, x); break;
        case 7: r = x; fe_normalize(r); break;
        case 8: fe_mul_small(r, x, b[0]); break;
        case 9: flag = fe_is_zero(x); break;
        case 10: flag = fe_eq(x, y); break;
        case 11: flag = fe_is_odd(x); break;
        case 12: { fe s, d; fe_add_lazy(s, x, y); fe_sub_lazy<2>(d, x, y); fe_mul(r, d, s); break; }          // (a+b)(a-b), both operands unreduced
        case 13: { fe t; fe_add_lazy(t, y, y); fe_sub_lazy<4>(t, x, t); fe_carry(t); fe_sqr(r, t); break; }  // (a-2b)^2
        case 14: r = x; break;
        case 15: fe_inv_gcd(r, x); break;
        case 16: fe_mul_sub<2>(r, x, y, x); break;                                                               // xy - x
        case 17: { fe hh; fe_dbl_lazy(hh, y); fe_add_lazy(hh, hh, x); fe_sqr_sub<4>(r, x, hh); break; }           // x^2 - (2y + x): the mixed addition's X3
        case 18: fe_sqr_sub2<2>(r, x, y); break;                                                                 // x^2 - 2y: the doubling's X'
        case 19: { fe t, nb, db; fe_sub_lazy<2>(t, y, x); fe_neg_lazy(nb, y); fe_dbl_lazy(db, y); fe_muladd(r, x, t, nb, db); break; }   // x(y - x) - 2y^2: the doubling's Y' at its operand bounds
        case 20: { fe d, sm; fe_add_lazy(sm, x, y); fe_sub_lazy<2>(d, x, y); fe_mul_sub<2>(r, d, sm, y); break; }  // (x - y)(x + y) - y, unreduced factors
        case 21: fe_mul_small(r, x, 3); break;
        case 22: fe_mul_small(x, x, 11); r = x; break;
        case 23: fe_mul_small(x, x, 1771); r = x; break;
        case 24: fe_mul_small(x, x, 11); fe_neg(r, x); break;
        case 25: { uint32_t t[16]; PLUME_UNROLL for (int k = 0; k < 8; k++) { t[k] = a[k]; t[8 + k] = b[k]; } fe_from_words16(r, t); break; }
        case 26: r = x; fe_cmov(r, y, (a[0] & 1u) != 0); break;
        case 27: flag = words_lt_p(a); break;
    }
    if ((OP >= 9 && OP <= 11) || OP == 27) { PLUME_UNROLL for (int k = 0; k < 8; k++) out[k] = k == 0 ? (uint32_t)flag : 0u; return; }
    fe_normalize(r);
    fe_to_words(out, r);
}

// the constants of fe_mul_k in the raw ops: beta (the endomorphism's, what the table passes multiply by) and the largest canonical limbs a constant can have (2^256 - 1)
PLUME_HD fe fe_all_ones() { return fe_set(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu); }

// The products on RAW limbs (9 words per operand, NOT canonical: whatever magnitudes the caller's contract allows) -> raw result limbs, so that a test can drive the
// column sums to their bounds and look at the tightness of what comes back.  op: 0 fe_mul(a, b), 1 fe_sqr(a), 2 fe_muladd(a, b, c, e), 3 fe_mul_sub<2>(a, b, c), 4 fe_sqr_sub<4>(a, c),
// 5 fe_sqr_sub2<2>(a, c), 6 fe_sqr3(a), 7 fe_sqr2(a), 8 fe_sqr_d(a) -> r | dbl, 9 fe_sqr2_d(a) -> r | dbl, 10 fe_mul_k(beta, a), 11 fe_mul_k(2^256 - 1 as limbs, a),
// the ALIASING forms ("r may alias a or b", plume_fe_mul.inc; on the device that rests on the asm constraints), x = a, y = b:
// 12 fe_mul(x, x, y), 13 fe_mul(y, x, y), 14 fe_mul(x, x, x), 15 fe_sqr(x, x), 16 fe_mul_sub<2>(x, x, y, x), 17 fe_muladd(x, x, y, x, y)
// out: 18 words
template <int OP>
PLUME_HD void fe_raw(const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* e, uint32_t* out) {
    fe x, y, z, w, r = fe_zero(), r2 = fe_zero();
    PLUME_UNROLL for (int k = 0; k < 9; k++) { x.v[k] = a[k]; y.v[k] = b[k]; z.v[k] = c[k]; w.v[k] = e[k]; }
    switch (OP) {
        case 0: fe_mul(r, x, y); break;
        case 1: fe_sqr(r, x); break;
        case 2: fe_muladd(r, x, y, z, w); break;
        case 3: fe_mul_sub<2>(r, x, y, z); break;
        case 4: fe_sqr_sub<4>(r, x, z); break;
        case 5: fe_sqr_sub2<2>(r, x, z); break;
        case 6: fe_sqr3(r, x); break;
        case 7: fe_sqr2(r, x); break;
        case 8: fe_sqr_d(r, r2, x); break;
        case 9: fe_sqr2_d(r, r2, x); break;
        case 10: fe_mul_k(r, fe_beta(), x); break;
        case 11: fe_mul_k(r, fe_all_ones(), x); break;
        case 12: fe_mul(x, x, y); r = x; break;
        case 13: fe_mul(y, x, y); r = y; break;
        case 14: fe_mul(x, x, x); r = x; break;
        case 15: fe_sqr(x, x); r = x; break;
        case 16: fe_mul_sub<2>(x, x, y, x); r = x; break;
        case 17: fe_muladd(x, x, y, x, y); r = x; break;
    }
    PLUME_UNROLL for (int k = 0; k < 9; k++) { out[k] = r.v[k]; out[9 + k] = r2.v[k]; }
}

// The group law on RAW limbs: every lazy sum / difference that feeds a product inside jac_dbl / jac_dbl_neg / jac_madd / jac_add, driven by operands whose limbs
// sit at the ends of the "tight" range -- the host build's PLUME_FE_CHECK assertions (fe_mul_inputs_ok: limbs 0..7 by the column bound, limb 8 <= 2^26) abort on a violation.
// op: 0 jac_dbl, 1 jac_dbl_neg, 2 jac_madd<false>, 3 jac_madd<true>, 4 the same with the row's y negated lazily (what a negative digit does), 5 jac_add (q = (qx, qy, p.z)).
// p = (x, y, z) and the affine (qx, qy): 9 words each; out: the resulting x, y, z (27 words).
template <int OP>
PLUME_HD void group_raw(const uint32_t* px, const uint32_t* py, const uint32_t* pz, const uint32_t* qx, const uint32_t* qy, uint32_t* out) {
    jac p; p.inf = 0;
    fe ax, ay;
    PLUME_UNROLL for (int k = 0; k < 9; k++) { p.x.v[k] = px[k]; p.y.v[k] = py[k]; p.z.v[k] = pz[k]; ax.v[k] = qx[k]; ay.v[k] = qy[k]; }
    switch (OP) {
        case 0: jac_dbl(p); break;
        case 1: jac_dbl_neg(p); break;
        case 2: jac_madd<false>(p, ax, ay); break;
        case 3: jac_madd<true>(p, ax, ay); break;
        case 4: { fe ny; fe_neg_lazy(ny, ay); jac_madd<false>(p, ax, ny); break; }
        case 5: { jac q; q.inf = 0; q.x = ax; q.y = ay; q.z = p.z; jac_add(p, q); break; }
    }
    PLUME_UNROLL for (int k = 0; k < 9; k++) { out[k] = p.x.v[k]; out[9 + k] = p.y.v[k]; out[18 + k] = p.z.v[k]; }
}

// op: 0 mul, 1 add, 2 neg, 3 reduce of 512-bit a|b (a low)
template <int OP>
PLUME_HD void sc_op(const uint32_t* a, const uint32_t* b, uint32_t* out) {
    sc x, y, r;
    PLUME_UNROLL for (int k = 0; k < 8; k++) { x.v[k] = a[k]; y.v[k] = b[k]; r.v[k] = 0; }
    if (OP == 0) sc_mul(r, x, y);
    else if (OP == 1) sc_add(r, x, y);
    else if (OP == 2) sc_neg(r, x);
    else { uint32_t t[16]; PLUME_UNROLL for (int k = 0; k < 8; k++) { t[k] = x.v[k]; t[8 + k] = y.v[k]; } sc_reduce_wide(r, t); }
    PLUME_UNROLL for (int k = 0; k < 8; k++) out[k] = r.v[k];
}

// k (8 limbs) -> m1[4], neg1, m2[4], neg2 (10 words) and the PLUME_NPOS Eisenstein digit codes of the pair (int8)
PLUME_HD void glv(const uint32_t* k, uint32_t* out, int8_t* digits) {
    sc x; PLUME_UNROLL for (int j = 0; j < 8; j++) x.v[j] = k[j];
    glv_half h1, h2;
    glv_split(h1, h2, x);
    PLUME_UNROLL for (int j = 0; j < 4; j++) { out[j] = h1.m[j]; out[5 + j] = h2.m[j]; }
    out[4] = h1.neg; out[9] = h2.neg;
    eisd_store_glv(digits, 1, h1, h2, false);
}

PLUME_HD void sha256(const uint8_t* data, uint32_t len, uint8_t* out) {
    uint32_t st[8];
    sha256_init(st);
    sha256_absorb_pad(st, 0u, len, [&](uint32_t pos) -> uint32_t { return data[pos]; });
    for (int i = 0; i < 8; i++) { out[4 * i] = (uint8_t)(st[i] >> 24); out[4 * i + 1] = (uint8_t)(st[i] >> 16); out[4 * i + 2] = (uint8_t)(st[i] >> 8); out[4 * i + 3] = (uint8_t)st[i]; }
}

PLUME_HD void sc_from_be_bytes(sc& r, const uint8_t* b) {      // a record at any address (caller arrays of the harness are byte arrays)
    alignas(16) uint8_t cb[32];
    for (int k = 0; k < 32; k++) cb[k] = b[k];
    sc_from_be_aligned(r, cb);
}
PLUME_HD sc sc_one() { sc one; PLUME_UNROLL for (int k = 0; k < 8; k++) one.v[k] = k == 0 ? 1u : 0u; return one; }

// the half-GCD in Z[w] (plume_eis.h) for one challenge c (32 bytes big-endian, canonical): out = t0 - 1, t1, u0, u1 as signed 128-bit little-endian integers (4 x 16 bytes),
// tau = t0 + t1 lambda mod n (32 bytes BE), okf = the bound flag
PLUME_HD void eis_half_gcd_lane(const uint8_t* c_be, uint8_t* out, uint8_t* tau_be, uint8_t* okf) {
    sc c; sc_from_be_bytes(c, c_be);
    eis_short e;
    glv_half g0, g1;
    glv_split(g0, g1, c);
    eis_half_gcd(e, g0, g1);
    const uint32_t negs[4] = {e.tneg[0], e.tneg[1], e.uneg[0], e.uneg[1]};
    for (int k = 0; k < 4; k++) {
        const uint32_t* mag = k == 0 ? e.t[0] : k == 1 ? e.t[1] : k == 2 ? e.u[0] : e.u[1];
        __int128 v = 0;
        for (int w = 2; w >= 0; w--) v = (v << 32) | mag[w];
        if (negs[k]) v = -v;
        for (int b = 0; b < 16; b++) out[16 * k + b] = (uint8_t)((unsigned __int128)v >> (8 * b));
    }
    alignas(16) uint8_t tb[32];
    sc_to_be_aligned(tb, e.tau);
    for (int k = 0; k < 32; k++) tau_be[k] = tb[k];
    *okf = e.ok ? 1 : 0;
}
// eis_consistent(half-GCD of c, c) for one challenge, and the same after one tamper of the pair: which = 0 none, 1 upsilon's first coefficient + 1, 2 upsilon's second
// coefficient's sign flipped, 3 tau + 1, 4 the pair of ANOTHER challenge (c + 1)
template <int WHICH>
PLUME_HD void eis_consistent_lane(const uint8_t* c_be, uint8_t* out) {
    sc c; sc_from_be_bytes(c, c_be);
    sc c_for_pair = c;
    if (WHICH == 4) { const sc one = sc_one(); sc_add(c_for_pair, c, one); }
    eis_short e;
    glv_half g0, g1;
    glv_split(g0, g1, c_for_pair);
    eis_half_gcd(e, g0, g1);
    if (WHICH == 1) e.u[0][0] ^= 1u;
    if (WHICH == 2) e.uneg[1] ^= 1u;
    if (WHICH == 3) { const sc one = sc_one(); sc_add(e.tau, e.tau, one); }
    *out = eis_consistent(e, c) ? 1 : 0;
}
// the digit table of eisd_store in its two forms (the 64-entry table, the register-resident packing the kernels run) for t = (ta, tb) in [-4, 4]^2, idx = 9 (ta + 4) + tb + 4
PLUME_HD void eisd_entries_lane(uint32_t idx, uint32_t* out) {
    const int ta = (int)(idx / 9u) - 4, tb = (int)(idx % 9u) - 4;
    out[0] = eisd_entry_table(ta, tb);
    out[1] = eisd_entry(ta, tb);
}

// The map behind hash_to_curve (plume_h2c.h) on CHOSEN field elements -- through the ABI u0 and u1 are SHA-256 outputs, so the branches that depend on them (the tangent
// and the identity of eprime_add_frac, SSWU's tv2 == 0 exception) are reached from here only.
// op: 0 sswu_frac(u, &extra) -> xn, xd, y, extra.tv1, extra.root | extra.is_sq
//     1 map2_to_curve_jac(u0, u1) -> X, Y, Z | inf (the raw Jacobian representative)
//     2 the same from two sswu_frac calls and maps_to_curve_jac, (a, b, y0) = map(u1), (c, d, y1) = map(u0) as its comment states -> X, Y, Z | inf
//     3 eprime_add_frac(a, b, y0, c, d, y1) -> xn, xd, yn, yd | the returned bool (zeros when false)
//     4 iso3_frac_to_jac(xn, xd, y) -> X, Y, Z | inf,  5 iso3_frac_to_jac(xn, xd, yn, &yd) -> X, Y, Z | inf
//     6 fe_from_be48_words on the first 12 words of in (big-endian, most significant first) -> the value
// in: six 256-bit integers as 8 little-endian words each (any value, also >= p); out: six canonical values, then the flag
template <int OP>
PLUME_HD void h2c_op(const uint32_t* in, uint32_t* out) {
    fe i0, i1, i2, i3, i4, i5;
    fe o0 = fe_zero(), o1 = fe_zero(), o2 = fe_zero(), o3 = fe_zero(), o4 = fe_zero(), o5 = fe_zero();
    uint32_t flag = 0;
    fe_from_words(i0, in); fe_from_words(i1, in + 8); fe_from_words(i2, in + 16); fe_from_words(i3, in + 24); fe_from_words(i4, in + 32); fe_from_words(i5, in + 40);
    if constexpr (OP == 0) {
        sswu_extra ex;
        sswu_frac(o0, o1, o2, i0, &ex);
        o3 = ex.tv1; o4 = ex.root; flag = ex.is_sq ? 1u : 0u;
    } else if constexpr (OP == 1 || OP == 2) {
        jac h;
        if constexpr (OP == 1) map2_to_curve_jac(h, i0, i1);
        else {
            fe a, b, y0, c, d, y1;
            sswu_frac(c, d, y1, i0);
            sswu_frac(a, b, y0, i1);
            maps_to_curve_jac(h, a, b, y0, c, d, y1);
        }
        o0 = h.x; o1 = h.y; o2 = h.z; flag = h.inf;
    } else if constexpr (OP == 3) {
        flag = eprime_add_frac(o0, o1, o2, o3, i0, i1, i2, i3, i4, i5) ? 1u : 0u;
        if (!flag) { o0 = fe_zero(); o1 = fe_zero(); o2 = fe_zero(); o3 = fe_zero(); }
    } else if constexpr (OP == 4 || OP == 5) {
        jac h;
        if constexpr (OP == 4) iso3_frac_to_jac(h, i0, i1, i2); else iso3_frac_to_jac(h, i0, i1, i2, &i3);
        o0 = h.x; o1 = h.y; o2 = h.z; flag = h.inf;
    } else {
        fe_from_be48_words(o0, in);
    }
    fe_normalize(o0); fe_normalize(o1); fe_normalize(o2); fe_normalize(o3); fe_normalize(o4); fe_normalize(o5);
    fe_to_words(out, o0); fe_to_words(out + 8, o1); fe_to_words(out + 16, o2); fe_to_words(out + 24, o3); fe_to_words(out + 32, o4); fe_to_words(out + 40, o5);
    out[48] = flag;
}

// RFC 6979's candidate loop (plume_nonce.h rfc6979_k_core) for ANY modulus q of 256 bits with its top bit set: with q = n a retry has probability 2^-128, with other
// moduli the loop body runs, and on the GPU it runs while any lane of the wavefront still needs a candidate (nonce_any), the lanes that have their k keeping it.
// q, x, h1, aux: 8 big-endian words each (aux is not read when AUX is off: on or off for the whole launch, as in sign_nonce); k: 8 big-endian words, *used: the count
template <int CAP, bool AUX>
PLUME_HD void rfc6979_lane(const uint32_t* q, const uint32_t* x, const uint32_t* h1, const uint32_t* aux, uint32_t* k, uint32_t* used) {
    uint32_t qw[8], xw[8], hw[8], aw[8], kw[8];
    PLUME_UNROLL for (int j = 0; j < 8; j++) { qw[j] = q[j]; xw[j] = x[j]; hw[j] = h1[j]; aw[j] = AUX ? aux[j] : x[j]; }
    *used = rfc6979_k_core<CAP, AUX>(kw, qw, xw, hw, aw);
    PLUME_UNROLL for (int j = 0; j < 8; j++) k[j] = kw[j];
}
// host side: (cap, aux) -> f(std::integral_constant<int, CAP>, std::bool_constant<AUX>); false for a cap that is not compiled
template <class F>
inline bool dispatch_nonce(int cap, int aux, F&& f) {
    if (cap == 16) { if (aux) f(std::integral_constant<int, 16>{}, std::true_type{}); else f(std::integral_constant<int, 16>{}, std::false_type{}); return true; }
    if (cap == 4) { if (aux) f(std::integral_constant<int, 4>{}, std::true_type{}); else f(std::integral_constant<int, 4>{}, std::false_type{}); return true; }
    return false;
}

}  // namespace plume_lanes
