// Public keys and Ethereum addresses from ECDSA signatures (plume_ecdsa_recover_batch, include/plume_hip.h): the semantics of Ethereum's ecrecover precompile with a one-byte
// v that may also be 0 or 1.  For item i, with z = hash mod n and R the curve point with x = r and y of v's parity,
//     Q = r^-1 (s R - z G) = u1 G + u2 R,   u1 = -z r^-1,  u2 = s r^-1  (mod n);      address = Keccak-256(Qx || Qy)[12..32)
// Four stages, one lane per item each (kernels in plume_ecdsa_kernels.hip):
//   ecdsa_prepare    validate v, r, s; decompress R (decompress_point, plume_stages.h); r^-1 by sc_inv below; u1 (kept as words for the comb), the Eisenstein digits of the
//                    GLV pair of u2 (eisd_store_glv), R as table job i, the item flag
//   (tables)         the existing table stage over n jobs: rows R, theta R, 2R by one batched inversion (launch_tables)
//   ecdsa_mul        u2 R along one joint slot of PLUME_NPOS positions (msm_runk_impl, the signer's runner with K = 1), then u1 G from the doubling-free comb
//                    (comb_add_g: fifteen additions) onto the same accumulator.  The hot form uses the unchecked additions; a lane whose chain met p == +-q (Z = 0 mod p,
//                    jac_madd) files its item, and a second, dense launch redoes the filed items with the checked additions -- the verifier's redo scheme (redo_file).
//                    Inputs that make u1 G = +-u2 R exist (R = k G, hash = -+s k): the final additions are exactly where they meet.
//   (to affine)      the existing batched conversion (normalize_points)
//   ecdsa_finalize   identity -> invalid; Keccak-256 (plume_keccak.h); compare with expect; WRITE the records (recover_store, plume_recover.h) and the status
//     status 3 (PLUME_ECDSA_INVALID)   v, r or s out of range (or s high under PLUME_ECDSA_LOW_S), no point with x = r, or Q is the identity: every record all zero
//     status 1 (PLUME_ECDSA_MATCH)     expect is NULL or equals the address
//     status 0 (PLUME_ECDSA_MISMATCH)  pk and address are written all the same
// Every value here is public: plain branches.
// sc_inv: inversion mod n by the same safegcd divsteps as fe_inv_gcd (plume_field.h: divsteps30 and update_fg30 are shared; the d/e update and the final normalisation are
// written here for the modulus n, whose 30-bit limbs are dense where p's are sparse -- the p path is untouched).  A Fermat ladder over sc_mul would be 256 squarings + ~128
// multiplications of the 8 x 32-bit carry-chain form, some 10^5 instructions per item; this is ~1.2 * 10^4.
// Compiles as plain C++ for the host (tests/ecdsa, tests/hostsim), like the other headers.
#pragma once
#include "plume_keccak.h"

#define PLUME_ECDSAK_MISMATCH 0u       // PLUME_ECDSA_* (include/plume_hip.h)
#define PLUME_ECDSAK_MATCH 1u
#define PLUME_ECDSAK_INVALID 3u
#define PLUME_ECDSAK_LOW_S 1           // flag bit 0: s > (n - 1) / 2 is invalid (EIP-2)

namespace plume {

// ------------------------------------------------------------------------------------------------ inversion mod n
// n as nine 30-bit limbs (non-negative), n^-1 mod 2^30
PLUME_HD constexpr int32_t s30_n(int i) {
    return i == 0 ? 0x10364141 : i == 1 ? 0x3F497A33 : i == 2 ? 0x348A03BB : i == 3 ? 0x2BB739AB : i == 4 ? 0x3FFFFEBA : i == 8 ? 0xFFFF : 0x3FFFFFFF;
}
#define PLUME_N_INV30 0x2A774EC1u
// (d, e) <- t * (d, e) / 2^30  (mod n), both kept in (-2n, n): update_de30 with n's limbs
PLUME_HD void update_de30_n(s30& d, s30& e, const trans30& t) {
    const int32_t sd = d.v[8] >> 31, se = e.v[8] >> 31;
    int32_t md = (t.u & sd) + (t.v & se), me = (t.q & sd) + (t.r & se);
    int64_t cd = mad_i64(mad_i64(0, t.u, d.v[0]), t.v, e.v[0]);
    int64_t ce = mad_i64(mad_i64(0, t.q, d.v[0]), t.r, e.v[0]);
    md -= (int32_t)((PLUME_N_INV30 * (uint32_t)cd + (uint32_t)md) & PLUME_M30);
    me -= (int32_t)((PLUME_N_INV30 * (uint32_t)ce + (uint32_t)me) & PLUME_M30);
    cd = mad_i64(cd, s30_n(0), md); ce = mad_i64(ce, s30_n(0), me);
    cd >>= 30; ce >>= 30;
    PLUME_UNROLL for (int i = 1; i < 9; i++) {
        const int32_t di = d.v[i], ei = e.v[i];
        cd = mad_i64(mad_i64(cd, t.u, di), t.v, ei);
        ce = mad_i64(mad_i64(ce, t.q, di), t.r, ei);
        cd = mad_i64(cd, s30_n(i), md); ce = mad_i64(ce, s30_n(i), me);
        d.v[i - 1] = (int32_t)cd & PLUME_M30; cd >>= 30;
        e.v[i - 1] = (int32_t)ce & PLUME_M30; ce >>= 30;
    }
    d.v[8] = (int32_t)cd; e.v[8] = (int32_t)ce;
}
// r in (-2n, n) -> [0, n), negated first when sign < 0: normalize30 with n's limbs
PLUME_HD void normalize30_n(s30& r, int32_t sign) {
    int32_t cond_add = r.v[8] >> 31;
    const int32_t cond_neg = sign >> 31;
    PLUME_UNROLL for (int i = 0; i < 9; i++) { r.v[i] += s30_n(i) & cond_add; r.v[i] = (r.v[i] ^ cond_neg) - cond_neg; }
    PLUME_UNROLL for (int i = 0; i < 8; i++) { r.v[i + 1] += r.v[i] >> 30; r.v[i] &= PLUME_M30; }
    cond_add = r.v[8] >> 31;
    PLUME_UNROLL for (int i = 0; i < 9; i++) r.v[i] += s30_n(i) & cond_add;
    PLUME_UNROLL for (int i = 0; i < 8; i++) { r.v[i + 1] += r.v[i] >> 30; r.v[i] &= PLUME_M30; }
}
// r = a^-1 mod n for canonical a (0 for a = 0); r canonical
PLUME_HD void sc_inv(sc& r, const sc& a) {
    s30 d, e, f, g;
    PLUME_UNROLL for (int i = 0; i < 9; i++) {
        const int bit = 30 * i, wi = bit >> 5, sh = bit & 31;
        uint32_t lo = a.v[wi] >> sh;
        if (sh > 2 && wi + 1 < 8) lo |= a.v[wi + 1] << (32 - sh);
        g.v[i] = (int32_t)(lo & PLUME_M30);
        f.v[i] = s30_n(i); d.v[i] = 0; e.v[i] = i == 0 ? 1 : 0;
    }
    int32_t zeta = -1;
    PLUME_NOUNROLL for (int it = 0; it < 20; it++) {
        trans30 t;
        zeta = divsteps30(zeta, (uint32_t)f.v[0], (uint32_t)g.v[0], t);
        update_de30_n(d, e, t);
        update_fg30(f, g, t);
    }
    normalize30_n(d, f.v[8]);                        // f = +-1 now (a = 0: d = 0)
    PLUME_UNROLL for (int k = 0; k < 8; k++) {
        const int bit = 32 * k, li = bit / 30, sh = bit - 30 * li;
        uint32_t v = (uint32_t)d.v[li] >> sh;
        const int have = 30 - sh;
        if (li + 1 < 9) v |= (uint32_t)d.v[li + 1] << have;
        r.v[k] = v;
    }
}

// ------------------------------------------------------------------------------------------------------ the stages
struct EcdsaArgs {
    int flags;                        // PLUME_ECDSAK_LOW_S
    int pk_format, addr_format;       // PLUME_ETHK_PK_*, PLUME_ETHK_ADDR_*
    uint32_t n;
    // the caller's arrays, at any byte offset
    const uint8_t *hash, *r, *s;      // 32 big-endian bytes per item
    const uint8_t* v;                 // 1 byte per item: 0, 1, 27 or 28
    const uint8_t* expect;            // 20 bytes per item, or NULL
    uint8_t* pk;                      // eth_pk_width(pk_format) bytes per item, or NULL
    uint8_t* address;                 // eth_address_width(addr_format) bytes per item, or NULL
    uint8_t* status;                  // 1 byte per item, or NULL
    // workspace
    uint32_t* bases;                  // n job records (st_base): R of item i, affine
    uint8_t* jobflags;                // n
    uint8_t* itemflags;               // n: non-zero = invalid at the prepare stage
    uint32_t* tab;                    // n window tables (R, theta R, 2R)
    int8_t* digs;                     // PLUME_NPOS x n digit codes of u2's GLV pair, row-major (row p of item i at digs[p * n + i])
    uint32_t* u1;                     // 8 x n words, word-major: u1 for the comb
    uint32_t* res;                    // Jacobian SoA over n results; affine X, Y behind the conversion stage
    uint8_t* resinf;                  // n
    uint32_t* redo;                   // redo[0] = number of items whose unchecked chain met p == +-q, redo[1 + k] = the k-th such item; zeroed by the prepare stage
    const uint32_t* gcomb;            // the doubling-free comb of G (PLUME_COMB_WORDS), shared with the signer
};

// (n - 1) / 2 as words
PLUME_HD uint32_t sc_half_n(int i) {
    return i == 0 ? 0x681B20A0u : i == 1 ? 0xDFE92F46u : i == 2 ? 0x57A4501Du : i == 3 ? 0x5D576E73u : i == 7 ? 0x7FFFFFFFu : 0xFFFFFFFFu;
}
PLUME_HD bool sc_is_high(const sc& a) {      // a > (n - 1) / 2
    uint32_t bw = 0;
    PLUME_UNROLL for (int i = 0; i < 8; i++) (void)subb(sc_half_n(i), a.v[i], bw);
    return bw != 0;
}
// v -> the parity of R's y; false: no recovery id
PLUME_HD bool ecdsa_parity(uint32_t& parity, uint32_t v) {
    if (v == 0u || v == 1u) { parity = v; return true; }
    if (v == 27u || v == 28u) { parity = v - 27u; return true; }
    parity = 0u;
    return false;
}
// the prepare stage of one item without its stores: false = invalid; else R (affine, canonical), u1 and u2
PLUME_HD bool ecdsa_prepare_values(fe& rx, fe& ry, sc& u1, sc& u2, int flags, const uint8_t* hash, const uint8_t* rb, const uint8_t* sb, uint32_t v) {
    uint32_t parity;
    sc r, s, z;
    sc_from_be(r, rb); sc_from_be(s, sb); sc_from_be(z, hash);
    bool ok = ecdsa_parity(parity, v);
    ok = ok && !sc_is_zero(r) && sc_lt_n(r) && !sc_is_zero(s) && sc_lt_n(s);
    if ((flags & PLUME_ECDSAK_LOW_S) && sc_is_high(s)) ok = false;
    if (!ok) return false;
    alignas(16) uint8_t in33[36], rec[64];
    in33[0] = (uint8_t)(2u + parity);
    PLUME_UNROLL for (int k = 0; k < 32; k++) in33[1 + k] = rb[k];
    if (!decompress_point(rec, in33)) return false;                                     // r < n < p: only "x^3 + 7 has no square root" fails here
    (void)reload_affine_be(rx, ry, rec);
    sc_cond_sub_n(z);                                                                   // any 32 bytes are a hash: z = hash mod n (hash < 2^256 < 2n)
    sc ri, t;
    sc_inv(ri, r);
    sc_mul(t, z, ri); sc_neg(u1, t);
    sc_mul(u2, s, ri);
    return true;
}
// lane i of k_ecdsa_prepare
PLUME_HD void ecdsa_prepare(const EcdsaArgs& a, uint32_t i) {
    fe rx, ry;
    sc u1, u2;
    const bool ok = ecdsa_prepare_values(rx, ry, u1, u2, a.flags, a.hash + 32 * (size_t)i, a.r + 32 * (size_t)i, a.s + 32 * (size_t)i, a.v[i]);
    a.itemflags[i] = (uint8_t)(ok ? 0u : 1u);
    jac p; p.inf = 0; p.z = fe_small(1);
    if (ok) { p.x = rx; p.y = ry; } else { p.x = fe_gx(); p.y = fe_gy(); }              // (an invalid item's job builds a dummy table, as everywhere else)
    st_base(a.bases, i, p);
    a.jobflags[i] = (uint8_t)((ok ? PLUME_JOB_OK : PLUME_JOB_INVALID) | PLUME_JOB_AFFINE);
    if (!ok) return;                                                                    // its digit rows and u1 are never read
    PLUME_UNROLL for (int w = 0; w < 8; w++) a.u1[(size_t)w * a.n + i] = u1.v[w];
    glv_half h1, h2;
    glv_split(h1, h2, u2);
    eisd_store_glv(a.digs + i, a.n, h1, h2, false);
}
// lane of k_ecdsa_mul (CHECKED = false: a chain that met p == +-q files its item and stores nothing) and of k_ecdsa_mul_redo (CHECKED = true).  dig: the lane's digit area
// (LDS on the device), element stride
template <bool CHECKED>
PLUME_HD void ecdsa_mul(const EcdsaArgs& a, uint32_t i, int8_t* dig, uint32_t stride) {
    jac acc;
    if (a.itemflags[i]) {
        acc.x = fe_small(1); acc.y = fe_small(1); acc.z = fe_small(0); acc.inf = 1;
    } else {
        const int8_t* d = a.digs + i;
        PLUME_UNROLL for (int p = 0; p < PLUME_NPOS; p++) dig[(uint32_t)p * stride] = d[(size_t)p * a.n];
        if (CHECKED) PLUME_COUNT_FALLBACK();
        msm_runk_impl<CHECKED, PLUME_NPOS, 1>(acc, a.tab + (size_t)i * PLUME_TAB_WORDS, 0, dig, stride);      // u2 R
        sc k;                                                                          // (loaded after the chain: eight registers the chain does not have to carry)
        PLUME_UNROLL for (int w = 0; w < 8; w++) k.v[w] = a.u1[(size_t)w * a.n + i];
        comb_add_g<CHECKED>(acc, k, a.gcomb);                                          // + u1 G
        if (!CHECKED && !acc.inf && fe_is_zero(acc.z)) { redo_file(a.redo, i); return; }
    }
    st_jac_soa(a.res, a.n, i, acc);
    a.resinf[i] = (uint8_t)acc.inf;
}

// the address record of the 20 address bytes ad (five memory-order words), as eth_address_item lays it out
PLUME_HD void ecdsa_address_record(uint32_t r[16], int addr_format, const uint32_t ad[5]) {
    PLUME_UNROLL for (int k = 0; k < 16; k++) r[k] = 0u;
    if (addr_format == PLUME_ETHK_ADDR_EIP55) {
        uint32_t hex[10], up[5];
        PLUME_UNROLL for (int k = 0; k < 10; k++) hex[k] = eth_hex4(ad[k >> 1] >> (16 * (k & 1)), 0u);
        keccak256_lanes<5, 5>(up, hex);
        PLUME_UNROLL for (int k = 0; k < 10; k++) hex[k] = eth_hex4(ad[k >> 1] >> (16 * (k & 1)), up[k >> 1] >> (16 * (k & 1)));
        r[0] = 0x7830u | (hex[0] << 16);                                                // "0x"
        PLUME_UNROLL for (int k = 1; k < 10; k++) r[k] = (hex[k - 1] >> 16) | (hex[k] << 16);
        r[10] = hex[9] >> 16;
    } else if (addr_format == PLUME_ETHK_ADDR_RECORD64) {
        PLUME_UNROLL for (int k = 0; k < 5; k++) r[11 + k] = ad[k];
    } else {
        PLUME_UNROLL for (int k = 0; k < 5; k++) r[k] = ad[k];
    }
}
PLUME_HD void ecdsa_put(const EcdsaArgs& a, uint32_t i, const uint32_t pkr[16], const uint32_t adr[16]) {
    if (a.pk) { if (a.pk_format == PLUME_ETHK_PK_SEC1) recover_store<33>(a.pk + 33 * (size_t)i, pkr); else recover_store<64>(a.pk + 64 * (size_t)i, pkr); }
    if (a.address) {
        if (a.addr_format == PLUME_ETHK_ADDR_RECORD64) recover_store<64>(a.address + 64 * (size_t)i, adr);
        else if (a.addr_format == PLUME_ETHK_ADDR_EIP55) recover_store<42>(a.address + 42 * (size_t)i, adr);
        else recover_store<20>(a.address + 20 * (size_t)i, adr);
    }
}
// lane i of k_ecdsa_finalize: res holds affine X, Y (normalize_points ran on it)
PLUME_HD void ecdsa_finalize(const EcdsaArgs& a, uint32_t i) {
    uint32_t pkr[16], adr[16];
    PLUME_UNROLL for (int k = 0; k < 16; k++) { pkr[k] = 0u; adr[k] = 0u; }
    if (a.itemflags[i] || a.resinf[i]) {                                                // rejected by the prepare stage, or Q is the identity
        ecdsa_put(a, i, pkr, adr);
        if (a.status) a.status[i] = (uint8_t)PLUME_ECDSAK_INVALID;
        return;
    }
    fe x, y;
    ld_fe_soa(x, a.res, a.n, i); ld_fe_soa(y, a.res + (size_t)PLUME_FE_W * a.n, a.n, i);
    fe_normalize(x); fe_normalize(y);
    uint32_t xw[8], yw[8], q[16], dg[8], ad[5];
    fe_to_words(xw, x); fe_to_words(yw, y);
    PLUME_UNROLL for (int k = 0; k < 8; k++) { q[k] = bswap32(xw[7 - k]); q[8 + k] = bswap32(yw[7 - k]); }   // x || y big-endian in memory order
    keccak256_lanes<8, 8>(dg, q);
    PLUME_UNROLL for (int k = 0; k < 5; k++) ad[k] = dg[3 + k];                           // bytes 12 .. 31
    recover_record(pkr, a.pk_format == PLUME_ETHK_PK_SEC1 ? PLUME_RCV_FMT_SEC1 : PLUME_RCV_FMT_AFFINE64, xw, yw, false);
    if (a.address) ecdsa_address_record(adr, a.addr_format, ad);
    ecdsa_put(a, i, pkr, adr);
    if (!a.status) return;
    uint32_t diff = 0;
    if (a.expect) {
        uint32_t e[5];
        eth_load20(e, a.expect + 20 * (size_t)i);
        PLUME_UNROLL for (int k = 0; k < 5; k++) diff |= e[k] ^ ad[k];
    }
    a.status[i] = (uint8_t)(diff == 0 ? PLUME_ECDSAK_MATCH : PLUME_ECDSAK_MISMATCH);
}

}  // namespace plume
