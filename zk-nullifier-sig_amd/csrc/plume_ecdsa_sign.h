// Deterministic ECDSA signatures with a recovery id (plume_ecdsa_sign_batch, include/plume_hip.h): what geth, ethers and libsecp256k1 produce for the same key and digest.
// For item i, with z = hash mod n and k the RFC 6979 §3.2 nonce (HMAC-SHA-256, q = n, x = sk as given, h1 = hash itself -- NOT the PLUME preimage of plume_nonce.h;
// aux appends its 32 bytes in steps d and f, §3.6),
//     R = k G,   r = R.x mod n,   s = k^-1 (z + r sk) mod n,   s > (n - 1) / 2: s <- n - s and the parity flips,   v = parity of R.y after that flip (+ 27)
// Four stages, one lane per item (kernels in plume_ecdsa_sign_kernels.hip):
//   ecdsa_sign_nonce     range check of sk; rfc6979_k_core (plume_nonce.h, generic in h1); k goes to the context's workspace as k_sign_nonce stores it: 32 big-endian bytes
//   ecdsa_sign_gmul      k G by the comb at the context's uniform level -- comb_mul_g, comb_mul_g_uniform, comb_mul_g_scan (plume_ec.h), each with its own checked redo,
//                        exactly what the PLUME signer runs for r G.  With the self-check on, a second pass of the same comb computes sk G (task n + i)
//   (to affine)          the existing batched conversion (normalize_points)
//   ecdsa_sign_finalize  r from x; k^-1 by sc_inv (plume_ecdsa.h: fixed iteration count, no data-dependent branch); s; low-s and v; the stores
//     status 0                              signed
//     status 2 (PLUME_STATUS_BAD_SCALAR)    sk outside [1, n - 1], or the nonce cap (PLUME_NONCE_ROUNDS candidates) ran out
//     status 4 (PLUME_STATUS_IDENTITY)      r = 0, s = 0, or R.x >= n (a recovery id the one-byte v does not represent; probability ~2^-128; no retry)
//     any non-zero status: r, s, v all zero
// Everything that touches sk, k, k^-1 or z + r sk is select-based: r = x - n when x >= n, the low-s negation, the zeroing of failed items.  No branch and no address here
// depends on them; the one data-dependent loop is the RFC's retry inside rfc6979_k_core, and the comb's digit-dependent parts are those of the chosen uniform level.
// The self-check (plume_set_sign_selfcheck): finalize writes context-owned staging (r, s, v, status and sk G as x || y), the recover stages of plume_ecdsa.h turn the staged
// (hash, r, s, v) back into a public key, and ecdsa_sign_release -- one lane per item -- is the only thing that writes the caller's arrays: the staged values where the
// recovered key equals the staged sk G; zeros with status 8 for any other item whose own status was 0; an item with a status of its own as mode 0 writes it.
// Compiles as plain C++ for the host (tests/ecdsa_sign), like the other headers.
#pragma once
#include "plume_ecdsa.h"
#include "plume_nonce.h"
#include "plume_selfcheck.h"

#define PLUME_ECDSAK_SIGN_V27 1        // flag bit 0: v is 27 or 28 (PLUME_ECDSA_SIGN_V27, include/plume_hip.h)

namespace plume {

struct EcdsaSignArgs {
    int flags;                        // PLUME_ECDSAK_SIGN_V27
    int uniform;                      // plume_set_sign_uniform: which form of the comb
    uint32_t n;
    uint32_t ntask;                   // points per item: 1 (k G), or 2 with the self-check (task n + i: sk G)
    // the caller's arrays, at any byte offset
    const uint8_t *hash, *sk;         // 32 big-endian bytes per item
    const uint8_t* aux;               // 32 bytes per item, or NULL
    uint8_t *r, *s;                   // 32 big-endian bytes per item (the staging, with the self-check)
    uint8_t *v, *status;              // 1 byte per item
    uint8_t* pkstage;                 // self-check only: sk G as 64 bytes x || y per item, zero for an item with a status; else NULL
    // workspace
    uint8_t* k;                       // 32 big-endian bytes per item, 4-byte aligned: the nonce (wiped behind finalize)
    uint8_t* itemflags;               // n: the status bits of the nonce stage
    uint32_t* res;                    // Jacobian SoA over ntask n points; affine X, Y behind the conversion stage
    uint8_t* resinf;                  // ntask n
    const uint32_t* gcomb;            // the doubling-free comb of G (levels 0, 1)
    const uint32_t* gscan;            // the small scanned table of G (level 2)
};

// 32 bytes at any alignment as big-endian words, w[0] the most significant (plume_nonce.h's order)
PLUME_HD void be_words_load_any(uint32_t w[8], const uint8_t* p) {
    if (((uintptr_t)p & 3u) == 0) { be_words_load(w, p); return; }
    PLUME_UNROLL for (int j = 0; j < 8; j++) w[j] = ((uint32_t)p[4 * j] << 24) | ((uint32_t)p[4 * j + 1] << 16) | ((uint32_t)p[4 * j + 2] << 8) | (uint32_t)p[4 * j + 3];
}
PLUME_HD void sc_from_be_words(sc& r, const uint32_t w[8]) { PLUME_UNROLL for (int j = 0; j < 8; j++) r.v[j] = w[7 - j]; }
PLUME_HD void sc_select(sc& r, uint32_t mask, const sc& a, const sc& b) { PLUME_UNROLL for (int j = 0; j < 8; j++) r.v[j] = sel32(mask, a.v[j], b.v[j]); }   // mask all ones: a

// the nonce of one item without its stores: k (zero for a failed item); returns the status bits.  used: rfc6979_k_core's count
template <int CAP = PLUME_NONCE_ROUNDS>
PLUME_HD uint32_t ecdsa_sign_nonce_values(uint32_t k[8], uint32_t& used, const uint8_t* hash, const uint8_t* sk, const uint8_t* aux) {
    uint32_t x[8], h1[8], q[8];
    be_words_load_any(x, sk);
    be_words_load_any(h1, hash);
    secp256k1_n_be(q);
    const bool sk_ok = be256_in_range(x, q);
    if (aux) {                                                           // the same for every lane of the launch
        uint32_t ax[8];
        be_words_load_any(ax, aux);
        used = rfc6979_k_core<CAP, true>(k, q, x, h1, ax);
    } else {
        used = rfc6979_k_core<CAP, false>(k, q, x, h1, x);
    }
    const uint32_t bad = sel_mask(!sk_ok | (used == 0u));
    PLUME_UNROLL for (int j = 0; j < 8; j++) k[j] = sel32(bad, 0u, k[j]);
    return bad & PLUME_ST_BAD_SCALAR;
}
// lane i of k_ecdsa_sign_nonce; returns rfc6979_k_core's count
template <int CAP = PLUME_NONCE_ROUNDS>
PLUME_HD uint32_t ecdsa_sign_nonce(const EcdsaSignArgs& a, uint32_t i) {
    uint32_t k[8], used;
    const uint32_t st = ecdsa_sign_nonce_values<CAP>(k, used, a.hash + 32 * (size_t)i, a.sk + 32 * (size_t)i, a.aux ? a.aux + 32 * (size_t)i : nullptr);
    be_words_store(a.k + 32 * (size_t)i, k);
    a.itemflags[i] = (uint8_t)st;
    return used;
}

// task which n + i of k_ecdsa_sign_gmul: k G (which 0) or, for the self-check, sk G (which 1)
template <int UNIFORM = 0>
PLUME_HD void ecdsa_sign_gmul(const EcdsaSignArgs& a, uint32_t i, uint32_t which) {
    const size_t nt = (size_t)a.ntask * a.n, t = (size_t)which * a.n + i;
    sc k;
    if (which) { uint32_t w[8]; be_words_load_any(w, a.sk + 32 * (size_t)i); sc_from_be_words(k, w); sc_cond_sub_n(k); }   // (an sk out of range is flagged already: any point will do)
    else sc_from_be_aligned(k, a.k + 32 * (size_t)i);
    jac acc;
    if (UNIFORM == 2) comb_mul_g_scan(acc, k, a.gscan);
    else if (UNIFORM == 1) comb_mul_g_uniform(acc, k, a.gcomb);
    else comb_mul_g(acc, k, a.gcomb);                                    // the identity for the zero nonce of a failed item
    st_jac_soa(a.res, nt, t, acc);
    a.resinf[t] = (uint8_t)acc.inf;
}

// r = x mod n for the canonical field element x (little-endian words): x < p < 2n, one subtraction by select.  Returns PLUME_ST_IDENTITY when x >= n or r = 0, else 0
PLUME_HD uint32_t ecdsa_sign_r_from_x(sc& r, const uint32_t xw[8]) {
    sc x, t;
    uint32_t bw = 0;
    PLUME_UNROLL for (int j = 0; j < 8; j++) { x.v[j] = xw[j]; t.v[j] = subb(xw[j], sc_n(j), bw); }
    const uint32_t ge = sel_mask(bw == 0);
    sc_select(r, ge, t, x);
    return (ge | sel_mask(sc_is_zero(r))) & PLUME_ST_IDENTITY;
}
// the signature of one item from R = (xw, y_odd), the nonce k, sk = d and z, all canonical: r, the low s, the parity behind the flip.  Returns PLUME_ST_IDENTITY for the
// degenerate outcomes (r, s are then whatever the arithmetic gave: the caller zeroes them), else 0
PLUME_HD uint32_t ecdsa_sign_values(sc& r, sc& s, uint32_t& parity, const uint32_t xw[8], uint32_t y_odd, const sc& k, const sc& d, const sc& z) {
    uint32_t st = ecdsa_sign_r_from_x(r, xw);
    sc ki, t, ns;
    sc_inv(ki, k);
    sc_mul(t, r, d);
    sc_add(t, t, z);
    sc_mul(s, ki, t);
    st |= sel_mask(sc_is_zero(s)) & PLUME_ST_IDENTITY;
    const uint32_t high = sel_mask(sc_is_high(s));
    sc_neg(ns, s);
    sc_select(s, high, ns, s);
    parity = (y_odd ^ (high & 1u)) & 1u;
    return st;
}
// a scalar as the eight memory-order words of its 32 big-endian bytes
PLUME_HD void sc_to_record(uint32_t rec[16], const sc& a) {
    PLUME_UNROLL for (int j = 0; j < 8; j++) rec[j] = bswap32(a.v[7 - j]);
    PLUME_UNROLL for (int j = 8; j < 16; j++) rec[j] = 0u;
}
// lane i of k_ecdsa_sign_finalize: res holds affine X, Y (normalize_points ran on it)
PLUME_HD void ecdsa_sign_finalize(const EcdsaSignArgs& a, uint32_t i) {
    const size_t nt = (size_t)a.ntask * a.n;
    fe x, y;
    ld_fe_soa(x, a.res, nt, i); ld_fe_soa(y, a.res + (size_t)PLUME_FE_W * nt, nt, i);
    fe_normalize(x); fe_normalize(y);
    uint32_t xw[8], yw[8], w[8];
    fe_to_words(xw, x); fe_to_words(yw, y);
    sc k, d, z, r, s;
    sc_from_be_aligned(k, a.k + 32 * (size_t)i);
    be_words_load_any(w, a.sk + 32 * (size_t)i); sc_from_be_words(d, w); sc_cond_sub_n(d);
    be_words_load_any(w, a.hash + 32 * (size_t)i); sc_from_be_words(z, w); sc_cond_sub_n(z);                   // any 32 bytes are a hash: z = hash mod n (hash < 2^256 < 2n)
    uint32_t parity;
    const uint32_t own = a.itemflags[i];
    const uint32_t deg = ecdsa_sign_values(r, s, parity, xw, yw[0] & 1u, k, d, z) | (sel_mask(a.resinf[i] != 0) & PLUME_ST_IDENTITY);
    const uint32_t st = sel32(sel_mask(own != 0u), own, deg);                                                  // the nonce stage's verdict comes first
    const uint32_t failed = sel_mask(st != 0u);
    uint32_t rec[16];
    const sc zero = {{0, 0, 0, 0, 0, 0, 0, 0}};
    sc_select(r, failed, zero, r); sc_select(s, failed, zero, s);
    sc_to_record(rec, r); recover_store<32>(a.r + 32 * (size_t)i, rec);
    sc_to_record(rec, s); recover_store<32>(a.s + 32 * (size_t)i, rec);
    a.v[i] = (uint8_t)sel32(failed, 0u, parity + ((a.flags & PLUME_ECDSAK_SIGN_V27) ? 27u : 0u));
    a.status[i] = (uint8_t)st;
    if (!a.pkstage) return;
    fe px, py;                                                                                                 // the self-check's side of the bargain: sk G, public
    ld_fe_soa(px, a.res, nt, (size_t)a.n + i); ld_fe_soa(py, a.res + (size_t)PLUME_FE_W * nt, nt, (size_t)a.n + i);
    fe_normalize(px); fe_normalize(py);
    fe_to_words(xw, px); fe_to_words(yw, py);
    recover_record(rec, PLUME_RCV_FMT_AFFINE64, xw, yw, st != 0u || a.resinf[(size_t)a.n + i] != 0);
    recover_store<64>(a.pkstage + 64 * (size_t)i, rec);
}

// ------------------------------------------------------------------------------------------------ the self-check's release
struct EcdsaSignReleaseArgs {
    uint32_t n;
    // the staging: 16-byte aligned arrays
    const uint8_t *stage_r, *stage_s;         // 32 B / item
    const uint8_t *stage_v, *stage_status;    // 1 B / item
    const uint8_t* stage_pk;                  // 64 B / item: sk G
    const uint8_t* rec_pk;                    // 64 B / item: the key the recover stages found
    const uint8_t* rec_status;                // 1 B / item: their status (PLUME_ECDSAK_MATCH = a key was found)
    // the caller's arrays, at any byte offset
    uint8_t *r, *s, *v, *status;
};
// the verdict on one staged item: true = the recovered key is the signer's
PLUME_HD bool ecdsa_sign_release_verdict(const uint8_t* stage_pk64, const uint8_t* rec_pk64, uint32_t rec_status) {
    uint32_t diff = 0;
    PLUME_UNROLL for (int j = 0; j < 16; j++) diff |= ((const uint32_t*)stage_pk64)[j] ^ ((const uint32_t*)rec_pk64)[j];
    return rec_status == PLUME_ECDSAK_MATCH && diff == 0;
}
// lane i of k_ecdsa_sign_release.  Every value here is public (a withheld s is secret only in that it must not be RELEASED): plain branches
PLUME_HD void ecdsa_sign_release(const EcdsaSignReleaseArgs& a, uint32_t i) {
    const uint32_t own = a.stage_status[i];
    const bool pass = own != 0u || ecdsa_sign_release_verdict(a.stage_pk + 64 * (size_t)i, a.rec_pk + 64 * (size_t)i, a.rec_status[i]);
    uint32_t rr[16], rs[16];
    PLUME_UNROLL for (int j = 0; j < 16; j++) { rr[j] = 0u; rs[j] = 0u; }
    if (pass) {
        PLUME_UNROLL for (int j = 0; j < 8; j++) { rr[j] = ((const uint32_t*)(a.stage_r + 32 * (size_t)i))[j]; rs[j] = ((const uint32_t*)(a.stage_s + 32 * (size_t)i))[j]; }
    }
    recover_store<32>(a.r + 32 * (size_t)i, rr);
    recover_store<32>(a.s + 32 * (size_t)i, rs);
    a.v[i] = pass ? a.stage_v[i] : (uint8_t)0;
    a.status[i] = (uint8_t)(pass ? own : PLUME_ST_SELFCHECK_FAILED);
}

}  // namespace plume
