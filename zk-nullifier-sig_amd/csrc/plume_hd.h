// BIP-32 key derivation on secp256k1 (plume_hd_master_batch, plume_hd_derive_priv_batch, plume_hd_derive_pub_batch, include/plume_hip.h).
//     I = HMAC-SHA512(key = c_par, data),  IL = I[0:32],  IR = I[32:64],  index i as four big-endian bytes
//     CKDpriv   data = 00 || ser256(k_par) || i  for i >= 2^31 (hardened),  serP(k_par G) || i  otherwise;   k_i = IL + k_par mod n,  c_i = IR
//     CKDpub    non-hardened only: data = serP(K_par) || i;   K_i = IL G + K_par,  c_i = IR
//     master    I = HMAC-SHA512(key = "Bitcoin seed", seed);  k = IL,  c = IR
// One lane per item; an item walks `depth` levels of its path.  The kernels (plume_hd_kernels.hip), private form:
//   hd_priv_load     range check of the parent key; k and the chain code go to the context's workspace (32 big-endian bytes each), the status byte beside them
//   per level        hd_gmul: k G by the comb at the context's uniform level, exactly the signer's (comb_mul_g, comb_mul_g_uniform, comb_mul_g_scan, each with its checked
//                    redo) -- at EVERY level for EVERY item, hardened or not, so that the lanes stay uniform and nobody has to look at the paths;
//                    (to affine) the existing batched conversion;  hd_priv_step: serP from the affine point, the hardened or the public preimage chosen per lane by
//                    select on the index bit, the HMAC, the tweak (hd_priv_tweak)
//   behind the last  hd_gmul, to affine, hd_finish: sk, chain code, public key, address (the Keccak / address body of plume_ecdsa.h) and the status
// public form: hd_pub_load (the parent key decoded and validated as plume_eth_address_batch does, into the result array as an affine point), per level hd_pub_step (the HMAC
// over serP(K), IL G by the comb -- IL is public here, the digit-dependent comb is fine -- plus K: hd_pub_tweak) and the conversion, then hd_finish.
//     status 0                                derived
//     status 2  (PLUME_STATUS_BAD_SCALAR)     parent sk outside [1, n - 1]; parent pk not a non-identity curve point in the given format
//     status 32 (PLUME_STATUS_HD_NO_KEY)      IL >= n, child scalar 0 or child point = identity at some level (master: IL = 0 or IL >= n)
//     status 64 (PLUME_STATUS_HD_HARDENED)    public derivation asked for an index >= 2^31
//     the first level that fails decides; any non-zero status: every output record of the item is all zero
// Everything that touches k_par, k_i or the hardened preimage is select-based: the range checks, the reduction of IL + k_par, zero detection, the zeroing of a failed
// item.  No branch and no address depends on them beyond what the chosen uniform level of the comb does with its digits.  A failed item carries k = 0 through the
// remaining levels (its k G is the identity, which the conversion skips); its status is an output, so finish may branch on it.
// Compiles as plain C++ for the host (tests/hd), like the other headers.
#pragma once
#include "plume_ecdsa_sign.h"
#include "plume_sha512.h"

#define PLUME_HDK_MAX_DEPTH 8          // PLUME_HD_MAX_DEPTH (include/plume_hip.h)
#define PLUME_HDK_SHARED_PARENT 1      // flags bit 0: one parent record for every item
#define PLUME_HDK_SHARED_PATH 2        // flags bit 1: one row of indices for every item
#define PLUME_ST_HD_NO_KEY 32u         // PLUME_STATUS_HD_NO_KEY
#define PLUME_ST_HD_HARDENED 64u       // PLUME_STATUS_HD_HARDENED
#define PLUME_HDK_WS_BYTES 65          // workspace per item: k, chain code, status

namespace plume {

struct HdArgs {
    int flags;                        // PLUME_HDK_SHARED_*
    int pk_format, addr_format;       // PLUME_ETHK_PK_*, PLUME_ETHK_ADDR_*
    int uniform;                      // plume_set_sign_uniform: which form of the comb (private form)
    uint32_t n, depth, level;         // level: the one hd_priv_step / hd_pub_step works on
    uint32_t seed_len;                // master only
    // the caller's arrays, at any byte offset
    const uint8_t* parent;            // private: sk, 32 B; public: pk in pk_format; master: the seeds, seed_len B.  One record with SHARED_PARENT
    const uint8_t* parent_chain;      // 32 B (one record with SHARED_PARENT)
    const uint8_t* path;              // uint32 [n][depth] row-major in memory order (one row with SHARED_PATH)
    uint8_t *child_sk, *child_chain;  // 32 B per item; child_chain may be NULL; child_sk NULL in the public form
    uint8_t* child_pk;                // eth_pk_width(pk_format) per item, or NULL
    uint8_t* address;                 // eth_address_width(addr_format) per item, or NULL
    uint8_t* status;                  // 1 B per item
    // workspace
    uint8_t *k, *chain;               // 32 big-endian bytes per item each, 4-byte aligned (wiped behind finish)
    uint8_t* st;                      // n: the status so far
    uint32_t* res;                    // Jacobian SoA over n points; affine X, Y behind the conversion stage
    uint8_t* resinf;                  // n
    const uint32_t* gcomb;            // the doubling-free comb of G (levels 0, 1; the public form)
    const uint32_t* gscan;            // the small scanned table of G (level 2)
};

// four bytes at any alignment as a little-endian word (a uint32 of the caller's in memory order)
PLUME_HD uint32_t hd_load_u32(const uint8_t* p) {
    if (((uintptr_t)p & 3u) == 0) return *(const uint32_t*)p;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
PLUME_HD uint32_t hd_index(const HdArgs& a, uint32_t i, uint32_t level) {
    const size_t row = (a.flags & PLUME_HDK_SHARED_PATH) ? 0 : (size_t)i;
    return hd_load_u32(a.path + 4 * (row * a.depth + level));
}
PLUME_HD size_t hd_parent_row(const HdArgs& a, uint32_t i) { return (a.flags & PLUME_HDK_SHARED_PARENT) ? 0 : (size_t)i; }

// I as its halves: IL as a scalar (not reduced), IR as eight big-endian words
PLUME_HD void hd_split(sc& il, uint32_t ir[8], const uint64_t I[8]) {
    PLUME_UNROLL for (int j = 0; j < 4; j++) { il.v[7 - 2 * j] = (uint32_t)(I[j] >> 32); il.v[6 - 2 * j] = (uint32_t)I[j]; }
    PLUME_UNROLL for (int j = 0; j < 4; j++) { ir[2 * j] = (uint32_t)(I[4 + j] >> 32); ir[2 * j + 1] = (uint32_t)I[4 + j]; }
}
// all ones when a >= n
PLUME_HD uint32_t sc_ge_n_mask(const sc& a) {
    uint32_t bw = 0;
    PLUME_UNROLL for (int j = 0; j < 8; j++) (void)subb(a.v[j], sc_n(j), bw);
    return sel_mask(bw == 0);
}
// the private tweak: k_child = IL + k_par mod n (k_par canonical).  Returns PLUME_ST_HD_NO_KEY when IL >= n or the sum is zero -- k_child is zero then -- else 0.  By select
PLUME_HD uint32_t hd_priv_tweak(sc& k_child, const sc& il, const sc& k_par) {
    const uint32_t ge = sc_ge_n_mask(il);
    sc sum;
    const sc zero = {{0, 0, 0, 0, 0, 0, 0, 0}};
    sc_add(sum, il, k_par);                                                    // (garbage for IL >= n: dropped below)
    const uint32_t bad = ge | sel_mask(sc_is_zero(sum));
    sc_select(k_child, bad, zero, sum);
    return bad & PLUME_ST_HD_NO_KEY;
}
// the public tweak: K_child = IL G + K_par, K_par affine and not the identity.  Returns PLUME_ST_HD_NO_KEY when IL >= n or the sum is the identity, else 0.  Public values
PLUME_HD uint32_t hd_pub_tweak(jac& child, const sc& il, const fe& px, const fe& py, const uint32_t* gcomb) {
    if (sc_ge_n_mask(il)) { child.x = fe_small(1); child.y = fe_small(1); child.z = fe_small(0); child.inf = 1; return PLUME_ST_HD_NO_KEY; }
    comb_mul_g(child, il, gcomb);
    jac_madd<true>(child, px, py);
    return child.inf ? PLUME_ST_HD_NO_KEY : 0u;
}

// the master key of one seed: k (zero when it has no key) and the chain code as big-endian words; returns the status
template <class ByteFn>
PLUME_HD uint32_t hd_master_values(sc& k, uint32_t chain[8], uint32_t seed_len, ByteFn byte) {
    const uint64_t key[4] = {0x426974636f696e20ull, 0x7365656400000000ull, 0ull, 0ull};   // "Bitcoin seed"
    Hmac512Key hk;
    hmac_sha512_key(hk, key);
    uint64_t I[8];
    hmac_sha512_short(I, hk, seed_len, byte);
    sc il;
    hd_split(il, chain, I);
    const uint32_t bad = sc_ge_n_mask(il) | sel_mask(sc_is_zero(il));
    const sc zero = {{0, 0, 0, 0, 0, 0, 0, 0}};
    sc_select(k, bad, zero, il);
    PLUME_UNROLL for (int j = 0; j < 8; j++) chain[j] = sel32(bad, 0u, chain[j]);
    return bad & PLUME_ST_HD_NO_KEY;
}
// eight big-endian words as the memory-order words of their 32 bytes
PLUME_HD void hd_be_record(uint32_t rec[16], const uint32_t w[8]) {
    PLUME_UNROLL for (int j = 0; j < 8; j++) rec[j] = bswap32(w[j]);
    PLUME_UNROLL for (int j = 8; j < 16; j++) rec[j] = 0u;
}
// lane i of k_hd_master
PLUME_HD void hd_master_item(const HdArgs& a, uint32_t i) {
    const uint8_t* seed = a.parent + (size_t)a.seed_len * i;
    sc k; uint32_t chain[8], rec[16];
    const uint32_t st = hd_master_values(k, chain, a.seed_len, [&](uint32_t pos) -> uint64_t { return seed[pos]; });
    sc_to_record(rec, k); recover_store<32>(a.child_sk + 32 * (size_t)i, rec);
    hd_be_record(rec, chain); recover_store<32>(a.child_chain + 32 * (size_t)i, rec);
    a.status[i] = (uint8_t)st;
}

// lane i of k_hd_priv_load
PLUME_HD void hd_priv_load(const HdArgs& a, uint32_t i) {
    const size_t row = hd_parent_row(a, i);
    uint32_t x[8], c[8], q[8];
    be_words_load_any(x, a.parent + 32 * row);
    be_words_load_any(c, a.parent_chain + 32 * row);
    secp256k1_n_be(q);
    const uint32_t bad = sel_mask(!be256_in_range(x, q));
    PLUME_UNROLL for (int j = 0; j < 8; j++) x[j] = sel32(bad, 0u, x[j]);
    be_words_store(a.k + 32 * (size_t)i, x);
    be_words_store(a.chain + 32 * (size_t)i, c);
    a.st[i] = (uint8_t)(bad & PLUME_ST_BAD_SCALAR);
}
// lane i of k_hd_gmul: k G of the workspace's k
template <int UNIFORM = 0>
PLUME_HD void hd_gmul(const HdArgs& a, uint32_t i) {
    sc k;
    sc_from_be_aligned(k, a.k + 32 * (size_t)i);
    jac acc;
    if (UNIFORM == 2) comb_mul_g_scan(acc, k, a.gscan);
    else if (UNIFORM == 1) comb_mul_g_uniform(acc, k, a.gcomb);
    else comb_mul_g(acc, k, a.gcomb);                                          // the identity for the zero key of a failed item
    st_jac_soa(a.res, a.n, i, acc);
    a.resinf[i] = (uint8_t)acc.inf;
}
// the affine point of item i behind the conversion, as canonical little-endian words
PLUME_HD void hd_load_affine(uint32_t xw[8], uint32_t yw[8], const HdArgs& a, uint32_t i) {
    fe x, y;
    ld_fe_soa(x, a.res, a.n, i); ld_fe_soa(y, a.res + (size_t)PLUME_FE_W * a.n, a.n, i);
    fe_normalize(x); fe_normalize(y);
    fe_to_words(xw, x); fe_to_words(yw, y);
}
// one private level without its loads and stores: from k_par (canonical), the chain code and k_par G = (xw, y_odd), the child key and chain code; returns the status bits
PLUME_HD uint32_t hd_priv_level(sc& k_child, uint32_t chain_child[8], const sc& k_par, const uint32_t chain[8], const uint32_t xw[8], uint32_t y_odd, uint32_t idx) {
    const uint32_t hard = sel_mask((idx >> 31) != 0u);
    uint32_t body[8];
    PLUME_UNROLL for (int j = 0; j < 8; j++) body[j] = sel32(hard, k_par.v[7 - j], xw[7 - j]);
    const uint32_t b0 = sel32(hard, 0u, 2u + (y_odd & 1u));
    Hmac512Key hk;
    hmac_sha512_key32(hk, chain);
    uint64_t I[8];
    hmac_sha512_37(I, hk, b0, body, idx);
    sc il;
    hd_split(il, chain_child, I);
    return hd_priv_tweak(k_child, il, k_par);
}
// lane i of k_hd_priv_step, level a.level
PLUME_HD void hd_priv_step(const HdArgs& a, uint32_t i) {
    uint32_t xw[8], yw[8], c[8], cc[8], kw[8];
    hd_load_affine(xw, yw, a, i);
    sc k, kc;
    sc_from_be_aligned(k, a.k + 32 * (size_t)i);
    be_words_load(c, a.chain + 32 * (size_t)i);
    const uint32_t own = a.st[i];
    const uint32_t lvl = hd_priv_level(kc, cc, k, c, xw, yw[0] & 1u, hd_index(a, i, a.level));
    const uint32_t st = sel32(sel_mask(own != 0u), own, lvl);                   // the first level that fails decides
    const uint32_t failed = sel_mask(st != 0u);
    PLUME_UNROLL for (int j = 0; j < 8; j++) { kw[j] = sel32(failed, 0u, kc.v[7 - j]); cc[j] = sel32(failed, 0u, cc[j]); }
    be_words_store(a.k + 32 * (size_t)i, kw);
    be_words_store(a.chain + 32 * (size_t)i, cc);
    a.st[i] = (uint8_t)st;
}

// lane i of k_hd_pub_load: the parent key as an affine point in the result array (G stands in for a rejected one)
PLUME_HD void hd_pub_load(const HdArgs& a, uint32_t i) {
    const size_t row = hd_parent_row(a, i);
    EthArgs e;
    e.pk_format = a.pk_format; e.addr_format = 0; e.n = a.n; e.pk = a.parent; e.expect = nullptr; e.address = nullptr; e.status = nullptr;
    uint32_t q[16], c[8], wx[8], wy[8];
    const bool ok = eth_load_pk(q, e, (uint32_t)row);
    be_words_load_any(c, a.parent_chain + 32 * row);
    PLUME_UNROLL for (int k = 0; k < 8; k++) { wx[k] = bswap32(q[7 - k]); wy[k] = bswap32(q[15 - k]); }
    jac p;
    fe_from_words(p.x, wx); fe_from_words(p.y, wy); p.z = fe_small(1); p.inf = 0;
    if (!ok) { p.x = fe_gx(); p.y = fe_gy(); }
    st_jac_soa(a.res, a.n, i, p);
    a.resinf[i] = 0;
    be_words_store(a.chain + 32 * (size_t)i, c);
    a.st[i] = (uint8_t)(ok ? 0u : PLUME_ST_BAD_SCALAR);
}
// one public level without its loads and stores: from K_par = (x, y) affine and the chain code, the child point and chain code; returns the status bits
PLUME_HD uint32_t hd_pub_level(jac& child, uint32_t chain_child[8], const fe& x, const fe& y, const uint32_t chain[8], uint32_t idx, const uint32_t* gcomb) {
    if (idx >> 31) { child.x = fe_small(1); child.y = fe_small(1); child.z = fe_small(0); child.inf = 1; return PLUME_ST_HD_HARDENED; }
    uint32_t xw[8], yw[8], body[8];
    fe_to_words(xw, x); fe_to_words(yw, y);
    PLUME_UNROLL for (int j = 0; j < 8; j++) body[j] = xw[7 - j];
    Hmac512Key hk;
    hmac_sha512_key32(hk, chain);
    uint64_t I[8];
    hmac_sha512_37(I, hk, 2u + (yw[0] & 1u), body, idx);
    sc il;
    hd_split(il, chain_child, I);
    return hd_pub_tweak(child, il, x, y, gcomb);
}
// lane i of k_hd_pub_step, level a.level
PLUME_HD void hd_pub_step(const HdArgs& a, uint32_t i) {
    fe x, y;
    ld_fe_soa(x, a.res, a.n, i); ld_fe_soa(y, a.res + (size_t)PLUME_FE_W * a.n, a.n, i);
    fe_normalize(x); fe_normalize(y);
    uint32_t c[8], cc[8];
    be_words_load(c, a.chain + 32 * (size_t)i);
    const uint32_t own = a.st[i];
    jac child;
    const uint32_t lvl = hd_pub_level(child, cc, x, y, c, hd_index(a, i, a.level), a.gcomb);
    const uint32_t st = own ? own : lvl;
    if (st) {                                                                   // a failed item walks on as G: every later level has a point to hash
        child.x = fe_gx(); child.y = fe_gy(); child.z = fe_small(1); child.inf = 0;
        PLUME_UNROLL for (int j = 0; j < 8; j++) cc[j] = 0u;
    }
    st_jac_soa(a.res, a.n, i, child);
    a.resinf[i] = 0;
    be_words_store(a.chain + 32 * (size_t)i, cc);
    a.st[i] = (uint8_t)st;
}

// lane i of k_hd_finish: res holds the affine child point.  has_sk: the private form
PLUME_HD void hd_finish(const HdArgs& a, uint32_t i) {
    uint32_t xw[8], yw[8], c[8], rec[16], pkr[16], adr[16];
    hd_load_affine(xw, yw, a, i);
    be_words_load(c, a.chain + 32 * (size_t)i);
    const uint32_t own = a.st[i];
    const uint32_t st = own | (sel_mask(own == 0u && a.resinf[i] != 0) & PLUME_ST_HD_NO_KEY);
    const uint32_t failed = sel_mask(st != 0u);
    if (a.child_sk) {
        uint32_t kw[8];
        be_words_load(kw, a.k + 32 * (size_t)i);
        PLUME_UNROLL for (int j = 0; j < 8; j++) kw[j] = sel32(failed, 0u, kw[j]);
        hd_be_record(rec, kw); recover_store<32>(a.child_sk + 32 * (size_t)i, rec);
    }
    if (a.child_chain) {
        PLUME_UNROLL for (int j = 0; j < 8; j++) c[j] = sel32(failed, 0u, c[j]);
        hd_be_record(rec, c); recover_store<32>(a.child_chain + 32 * (size_t)i, rec);
    }
    a.status[i] = (uint8_t)st;
    if (!a.child_pk && !a.address) return;
    PLUME_UNROLL for (int k = 0; k < 16; k++) { pkr[k] = 0u; adr[k] = 0u; }
    if (!st) {                                                                  // the status is an output: public
        recover_record(pkr, a.pk_format == PLUME_ETHK_PK_SEC1 ? PLUME_RCV_FMT_SEC1 : PLUME_RCV_FMT_AFFINE64, xw, yw, false);
        if (a.address) {
            uint32_t q[16], dg[8], ad[5];
            PLUME_UNROLL for (int k = 0; k < 8; k++) { q[k] = bswap32(xw[7 - k]); q[8 + k] = bswap32(yw[7 - k]); }
            keccak256_lanes<8, 8>(dg, q);
            PLUME_UNROLL for (int k = 0; k < 5; k++) ad[k] = dg[3 + k];
            ecdsa_address_record(adr, a.addr_format, ad);
        }
    }
    if (a.child_pk) { if (a.pk_format == PLUME_ETHK_PK_SEC1) recover_store<33>(a.child_pk + 33 * (size_t)i, pkr); else recover_store<64>(a.child_pk + 64 * (size_t)i, pkr); }
    if (a.address) {
        if (a.addr_format == PLUME_ETHK_ADDR_RECORD64) recover_store<64>(a.address + 64 * (size_t)i, adr);
        else if (a.addr_format == PLUME_ETHK_ADDR_EIP55) recover_store<42>(a.address + 42 * (size_t)i, adr);
        else recover_store<20>(a.address + 20 * (size_t)i, adr);
    }
}

}  // namespace plume
