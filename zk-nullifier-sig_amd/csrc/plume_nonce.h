// Derived signing nonces: RFC 6979 §3.2 (HMAC-SHA-256, qlen = hlen = 256), optionally hedged with §3.6's extra input k', over the PLUME preimage
//     h1 = SHA-256("PLUME-RFC6979" || u8 version || u8 mode || pk_in (64 B, mode 1 only) || msg),   x = sk as given,   q = n.
// One item per lane, the nonce kept in registers until it is stored for SignArgs::r.  No branch and no address depends on sk, k' or h1; the one
// data-dependent branch is step h's retry (candidate outside [1, q-1], probability ~2^-128 for secp256k1), a loop that runs while ANY lane of the
// wavefront still needs a candidate and stops after PLUME_NONCE_ROUNDS candidates -- an item still without one gets r = 0, which the signer's
// scalar check turns into PLUME_STATUS_BAD_SCALAR.
// 256-bit values here are 8 big-endian 32-bit words (w[0] most significant): the byte order of SHA-256's words and of the stored nonce.
// Compiles as plain C++ for the host (tests/nonce), like the other headers.
#pragma once
#include "plume_sha256.h"
#include "plume_stages.h"

#ifndef PLUME_NONCE_ROUNDS
#define PLUME_NONCE_ROUNDS 16   // candidates per item before it is flagged (2^-2000 for n)
#endif

namespace plume {

struct NonceArgs {
    int version;              // 1 or 2: part of h1
    uint32_t n;
    const uint8_t* msgs; const uint64_t* msg_off;
    uint64_t msgs_bytes;      // an item whose offsets msg_span rejects hashes the empty span and never reads msgs (the signer flags it)
    const uint8_t *sk, *aux;  // 32 B / item each; aux NULL: plain RFC 6979
    const uint8_t* pk_in;     // 64 B / item or NULL: mode 1 / 0, part of h1
    uint8_t* r;               // out, 32 B / item: the layout of SignArgs::r
};

// true for every lane of the wavefront when any of them holds `p` (the host build: the one lane)
PLUME_HD bool nonce_any(bool p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __any(p ? 1 : 0) != 0;
#else
    return p;
#endif
}

// HMAC-SHA-256 with a 32-byte key K: the midstates after the blocks K ^ ipad and K ^ opad, computed once per K
struct HmacKey { uint32_t ist[8], ost[8]; };

PLUME_HD void hmac_key_zero(HmacKey& k) {     // K = 0^32 (step c)
    const uint32_t i[8] = {0xf454dead, 0x9725214f, 0x90daf2a0, 0xdf1228ea, 0x64e5750f, 0xa3924181, 0x824a932b, 0xf8e04e32};
    const uint32_t o[8] = {0xd385480f, 0x7abb6477, 0x37c9c538, 0x5dd82467, 0x8e043a72, 0x753434b0, 0xdeb82818, 0x361d45a6};
    PLUME_UNROLL for (int j = 0; j < 8; j++) { k.ist[j] = i[j]; k.ost[j] = o[j]; }
}
PLUME_HD void hmac_key_set(HmacKey& k, const uint32_t key[8]) {
    uint32_t w[16];
    sha256_init(k.ist);
    PLUME_UNROLL for (int j = 0; j < 16; j++) w[j] = (j < 8 ? key[j] : 0u) ^ 0x36363636u;
    sha256_compress(k.ist, w);
    sha256_init(k.ost);
    PLUME_UNROLL for (int j = 0; j < 16; j++) w[j] = (j < 8 ? key[j] : 0u) ^ 0x5c5c5c5cu;
    sha256_compress(k.ost, w);
}
// the outer hash over the 32-byte inner digest
PLUME_HD void hmac_outer(uint32_t out[8], const HmacKey& k, const uint32_t inner[8]) {
    uint32_t w[16];
    PLUME_UNROLL for (int j = 0; j < 16; j++) w[j] = j < 8 ? inner[j] : 0u;
    w[8] = 0x80000000u; w[15] = (64 + 32) * 8;
    PLUME_UNROLL for (int j = 0; j < 8; j++) out[j] = k.ost[j];
    sha256_compress(out, w);
}
// out = HMAC_K(V), or HMAC_K(V || 0x00) when zero_byte (step h's retry)
PLUME_HD void hmac_v(uint32_t out[8], const HmacKey& k, const uint32_t v[8], bool zero_byte = false) {
    uint32_t w[16], st[8];
    PLUME_UNROLL for (int j = 0; j < 16; j++) w[j] = j < 8 ? v[j] : 0u;
    w[8] = zero_byte ? 0x00800000u : 0x80000000u; w[15] = (64 + 32 + (zero_byte ? 1 : 0)) * 8;
    PLUME_UNROLL for (int j = 0; j < 8; j++) st[j] = k.ist[j];
    sha256_compress(st, w);
    hmac_outer(out, k, st);
}
// out = HMAC_K(V || b || x || h [|| aux]) (steps d and f): 97 or 129 bytes after the key block, i.e. 2 or 3 blocks.  Every word index is a
// compile-time constant once unrolled, so the message stays in registers.
template <bool AUX>
PLUME_HD void hmac_vbxh(uint32_t out[8], const HmacKey& k, const uint32_t v[8], uint32_t b, const uint32_t x[8], const uint32_t h[8], const uint32_t aux[8]) {
    constexpr int NS = AUX ? 24 : 16;                 // words after the byte b
    constexpr int NB = AUX ? 3 : 2;                   // blocks
    uint32_t m[16 * NB];
    PLUME_UNROLL for (int j = 0; j < 8; j++) m[j] = v[j];
    uint32_t prev = b;                                // the byte that precedes word s of the shifted sequence
    PLUME_UNROLL for (int s = 0; s < NS; s++) {
        const uint32_t ws = s < 8 ? x[s] : (s < 16 ? h[s - 8] : aux[s - 16]);
        m[8 + s] = (prev << 24) | (ws >> 8);
        prev = ws & 0xFFu;
    }
    m[8 + NS] = (prev << 24) | 0x00800000u;
    PLUME_UNROLL for (int j = 9 + NS; j < 16 * NB; j++) m[j] = 0;
    m[16 * NB - 1] = (64 + 32 + 1 + 4 * NS) * 8;
    uint32_t st[8];
    PLUME_UNROLL for (int j = 0; j < 8; j++) st[j] = k.ist[j];
    PLUME_UNROLL for (int blk = 0; blk < NB; blk++) {
        uint32_t w[16];
        PLUME_UNROLL for (int j = 0; j < 16; j++) w[j] = m[16 * blk + j];
        sha256_compress(st, w);
    }
    hmac_outer(out, k, st);
}

// a - b over big-endian words; returns the borrow out (1: a < b).  SHA-256 words pass through opaque_u32 before the chain (plume_field.h)
PLUME_HD uint32_t be256_sub(uint32_t d[8], const uint32_t a[8], const uint32_t b[8]) {
    uint32_t bw = 0;
    PLUME_UNROLL for (int j = 7; j >= 0; j--) d[j] = subb(opaque_u32(a[j]), b[j], bw);
    return bw;
}
// 1 <= k <= q - 1
PLUME_HD bool be256_in_range(const uint32_t k[8], const uint32_t q[8]) {
    uint32_t d[8], z = 0;
    const uint32_t lt = be256_sub(d, k, q);
    PLUME_UNROLL for (int j = 0; j < 8; j++) z |= k[j];
    return (lt != 0) & (z != 0);
}

// RFC 6979 §3.2 steps b-h for a modulus q of 256 bits whose top bit is set (h1 < 2^256 < 2q: bits2octets is one conditional subtraction, done as a select).
// aux NULL: nothing appended in steps d and f; otherwise its 32 bytes (§3.6).  CAP: candidates before giving up.
// k gets the nonce; returns the number of candidates used (1 = the first was in range), 0 when all CAP were out of range (k = 0 then).
template <int CAP, bool AUX>
PLUME_HD uint32_t rfc6979_k_core(uint32_t k[8], const uint32_t q[8], const uint32_t x[8], const uint32_t h1[8], const uint32_t aux[8]) {
    uint32_t h[8], d[8];
    const uint32_t keep = sel_mask(be256_sub(d, h1, q) != 0);          // h1 < q: h1 itself
    PLUME_UNROLL for (int j = 0; j < 8; j++) h[j] = sel32(keep, h1[j], d[j]);
    HmacKey K;
    hmac_key_zero(K);                                                   // c
    uint32_t V[8], T[8];
    PLUME_UNROLL for (int j = 0; j < 8; j++) V[j] = 0x01010101u;      // b
    hmac_vbxh<AUX>(T, K, V, 0x00, x, h, aux);                           // d
    hmac_key_set(K, T);
    hmac_v(V, K, V);                                                    // e
    hmac_vbxh<AUX>(T, K, V, 0x01, x, h, aux);                           // f
    hmac_key_set(K, T);
    hmac_v(V, K, V);                                                    // g
    hmac_v(V, K, V);                                                    // h: T = V, tlen = qlen
    bool ok = be256_in_range(V, q);
    uint32_t used = ok ? 1u : 0u;
    PLUME_UNROLL for (int j = 0; j < 8; j++) k[j] = V[j];
    PLUME_NOUNROLL for (uint32_t round = 2; round <= (uint32_t)CAP; round++) {
        if (!nonce_any(!ok)) break;                                      // wavefront-uniform: every lane runs the round, lanes that have their k keep it
        hmac_v(T, K, V, true);
        hmac_key_set(K, T);
        hmac_v(V, K, V);
        hmac_v(V, K, V);
        const bool fresh = !ok & be256_in_range(V, q);
        const uint32_t take = sel_mask(fresh);
        PLUME_UNROLL for (int j = 0; j < 8; j++) k[j] = sel32(take, V[j], k[j]);
        used = sel32(take, round, used);
        ok = ok | fresh;
    }
    const uint32_t none = sel_mask(!ok);
    PLUME_UNROLL for (int j = 0; j < 8; j++) k[j] = sel32(none, 0u, k[j]);
    return used;
}

PLUME_HD void be_words_load(uint32_t w[8], const uint8_t* p) {   // 32 bytes at a 4-byte aligned address
    const uint32_t* s = (const uint32_t*)p;
    PLUME_UNROLL for (int j = 0; j < 8; j++) w[j] = bswap32(s[j]);
}
PLUME_HD void be_words_store(uint8_t* p, const uint32_t w[8]) {
    uint32_t* d = (uint32_t*)p;
    PLUME_UNROLL for (int j = 0; j < 8; j++) d[j] = bswap32(w[j]);
}

// the domain tag "PLUME-RFC6979", 13 bytes, as big-endian words
PLUME_HD uint32_t nonce_domain_byte(uint32_t pos) {
    const uint32_t t[4] = {0x504C554Du, 0x452D5246u, 0x43363937u, 0x39000000u};
    uint32_t w = t[0];
    PLUME_UNROLL for (int j = 1; j < 4; j++) w = sel32(sel_mask((pos >> 2) == (uint32_t)j), t[j], w);
    return (w >> (8 * (3 - (pos & 3)))) & 0xFFu;
}
#define PLUME_NONCE_DOMAIN_LEN 13

// h1 of one item: pk64 NULL = mode 0
PLUME_HD void plume_nonce_h1(uint32_t h1[8], int version, const uint8_t* pk64, const uint8_t* msg, uint32_t len) {
    const uint32_t P = PLUME_NONCE_DOMAIN_LEN + 2 + (pk64 ? 64 : 0);
    const uint32_t mode = pk64 ? 1u : 0u;
    sha256_init(h1);
    sha256_absorb_pad(h1, 0, P + len, [=](uint32_t pos) -> uint32_t {
        if (pos < PLUME_NONCE_DOMAIN_LEN) return nonce_domain_byte(pos);
        if (pos == PLUME_NONCE_DOMAIN_LEN) return (uint32_t)version & 0xFFu;
        if (pos == PLUME_NONCE_DOMAIN_LEN + 1) return mode;
        if (pos < P) return pk64[pos - (PLUME_NONCE_DOMAIN_LEN + 2)];
        return msg[pos - P];
    });
}

PLUME_HD void secp256k1_n_be(uint32_t q[8]) {
    const uint32_t n[8] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFEu, 0xBAAEDCE6u, 0xAF48A03Bu, 0xBFD25E8Cu, 0xD0364141u};
    PLUME_UNROLL for (int j = 0; j < 8; j++) q[j] = n[j];
}

// rfc6979_k_core with aux NULL = plain RFC 6979 (the words of aux are then never read)
template <int CAP = PLUME_NONCE_ROUNDS>
PLUME_HD uint32_t rfc6979_k(uint32_t k[8], const uint32_t q[8], const uint32_t x[8], const uint32_t h1[8], const uint32_t* aux) {
    return aux ? rfc6979_k_core<CAP, true>(k, q, x, h1, aux) : rfc6979_k_core<CAP, false>(k, q, x, h1, x);
}

// the lane body of k_sign_nonce: item i's nonce into a.r (r = 0 when the cap ran out); returns rfc6979_k's count
template <int CAP = PLUME_NONCE_ROUNDS>
PLUME_HD uint32_t sign_nonce(const NonceArgs& a, uint32_t i) {
    uint64_t o0; uint32_t len;
    (void)msg_span(o0, len, a.msg_off, i, a.msgs_bytes);                // rejected offsets: the empty span, msgs never read (the signer flags the item)
    uint32_t x[8], h1[8], q[8], k[8], used;
    be_words_load(x, a.sk + 32 * (size_t)i);
    plume_nonce_h1(h1, a.version, a.pk_in ? a.pk_in + 64 * (size_t)i : nullptr, a.msgs + o0, len);
    secp256k1_n_be(q);
    if (a.aux) {                                                         // the same for every lane of the launch
        uint32_t aux[8];
        be_words_load(aux, a.aux + 32 * (size_t)i);
        used = rfc6979_k_core<CAP, true>(k, q, x, h1, aux);
    } else {
        used = rfc6979_k_core<CAP, false>(k, q, x, h1, x);
    }
    be_words_store(a.r + 32 * (size_t)i, k);
    return used;
}

}  // namespace plume
