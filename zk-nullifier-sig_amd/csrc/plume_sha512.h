// SHA-512 (FIPS 180-4) and HMAC-SHA-512 (RFC 2104) in the one fixed shape BIP-32 uses (plume_hd.h): one hash state per lane as eight 64-bit words, the 80 rounds fully
// unrolled over a rolling 16-word schedule whose indices are all literals once unrolled (a run-time index would send the window to scratch).
// The HMAC key is at most 32 bytes here (a chain code, or "Bitcoin seed"), so K ^ ipad and K ^ opad are one 128-byte block each, computed once per key (Hmac512Key, in the
// manner of HmacKey in plume_nonce.h); the data is one block too -- 37 bytes for a child key, 16 .. 64 bytes for a master seed -- and the outer hash is one block over the
// 64-byte inner digest: four compressions per HMAC.
// Compiles as plain C++ for the host (tests/hd), like the other headers.
// Library 0.18 adds, for PBKDF2 (plume_kdf.h), a smaller form of the same compression (sha512_compress_grouped, rotations on 32-bit halves) and the multi-block tail
// with padding for data of any length (sha512_absorb); what BIP-32 uses is unchanged.
#pragma once
#include "plume_field.h"

namespace plume {

PLUME_HD uint64_t rotr64(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }

PLUME_HD constexpr uint64_t sha512_k(int i) {
    constexpr uint64_t K[80] = {
        0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull, 0x59f111f1b605d019ull, 0x923f82a4af194f9bull,
        0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull, 0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull,
        0x9bdc06a725c71235ull, 0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull, 0x2de92c6f592b0275ull,
        0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull, 0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull,
        0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull, 0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull,
        0x53380d139d95b3dfull, 0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull, 0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull,
        0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull, 0x19a4c116b8d2d0c8ull,
        0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull,
        0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull, 0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull,
        0xc67178f2e372532bull, 0xca273eceea26619cull, 0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull,
        0x113f9804bef90daeull, 0x1b710b35131c471bull, 0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull,
        0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};
    return K[i];
}

PLUME_HD void sha512_init(uint64_t st[8]) {
    st[0] = 0x6a09e667f3bcc908ull; st[1] = 0xbb67ae8584caa73bull; st[2] = 0x3c6ef372fe94f82bull; st[3] = 0xa54ff53a5f1d36f1ull;
    st[4] = 0x510e527fade682d1ull; st[5] = 0x9b05688c2b3e6c1full; st[6] = 0x1f83d9abfb41bd6bull; st[7] = 0x5be0cd19137e2179ull;
}

// one compression; w[16] is consumed (used as the rolling schedule window)
PLUME_HD void sha512_compress(uint64_t st[8], uint64_t w[16]) {
    uint64_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
    PLUME_UNROLL for (int i = 0; i < 80; i++) {
        uint64_t wi;
        if (i < 16) {
            wi = w[i];
        } else {
            const uint64_t w15 = w[(i - 15) & 15], w2 = w[(i - 2) & 15];
            const uint64_t s0 = rotr64(w15, 1) ^ rotr64(w15, 8) ^ (w15 >> 7);
            const uint64_t s1 = rotr64(w2, 19) ^ rotr64(w2, 61) ^ (w2 >> 6);
            wi = w[i & 15] + s0 + w[(i - 7) & 15] + s1;
            w[i & 15] = wi;
        }
        const uint64_t S1 = rotr64(e, 14) ^ rotr64(e, 18) ^ rotr64(e, 41);
        const uint64_t ch = (e & f) ^ (~e & g);
        const uint64_t t1 = h + S1 + ch + sha512_k(i) + wi;
        const uint64_t S0 = rotr64(a, 28) ^ rotr64(a, 34) ^ rotr64(a, 39);
        const uint64_t mj = (a & b) ^ (a & c) ^ (b & c);
        const uint64_t t2 = S0 + mj;
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

// A rotation by a literal count on the 32-bit halves: two funnel shifts (v_alignbit_b32) on the device, where the compiler makes of the plain form two 64-bit shifts
// and two ORs.  N is 1 .. 63
template <int N>
PLUME_HD uint64_t rotr64_halves(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    if (N == 32) return ((uint64_t)lo << 32) | hi;
    const uint32_t a = N < 32 ? lo : hi, b = N < 32 ? hi : lo;      // the value rotated by 32 first when N > 32
    return ((uint64_t)__builtin_amdgcn_alignbit(a, b, N & 31) << 32) | __builtin_amdgcn_alignbit(b, a, N & 31);
#else
    return rotr64(x, N);
#endif
}
// One round on the eight working words as a[0 .. 7] = a .. h; the rotation of the roles is the caller's (literal indices once unrolled)
PLUME_HD void sha512_round(uint64_t& a, uint64_t& b, uint64_t& c, uint64_t& d, uint64_t& e, uint64_t& f, uint64_t& g, uint64_t& h, uint64_t kw) {
    const uint64_t S1 = rotr64_halves<14>(e) ^ rotr64_halves<18>(e) ^ rotr64_halves<41>(e);
    const uint64_t ch = (e & f) ^ (~e & g);
    const uint64_t t1 = h + S1 + ch + kw;
    const uint64_t S0 = rotr64_halves<28>(a) ^ rotr64_halves<34>(a) ^ rotr64_halves<39>(a);
    const uint64_t mj = (a & b) ^ (a & c) ^ (b & c);
    h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + S0 + mj;
}
// The same compression in a fifth of the code (plume_kdf.h: a loop body of two compressions has to leave room for two waves per SIMD): sixteen unrolled rounds over
// w as it comes, then four trips of sixteen unrolled rounds that roll the schedule, the round constants read from the table at 16 grp + i -- grp is uniform, so the
// table reads are scalar loads from constant memory and every index into w stays a literal.  w[16] is consumed
PLUME_HD void sha512_compress_grouped(uint64_t st[8], uint64_t w[16]) {
    uint64_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
    PLUME_UNROLL for (int i = 0; i < 16; i++) sha512_round(a, b, c, d, e, f, g, h, sha512_k(i) + w[i]);
    PLUME_NOUNROLL for (int grp = 1; grp < 5; grp++) {
        PLUME_UNROLL for (int i = 0; i < 16; i++) {
            const uint64_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
            const uint64_t s0 = rotr64_halves<1>(w15) ^ rotr64_halves<8>(w15) ^ (w15 >> 7);
            const uint64_t s1 = rotr64_halves<19>(w2) ^ rotr64_halves<61>(w2) ^ (w2 >> 6);
            w[i] += s0 + w[(i + 9) & 15] + s1;
            sha512_round(a, b, c, d, e, f, g, h, sha512_k(16 * grp + i) + w[i]);
        }
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

// SHA-512's tail over `len` bytes of any length given by byte(pos), 0 <= pos < len, padding included: `prefix` bytes (a multiple of 128) are already absorbed into st.
// One trip per 128-byte block, the block count a function of len alone; byte() is never asked for a position at or beyond len
template <class ByteFn>
PLUME_HD void sha512_absorb(uint64_t st[8], uint64_t prefix, uint64_t len, ByteFn byte) {
    const uint64_t nblk = (len + 17 + 127) / 128;          // the 0x80 byte and the 16-byte length field
    PLUME_NOUNROLL for (uint64_t b = 0; b < nblk; b++) {
        uint64_t w[16];
        PLUME_UNROLL for (int k = 0; k < 16; k++) {
            uint64_t word = 0;
            PLUME_UNROLL for (int q = 0; q < 8; q++) {
                const uint64_t pos = 128 * b + (uint64_t)(8 * k + q);
                uint64_t v = 0;
                if (pos < len) v = byte(pos);
                else if (pos == len) v = 0x80;
                word = (word << 8) | v;
            }
            w[k] = word;
        }
        if (b + 1 == nblk) w[15] = (prefix + len) << 3;    // (w[14], the length's upper half, is zero: lengths stay below 2^61)
        sha512_compress_grouped(st, w);
    }
}

// SHA-512 of `len` <= 111 bytes (one block) given by byte(pos), 0 <= pos < len; len is the same for every lane of a launch.  prefix_blocks 128-byte blocks are
// already absorbed into st
template <class ByteFn>
PLUME_HD void sha512_one_block(uint64_t st[8], uint32_t prefix_blocks, uint32_t len, ByteFn byte) {
    uint64_t w[16];
    PLUME_UNROLL for (int k = 0; k < 14; k++) {
        uint64_t word = 0;
        PLUME_UNROLL for (int q = 0; q < 8; q++) {
            const uint32_t pos = 8 * k + q;
            uint64_t v = 0;
            if (pos < len) v = byte(pos);
            else if (pos == len) v = 0x80;
            word = (word << 8) | v;
        }
        w[k] = word;
    }
    w[14] = 0;
    w[15] = (uint64_t)(128u * prefix_blocks + len) << 3;
    sha512_compress(st, w);
}

// HMAC-SHA-512 with a key of at most 32 bytes: the midstates after the blocks K ^ ipad and K ^ opad
struct Hmac512Key { uint64_t ist[8], ost[8]; };

// key: the key's bytes as four big-endian 64-bit words, zero beyond its length (HMAC pads a short key with zeros)
PLUME_HD void hmac_sha512_key(Hmac512Key& k, const uint64_t key[4]) {
    uint64_t w[16];
    sha512_init(k.ist);
    PLUME_UNROLL for (int j = 0; j < 16; j++) w[j] = (j < 4 ? key[j] : 0ull) ^ 0x3636363636363636ull;
    sha512_compress(k.ist, w);
    sha512_init(k.ost);
    PLUME_UNROLL for (int j = 0; j < 16; j++) w[j] = (j < 4 ? key[j] : 0ull) ^ 0x5c5c5c5c5c5c5c5cull;
    sha512_compress(k.ost, w);
}
// ... from the eight big-endian 32-bit words of a 32-byte key (a chain code)
PLUME_HD void hmac_sha512_key32(Hmac512Key& k, const uint32_t key[8]) {
    uint64_t kw[4];
    PLUME_UNROLL for (int j = 0; j < 4; j++) kw[j] = ((uint64_t)key[2 * j] << 32) | key[2 * j + 1];
    hmac_sha512_key(k, kw);
}
// the outer hash over the 64-byte inner digest (in place)
PLUME_HD void hmac_sha512_outer(uint64_t io[8], const Hmac512Key& k) {
    uint64_t w[16];
    PLUME_UNROLL for (int j = 0; j < 16; j++) w[j] = j < 8 ? io[j] : 0ull;
    w[8] = 0x8000000000000000ull; w[15] = (128 + 64) * 8;
    PLUME_UNROLL for (int j = 0; j < 8; j++) io[j] = k.ost[j];
    sha512_compress(io, w);
}
// out = HMAC_K(b0 || body || idx): the 37 bytes of a BIP-32 child: one byte, 32 bytes given as eight big-endian words, the index as four big-endian bytes
PLUME_HD void hmac_sha512_37(uint64_t out[8], const Hmac512Key& k, uint32_t b0, const uint32_t body[8], uint32_t idx) {
    uint32_t m[10];                                    // the byte stream as big-endian 32-bit words: everything behind b0 is shifted by one byte
    uint32_t prev = b0 & 0xFFu;
    PLUME_UNROLL for (int s = 0; s < 9; s++) {
        const uint32_t ws = s < 8 ? body[s] : idx;
        m[s] = (prev << 24) | (ws >> 8);
        prev = ws & 0xFFu;
    }
    m[9] = (prev << 24) | 0x00800000u;
    uint64_t w[16];
    PLUME_UNROLL for (int j = 0; j < 5; j++) w[j] = ((uint64_t)m[2 * j] << 32) | m[2 * j + 1];
    PLUME_UNROLL for (int j = 5; j < 15; j++) w[j] = 0;
    w[15] = (128 + 37) * 8;
    PLUME_UNROLL for (int j = 0; j < 8; j++) out[j] = k.ist[j];
    sha512_compress(out, w);
    hmac_sha512_outer(out, k);
}
// out = HMAC_K(data) for len <= 111 bytes given by byte(pos) (the master seed: 16 .. 64 bytes)
template <class ByteFn>
PLUME_HD void hmac_sha512_short(uint64_t out[8], const Hmac512Key& k, uint32_t len, ByteFn byte) {
    PLUME_UNROLL for (int j = 0; j < 8; j++) out[j] = k.ist[j];
    sha512_one_block(out, 1, len, byte);
    hmac_sha512_outer(out, k);
}

}  // namespace plume
