// Ethereum addresses of public keys (plume_eth_address_batch, include/plume_hip.h): address = Keccak-256(x || y)[12..32) over the 64 big-endian bytes of the affine
// point.  Keccak-256 is the ORIGINAL padding (first pad byte 0x01, last 0x80, rate 136 bytes), not SHA3-256 (0x06).  One lane per item (k_eth_address,
// plume_eth_kernels.hip): validate the key, one permutation for the address, a second one over the 40 lower-case hex digits when the EIP-55 form is asked for, compare
// with the expected address, WRITE the record and a status byte.
//     status 3 (PLUME_ETH_INVALID)   pk is not a non-identity curve point in the given format: the record is all zero, whatever expect holds
//     status 1 (PLUME_ETH_MATCH)     expect is NULL or equals the address
//     status 0 (PLUME_ETH_MISMATCH)  the address is written all the same
// A key is valid when its coordinates are below p, the point is on the curve and is NOT the identity: the all-zero record, which the verifier takes as the identity, has no
// address.  SEC1 input goes through decompress_point (plume_stages.h), 64-byte input through affine_on_curve (plume_ec.h): the verifier's own checks.
// The 25 lanes of the state are a local array that only ever sees literal indices: the 24 rounds are 24 expansions of one macro, every rotation amount and every rho/pi
// index is written out, so the state lives in registers (a run-time index would put it in scratch).  A 64-byte message is one absorb: lanes 0-7 are the message, lane 8
// is the 0x01 pad byte, lane 16 ends the 136-byte rate with 0x80 in its top byte.  Every value here is public: plain branches.
// Records are written the way k_recover_finalize writes its own (recover_store, plume_recover.h): strides 20 and 42 are no multiples of 16 and the caller's array may sit
// at any byte offset, so a record is byte stores up to the first 16-byte boundary inside it, 16-byte stores for the whole quads, byte stores for the rest.
// Compiles as plain C++ for the host (tests/eth, tests/hostsim), like the other headers.
#pragma once
#include "plume_recover.h"

#define PLUME_ETHK_MISMATCH 0u         // PLUME_ETH_* (include/plume_hip.h)
#define PLUME_ETHK_MATCH 1u
#define PLUME_ETHK_INVALID 3u
#define PLUME_ETHK_PK_AFFINE64 0       // 64 B x || y big-endian
#define PLUME_ETHK_PK_SEC1 1           // 33 B 02|03 || x
#define PLUME_ETHK_ADDR_RAW20 0        // 20 B
#define PLUME_ETHK_ADDR_RECORD64 1     // 44 zero bytes, then the 20 address bytes
#define PLUME_ETHK_ADDR_EIP55 2        // "0x" + 40 hex digits, mixed-case checksum, no terminator

namespace plume {

struct EthArgs {
    int pk_format, addr_format;       // PLUME_ETHK_PK_*, PLUME_ETHK_ADDR_*
    uint32_t n;
    const uint8_t* pk;                // 64 or 33 bytes per item
    const uint8_t* expect;            // 20 bytes per item, or NULL
    uint8_t* address;                 // eth_address_width(addr_format) bytes per item, or NULL
    uint8_t* status;                  // 1 byte per item, or NULL
};

PLUME_HD uint32_t eth_pk_width(int pk_format) { return pk_format == PLUME_ETHK_PK_SEC1 ? 33u : 64u; }
PLUME_HD uint32_t eth_address_width(int addr_format) { return addr_format == PLUME_ETHK_ADDR_RECORD64 ? 64u : addr_format == PLUME_ETHK_ADDR_EIP55 ? 42u : 20u; }

PLUME_HD uint64_t keccak_rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }

// one round of Keccak-f[1600] on a[25] (lane x + 5 y), round constant rc; b, c, d are the caller's temporaries.  Literal indices only.
#define PLUME_KECCAK_CHI(y)                                                                                                                        \
    a[y + 0] = b[y + 0] ^ (~b[y + 1] & b[y + 2]); a[y + 1] = b[y + 1] ^ (~b[y + 2] & b[y + 3]); a[y + 2] = b[y + 2] ^ (~b[y + 3] & b[y + 4]);        \
    a[y + 3] = b[y + 3] ^ (~b[y + 4] & b[y + 0]); a[y + 4] = b[y + 4] ^ (~b[y + 0] & b[y + 1]);
#define PLUME_KECCAK_ROUND(rc)                                                                                                                     \
    c[0] = a[0] ^ a[5] ^ a[10] ^ a[15] ^ a[20]; c[1] = a[1] ^ a[6] ^ a[11] ^ a[16] ^ a[21]; c[2] = a[2] ^ a[7] ^ a[12] ^ a[17] ^ a[22];              \
    c[3] = a[3] ^ a[8] ^ a[13] ^ a[18] ^ a[23]; c[4] = a[4] ^ a[9] ^ a[14] ^ a[19] ^ a[24];                                                         \
    d[0] = c[4] ^ keccak_rotl(c[1], 1); d[1] = c[0] ^ keccak_rotl(c[2], 1); d[2] = c[1] ^ keccak_rotl(c[3], 1);                                     \
    d[3] = c[2] ^ keccak_rotl(c[4], 1); d[4] = c[3] ^ keccak_rotl(c[0], 1);                                                                         \
    b[0] = a[0] ^ d[0];                          b[10] = keccak_rotl(a[1] ^ d[1], 1);    b[20] = keccak_rotl(a[2] ^ d[2], 62);                       \
    b[5] = keccak_rotl(a[3] ^ d[3], 28);         b[15] = keccak_rotl(a[4] ^ d[4], 27);   b[16] = keccak_rotl(a[5] ^ d[0], 36);                       \
    b[1] = keccak_rotl(a[6] ^ d[1], 44);         b[11] = keccak_rotl(a[7] ^ d[2], 6);    b[21] = keccak_rotl(a[8] ^ d[3], 55);                       \
    b[6] = keccak_rotl(a[9] ^ d[4], 20);         b[7] = keccak_rotl(a[10] ^ d[0], 3);    b[17] = keccak_rotl(a[11] ^ d[1], 10);                      \
    b[2] = keccak_rotl(a[12] ^ d[2], 43);        b[12] = keccak_rotl(a[13] ^ d[3], 25);  b[22] = keccak_rotl(a[14] ^ d[4], 39);                      \
    b[23] = keccak_rotl(a[15] ^ d[0], 41);       b[8] = keccak_rotl(a[16] ^ d[1], 45);   b[18] = keccak_rotl(a[17] ^ d[2], 15);                      \
    b[3] = keccak_rotl(a[18] ^ d[3], 21);        b[13] = keccak_rotl(a[19] ^ d[4], 8);   b[14] = keccak_rotl(a[20] ^ d[0], 18);                      \
    b[24] = keccak_rotl(a[21] ^ d[1], 2);        b[9] = keccak_rotl(a[22] ^ d[2], 61);   b[19] = keccak_rotl(a[23] ^ d[3], 56);                      \
    b[4] = keccak_rotl(a[24] ^ d[4], 14);                                                                                                          \
    PLUME_KECCAK_CHI(0) PLUME_KECCAK_CHI(5) PLUME_KECCAK_CHI(10) PLUME_KECCAK_CHI(15) PLUME_KECCAK_CHI(20)                                        \
    a[0] ^= rc;

// Keccak-f[1600]
PLUME_HD void keccak_f1600(uint64_t a[25]) {
    uint64_t b[25], c[5], d[5];
    PLUME_KECCAK_ROUND(0x0000000000000001ull) PLUME_KECCAK_ROUND(0x0000000000008082ull) PLUME_KECCAK_ROUND(0x800000000000808Aull) PLUME_KECCAK_ROUND(0x8000000080008000ull)
    PLUME_KECCAK_ROUND(0x000000000000808Bull) PLUME_KECCAK_ROUND(0x0000000080000001ull) PLUME_KECCAK_ROUND(0x8000000080008081ull) PLUME_KECCAK_ROUND(0x8000000000008009ull)
    PLUME_KECCAK_ROUND(0x000000000000008Aull) PLUME_KECCAK_ROUND(0x0000000000000088ull) PLUME_KECCAK_ROUND(0x0000000080008009ull) PLUME_KECCAK_ROUND(0x000000008000000Aull)
    PLUME_KECCAK_ROUND(0x000000008000808Bull) PLUME_KECCAK_ROUND(0x800000000000008Bull) PLUME_KECCAK_ROUND(0x8000000000008089ull) PLUME_KECCAK_ROUND(0x8000000000008003ull)
    PLUME_KECCAK_ROUND(0x8000000000008002ull) PLUME_KECCAK_ROUND(0x8000000000000080ull) PLUME_KECCAK_ROUND(0x000000000000800Aull) PLUME_KECCAK_ROUND(0x800000008000000Aull)
    PLUME_KECCAK_ROUND(0x8000000080008081ull) PLUME_KECCAK_ROUND(0x8000000000008080ull) PLUME_KECCAK_ROUND(0x0000000080000001ull) PLUME_KECCAK_ROUND(0x8000000080008008ull)
}
#undef PLUME_KECCAK_ROUND
#undef PLUME_KECCAK_CHI

// Keccak-256 of a message of NL whole 8-byte lanes (NL <= 15: one absorb); m: the message as little-endian 32-bit words in memory order; out: the first 20 or 32 bytes
// of the digest the same way (OW words)
template <int NL, int OW>
PLUME_HD void keccak256_lanes(uint32_t* out, const uint32_t* m) {
    uint64_t a[25];
    PLUME_UNROLL for (int k = 0; k < 25; k++) a[k] = 0;
    PLUME_UNROLL for (int k = 0; k < NL; k++) a[k] = (uint64_t)m[2 * k] | ((uint64_t)m[2 * k + 1] << 32);
    a[NL] = 0x01ull;                                                                     // the pad's first byte follows the message
    a[16] ^= 0x80ull << 56;                                                              // ... its last one ends the rate: byte 135
    keccak_f1600(a);
    PLUME_UNROLL for (int k = 0; k < OW; k++) out[k] = (uint32_t)(a[k >> 1] >> (32 * (k & 1)));
}

// the four lower-case hex digits of two bytes (v = b0 | b1 << 8), in memory order; up: the two bytes of the checksum hash at the same place -- a LETTER is upper-cased
// when its nibble of the hash is at least 8 (EIP-55)
PLUME_HD uint32_t eth_hex4(uint32_t v, uint32_t up) {
    const uint32_t x = (v & 0xFFu) | ((v & 0xFF00u) << 8), y = (up & 0xFFu) | ((up & 0xFF00u) << 8);
    const uint32_t nib = ((x >> 4) & 0x000F000Fu) | ((x & 0x000F000Fu) << 8);             // one nibble per byte, high nibble first
    const uint32_t hn = ((y >> 4) & 0x000F000Fu) | ((y & 0x000F000Fu) << 8);
    const uint32_t letter = ((nib + 0x06060606u) >> 4) & 0x01010101u;                    // nibble >= 10
    const uint32_t upper = letter & (hn >> 3);
    return nib + 0x30303030u + letter * 39u - upper * 32u;
}

// 20 bytes at any alignment as five little-endian words
PLUME_HD void eth_load20(uint32_t w[5], const uint8_t* p) {
    if (((uintptr_t)p & 3u) == 0) {
        PLUME_UNROLL for (int k = 0; k < 5; k++) w[k] = ((const uint32_t*)p)[k];
    } else {
        PLUME_UNROLL for (int k = 0; k < 5; k++) w[k] = (uint32_t)p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) | ((uint32_t)p[4 * k + 3] << 24);
    }
}

// the key of item i as the 16 memory-order words of x || y big-endian; false: no Ethereum key
PLUME_HD bool eth_load_pk(uint32_t q[16], const EthArgs& a, uint32_t i) {
    if (a.pk_format == PLUME_ETHK_PK_SEC1) {
        const uint8_t* in = a.pk + 33 * (size_t)i;
        alignas(16) uint8_t rec[64];
        const bool ok = decompress_point(rec, in) && in[0] != 0u;                       // (tag 00 decodes to the identity there)
        PLUME_UNROLL for (int k = 0; k < 16; k++) q[k] = ((const uint32_t*)rec)[k];
        return ok;
    }
    const uint8_t* in = a.pk + 64 * (size_t)i;
    if (((uintptr_t)in & 15u) == 0) {
        PLUME_UNROLL for (int k = 0; k < 4; k++) {
            const recover_quad v = ((const recover_quad*)in)[k];
            PLUME_UNROLL for (int j = 0; j < 4; j++) q[4 * k + j] = v.w[j];
        }
    } else {
        PLUME_UNROLL for (int k = 0; k < 16; k++) q[k] = (uint32_t)in[4 * k] | ((uint32_t)in[4 * k + 1] << 8) | ((uint32_t)in[4 * k + 2] << 16) | ((uint32_t)in[4 * k + 3] << 24);
    }
    uint32_t wx[8], wy[8], nz = 0;
    PLUME_UNROLL for (int k = 0; k < 8; k++) { wx[k] = bswap32(q[7 - k]); wy[k] = bswap32(q[15 - k]); nz |= wx[k] | wy[k]; }
    if (nz == 0 || !words_lt_p(wx) || !words_lt_p(wy)) return false;
    fe x, y;
    fe_from_words(x, wx); fe_from_words(y, wy);
    return affine_on_curve(x, y);
}

PLUME_HD void eth_put(const EthArgs& a, uint32_t i, const uint32_t r[16]) {
    if (!a.address) return;
    if (a.addr_format == PLUME_ETHK_ADDR_RECORD64) recover_store<64>(a.address + 64 * (size_t)i, r);
    else if (a.addr_format == PLUME_ETHK_ADDR_EIP55) recover_store<42>(a.address + 42 * (size_t)i, r);
    else recover_store<20>(a.address + 20 * (size_t)i, r);
}

// lane i of k_eth_address
PLUME_HD void eth_address_item(const EthArgs& a, uint32_t i) {
    uint32_t q[16], r[16];
    PLUME_UNROLL for (int k = 0; k < 16; k++) r[k] = 0u;
    if (!eth_load_pk(q, a, i)) {
        eth_put(a, i, r);
        if (a.status) a.status[i] = (uint8_t)PLUME_ETHK_INVALID;
        return;
    }
    uint32_t dg[8], ad[5];
    keccak256_lanes<8, 8>(dg, q);
    PLUME_UNROLL for (int k = 0; k < 5; k++) ad[k] = dg[3 + k];                           // bytes 12 .. 31
    if (a.address) {
        if (a.addr_format == PLUME_ETHK_ADDR_EIP55) {
            uint32_t hex[10], up[5];
            PLUME_UNROLL for (int k = 0; k < 10; k++) hex[k] = eth_hex4(ad[k >> 1] >> (16 * (k & 1)), 0u);
            keccak256_lanes<5, 5>(up, hex);
            PLUME_UNROLL for (int k = 0; k < 10; k++) hex[k] = eth_hex4(ad[k >> 1] >> (16 * (k & 1)), up[k >> 1] >> (16 * (k & 1)));
            r[0] = 0x7830u | (hex[0] << 16);                                            // "0x"
            PLUME_UNROLL for (int k = 1; k < 10; k++) r[k] = (hex[k - 1] >> 16) | (hex[k] << 16);
            r[10] = hex[9] >> 16;
        } else if (a.addr_format == PLUME_ETHK_ADDR_RECORD64) {
            PLUME_UNROLL for (int k = 0; k < 5; k++) r[11 + k] = ad[k];
        } else {
            PLUME_UNROLL for (int k = 0; k < 5; k++) r[k] = ad[k];
        }
        eth_put(a, i, r);
    }
    if (!a.status) return;
    uint32_t diff = 0;
    if (a.expect) {
        uint32_t e[5];
        eth_load20(e, a.expect + 20 * (size_t)i);
        PLUME_UNROLL for (int k = 0; k < 5; k++) diff |= e[k] ^ ad[k];
    }
    a.status[i] = (uint8_t)(diff == 0 ? PLUME_ETHK_MATCH : PLUME_ETHK_MISMATCH);
}

// ------------------------------------------------------------------------------------------------ ragged messages
// The digest a wallet signs (plume_eth_message_hash_batch, include/plume_hip.h): Keccak-256 of message i = msgs[msg_off[i] .. msg_off[i + 1]) itself (mode 0) or of
//     "\x19Ethereum Signed Message:\n" || decimal(len) || msg                                    (mode 1, EIP-191 version 0x45: personal_sign)
// One lane per item (k_eth_message_hash, plume_eth_kernels.hip).  The stream of P prefix bytes, len message bytes, S suffix bytes (none here: k_eth_tx_parse, plume_eth_tx.h,
// has some) and the pad (0x01 ... 0x80, rate 136) is absorbed block by block in a run-time loop; the state only ever sees literal indices, as above:
//   - a lane of the block that lies wholly inside the message is two aligned 8-byte loads and a funnel shift (the message starts at any byte), when both words lie inside
//     the msgs buffer; seventeen such tests, unrolled, XOR straight into a[0] .. a[16]
//   - every other lane that holds anything -- prefix, decimal length, the ragged head and tail of the message, the suffix, the pad -- is put together byte by byte from selects on the
//     byte's position (keccak_edge_lane) in ONE run-time loop over the block's lanes, and lands in the state through seventeen selects: there is no byte-indexed array
// Lanes of a wavefront run different block counts: the loop runs while any lane has a block left (nonce_any's rule, stated here so that this header does not need SHA-256).
// An item whose offsets msg_span rejects hashes the empty message and never reads msgs.  Every value is public: plain branches.
#define PLUME_ETHK_HASH_KECCAK256 0    // PLUME_ETH_HASH_* (include/plume_hip.h)
#define PLUME_ETHK_HASH_EIP191 1
#define PLUME_KECCAK_RATE 136u
#define PLUME_EIP191_PREFIX_LEN 26u

struct EthHashArgs {
    int mode;                         // PLUME_ETHK_HASH_*
    uint32_t n;
    const uint8_t* msgs; const uint64_t* msg_off;     // n + 1 offsets
    uint64_t msgs_bytes;
    uint8_t* hash;                    // 32 bytes per item, at any byte offset
};

PLUME_HD bool keccak_any(bool p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __any(p ? 1 : 0) != 0;
#else
    return p;
#endif
}

// the number of decimal digits of v (1 for 0)
PLUME_HD uint32_t dec_digits(uint32_t v) {
    uint32_t nd = 1, lim = 10;
    PLUME_UNROLL for (int k = 0; k < 9; k++) { nd += v >= lim ? 1u : 0u; lim *= 10u; }   // 10^1 .. 10^9: the last product still fits 32 bits
    return nd;
}
// ASCII digit d (0 = the most significant) of v, which has nd digits
PLUME_HD uint32_t dec_digit_at(uint32_t v, uint32_t nd, uint32_t d) {
    const uint32_t e = nd - 1u - d;
    uint32_t pw = 1u, p = 1u;
    PLUME_UNROLL for (uint32_t k = 1; k < 10; k++) { p *= 10u; pw = e == k ? p : pw; }
    return 0x30u + (v / pw) % 10u;
}
// eight bytes of "\x19Ethereum Signed Message:\n" from byte 8 q on, little-endian; zero past byte 25
PLUME_HD uint64_t eip191_prefix_lane(uint32_t q) {
    return q == 0 ? 0x7565726568744519ull : q == 1 ? 0x64656e676953206dull : q == 2 ? 0x6567617373654d20ull : q == 3 ? 0x0a3aull : 0ull;
}

// what one item absorbs: P prefix bytes, len bytes of the input at msg, S suffix bytes, the pad up to `last`, the final byte of the final block.  The prefix (at most 40
// bytes) and the suffix (at most 16) are little-endian lanes in named members, picked by selects: the message-hash kernel's stream is "26 + nd prefix bytes, no suffix",
// the transaction kernel's (plume_eth_tx.h) a type byte and a list header in front, the EIP-155 fields behind.
struct keccak_stream {
    const uint8_t* msg;
    uint32_t len, P, S;
    uint64_t p0, p1, p2, p3, p4, s0, s1;
    uint64_t total, last;             // P + len + S; 136 * blocks - 1
    uint64_t nblk;                    // blocks to absorb; 0: the lane only keeps its wavefront company
};
PLUME_HD void keccak_stream_init(keccak_stream& s, const uint8_t* msg, uint32_t len) {
    s.msg = msg; s.len = len; s.P = 0; s.S = 0;
    s.p0 = s.p1 = s.p2 = s.p3 = s.p4 = s.s0 = s.s1 = 0;
}
// after msg, len, P, S are set: the block count and the place of the last pad byte
PLUME_HD void keccak_stream_close(keccak_stream& s) {
    s.total = (uint64_t)s.P + s.len + s.S;
    s.nblk = s.total / PLUME_KECCAK_RATE + 1;                                            // the pad always adds a byte
    s.last = s.nblk * PLUME_KECCAK_RATE - 1;
}
PLUME_HD uint64_t keccak_prefix_lane(const keccak_stream& s, uint32_t q) { return q == 0 ? s.p0 : q == 1 ? s.p1 : q == 2 ? s.p2 : q == 3 ? s.p3 : s.p4; }
// byte `pos` of the stream
PLUME_HD uint32_t keccak_stream_byte(const keccak_stream& s, uint64_t pos) {
    if (pos < s.P) return (uint32_t)(keccak_prefix_lane(s, (uint32_t)pos >> 3) >> (8 * ((uint32_t)pos & 7))) & 0xFFu;
    const uint64_t body_end = (uint64_t)s.P + s.len;
    if (pos < body_end) return s.msg[pos - s.P];
    if (pos < s.total) {
        const uint32_t q = (uint32_t)(pos - body_end);
        return (uint32_t)((q < 8 ? s.s0 : s.s1) >> (8 * (q & 7))) & 0xFFu;
    }
    return (pos == s.total ? 0x01u : 0u) | (pos == s.last ? 0x80u : 0u);
}
// the lane of the stream that starts at byte pos (a multiple of 8), for a lane the aligned loads do not serve
PLUME_HD uint64_t keccak_edge_lane(const keccak_stream& s, uint64_t pos) {
    if (pos + 8 <= s.P) return keccak_prefix_lane(s, (uint32_t)pos >> 3);                   // wholly inside the prefix
    uint64_t v = 0;
    PLUME_NOUNROLL for (uint32_t b = 0; b < 8; b++) v |= (uint64_t)keccak_stream_byte(s, pos + b) << (8 * b);
    return v;
}
// eight message bytes at p (any alignment) by aligned loads: ok = false, and no load, unless the words that hold them lie inside [lo, hi)
PLUME_HD uint64_t keccak_load_lane(bool& ok, const uint8_t* p, const uint8_t* lo, const uint8_t* hi) {
    const uintptr_t a = (uintptr_t)p, w0 = a & ~(uintptr_t)7;
    const uint32_t sh = 8u * (uint32_t)(a & 7u);
    ok = w0 >= (uintptr_t)lo && w0 + (sh ? 16u : 8u) <= (uintptr_t)hi;
    if (!ok) return 0;
    const uint64_t x = *(const uint64_t*)w0;
    if (sh == 0) return x;
    const uint64_t y = *(const uint64_t*)(w0 + 8);
    return (x >> sh) | (y << (64u - sh));
}

// Keccak-256 of a stream: the digest as eight little-endian words in memory order.  [lo, hi) is the buffer the aligned loads may touch.  Every lane of a wavefront that
// is active at the call must make it (nblk = 0 for a lane with nothing to hash): the loop's condition is a vote.
PLUME_HD void keccak_stream_digest(uint32_t dg[8], const keccak_stream& s, const uint8_t* lo, const uint8_t* hi) {
    const uint64_t body_end = (uint64_t)s.P + s.len;
    uint64_t st[25];
    PLUME_UNROLL for (int k = 0; k < 25; k++) st[k] = 0;
    PLUME_NOUNROLL for (uint64_t blk = 0; keccak_any(blk < s.nblk); blk++) {
        if (blk < s.nblk) {
            const uint64_t base = blk * PLUME_KECCAK_RATE;
            uint32_t edge = 0;                                                           // bit j: lane j is not served by the aligned loads
            PLUME_UNROLL for (int j = 0; j < 17; j++) {
                const uint64_t pos = base + 8u * (uint32_t)j;
                bool ok = false;
                uint64_t v = 0;
                if (pos >= s.P && pos + 8 <= body_end) v = keccak_load_lane(ok, s.msg + (pos - s.P), lo, hi);
                st[j] ^= v;
                edge |= ok ? 0u : 1u << j;
            }
            PLUME_NOUNROLL for (uint32_t j = 0; j < 17; j++) {
                const uint64_t pos = base + 8u * j;
                if (!((edge >> j) & 1u) || (pos > s.total && j != 16u)) continue;         // served, or nothing but zero bytes (lane 16 may hold the last pad byte)
                const uint64_t v = keccak_edge_lane(s, pos);
                PLUME_UNROLL for (int k = 0; k < 17; k++) st[k] ^= (uint32_t)k == j ? v : 0ull;
            }
            keccak_f1600(st);
        }
    }
    PLUME_UNROLL for (int k = 0; k < 8; k++) dg[k] = (uint32_t)(st[k >> 1] >> (32 * (k & 1)));
}

// Keccak-256 of item i's stream: the digest as eight little-endian words in memory order
PLUME_HD void eth_message_digest(uint32_t dg[8], const EthHashArgs& a, uint32_t i) {
    uint64_t o0; uint32_t len;
    (void)msg_span(o0, len, a.msg_off, i, a.msgs_bytes);                                 // rejected offsets: the empty message, msgs never read
    keccak_stream s;
    keccak_stream_init(s, a.msgs + o0, len);
    if (a.mode == PLUME_ETHK_HASH_EIP191) {                                              // the fixed text, then the decimal length: bytes 26 .. 26 + nd
        const uint32_t nd = dec_digits(len);
        s.P = PLUME_EIP191_PREFIX_LEN + nd;
        s.p0 = eip191_prefix_lane(0); s.p1 = eip191_prefix_lane(1); s.p2 = eip191_prefix_lane(2); s.p3 = eip191_prefix_lane(3);
        PLUME_NOUNROLL for (uint32_t d = 0; d < nd; d++) {
            const uint64_t c = dec_digit_at(len, nd, d);
            if (d < 6) s.p3 |= c << (8 * (d + 2)); else s.p4 |= c << (8 * (d - 6));
        }
    }
    keccak_stream_close(s);
    keccak_stream_digest(dg, s, a.msgs, a.msgs + a.msgs_bytes);
}

// lane i of k_eth_message_hash
PLUME_HD void eth_message_hash_item(const EthHashArgs& a, uint32_t i) {
    uint32_t r[16];
    PLUME_UNROLL for (int k = 8; k < 16; k++) r[k] = 0u;
    eth_message_digest(r, a, i);
    recover_store<32>(a.hash + 32 * (size_t)i, r);
}

}  // namespace plume
