// PBKDF2-HMAC-SHA512 (RFC 8018), one output block, for a batch (plume_pbkdf2_sha512_batch, include/plume_hip.h): what BIP-39 makes a seed of a mnemonic sentence with.
//     U_1 = HMAC(P, S || 00000001),  U_j = HMAC(P, U_{j-1}),  T_1 = U_1 ^ U_2 ^ .. ^ U_c;   out = T_1[0 : dklen],  dklen <= 64
//     P: the password of the item, any length (longer than 128 bytes: replaced by its SHA-512, as HMAC says); S: the salt, salt_len bytes (the same length for every
//     item), with PLUME_KDFK_BIP39 the eight bytes "mnemonic" in front of it
// One lane per item.  The kernels (plume_kdf_kernels.hip):
//   kdf_key_item     the password read once: hashed first when longer than 128 bytes (one trip per block: a wavefront takes as long as its longest item), the midstates
//                    ist, ost behind K ^ ipad and K ^ opad, then U_1 (one to three inner blocks: uniform over the launch, salt_len is).  ist, ost, U, T = U go to the
//                    context's workspace, 32 words of 64 bits per item in the layout [32][n]: a wavefront's loads and stores of one word are contiguous
//   kdf_iter_item    `iters` rounds of U = HMAC(P, U), T ^= U from the workspace and back: two compressions of one fixed shape each -- a 64-byte message behind one
//                    absorbed block, w[8] the padding bit, w[9 .. 14] zero, w[15] the length.  The host enqueues it in slices (PLUME_KDF_SLICE)
//   kdf_finish_item  T[0 : dklen] big-endian into the caller's record, the status
//     status 0                                   derived
//     status 128 (PLUME_STATUS_KDF_BAD_INPUT)    pw_off[i + 1] < pw_off[i] or pw_off[i + 1] > pw_bytes: the item reads no byte of pw and its record is all zero
// What the lanes branch on and form addresses from is public: the offsets (so the lengths), salt_len, the flags, the iteration count, dklen.  No branch and no address
// depends on a byte of a password, a salt, a midstate or U / T.  A refused item carries zeros through the workspace; finish tells it by its offsets again.
// Compiles as plain C++ for the host (tests/kdf), like the other headers.
#pragma once
#include "plume_sha512.h"

#define PLUME_KDFK_BIP39 1             // PLUME_KDF_BIP39: flags bit 0
#define PLUME_KDFK_SHARED_SALT 2       // PLUME_KDF_SHARED_SALT: flags bit 1
#define PLUME_KDFK_MAX_SALT 256        // PLUME_KDF_MAX_SALT
#define PLUME_ST_KDF_BAD_INPUT 128u    // PLUME_STATUS_KDF_BAD_INPUT
#define PLUME_KDFK_WS_WORDS 32         // workspace per item, 64-bit words: ist, ost, U, T
// the rounds one k_kdf_iter dispatch runs at most: the host enqueues a derivation's remaining iterations in slices of this many, so that no single dispatch of a
// 2^20-item call runs for the whole derivation.  Per slice an item moves its 32 words twice, 512 B against 512 compressions
#define PLUME_KDF_SLICE 256

namespace plume {

struct KdfArgs {
    int flags;                        // PLUME_KDFK_*
    uint32_t n, salt_len, dklen;
    uint32_t iters;                   // kdf_iter_item: the rounds of this launch
    // the caller's arrays, at any byte offset (pw_off 8-byte aligned)
    const uint8_t* pw;                // the passwords, item i's at pw_off[i] .. pw_off[i + 1]
    const uint64_t* pw_off;           // n + 1
    uint64_t pw_bytes;
    const uint8_t* salt;              // salt_len bytes per item, one record with SHARED_SALT; may be null when salt_len is 0
    uint8_t* out;                     // dklen bytes per item
    uint8_t* status;                  // 1 B per item
    // workspace
    uint64_t* ws;                     // [32][n] (wiped behind finish)
};

// whether item i's offsets are sound; its password is pw[lo .. lo + len), len 0 for a refused item
PLUME_HD bool kdf_item_ok(const KdfArgs& a, uint32_t i, uint64_t& lo, uint64_t& len) {
    lo = a.pw_off[i];
    const uint64_t hi = a.pw_off[i + 1];
    const bool ok = hi >= lo && hi <= a.pw_bytes;
    len = ok ? hi - lo : 0;
    return ok;
}

// the outer hash over the 64-byte inner digest (in place), from the midstate ost
PLUME_HD void kdf_outer(uint64_t io[8], const uint64_t ost[8]) {
    uint64_t w[16];
    PLUME_UNROLL for (int j = 0; j < 16; j++) w[j] = j < 8 ? io[j] : 0ull;
    w[8] = 0x8000000000000000ull; w[15] = (128 + 64) * 8;
    PLUME_UNROLL for (int j = 0; j < 8; j++) io[j] = ost[j];
    sha512_compress_grouped(io, w);
}

// lane i of k_kdf_key
PLUME_HD void kdf_key_item(const KdfArgs& a, uint32_t i) {
    uint64_t lo, len;
    const bool ok = kdf_item_ok(a, i, lo, len);
    uint64_t* const ws = a.ws + i;
    if (!ok) {
        PLUME_UNROLL for (int j = 0; j < PLUME_KDFK_WS_WORDS; j++) ws[(size_t)j * a.n] = 0;
        return;
    }
    const uint8_t* const pw = a.pw + lo;
    uint64_t key[16];                                                          // the key block: the password, or its digest, zero beyond
    if (len > 128) {
        uint64_t dg[8];
        sha512_init(dg);
        sha512_absorb(dg, 0, len, [&](uint64_t pos) -> uint64_t { return pw[pos]; });
        PLUME_UNROLL for (int j = 0; j < 16; j++) key[j] = j < 8 ? dg[j] : 0ull;
    } else {
        PLUME_UNROLL for (int j = 0; j < 16; j++) {
            uint64_t word = 0;
            PLUME_UNROLL for (int q = 0; q < 8; q++) {
                const uint32_t pos = 8 * j + q;
                uint64_t v = 0;
                if (pos < len) v = pw[pos];
                word = (word << 8) | v;
            }
            key[j] = word;
        }
    }
    uint64_t ist[8], ost[8], w[16];
    sha512_init(ist);
    PLUME_UNROLL for (int j = 0; j < 16; j++) w[j] = key[j] ^ 0x3636363636363636ull;
    sha512_compress_grouped(ist, w);
    sha512_init(ost);
    PLUME_UNROLL for (int j = 0; j < 16; j++) w[j] = key[j] ^ 0x5c5c5c5c5c5c5c5cull;
    sha512_compress_grouped(ost, w);
    // U_1 = HMAC(P, ["mnemonic"] || salt || 00 00 00 01)
    const uint32_t pre = (a.flags & PLUME_KDFK_BIP39) ? 8u : 0u, slen = a.salt_len;
    const uint8_t* const salt = a.salt + ((a.flags & PLUME_KDFK_SHARED_SALT) ? 0 : (size_t)slen * i);
    uint64_t u[8];
    PLUME_UNROLL for (int j = 0; j < 8; j++) u[j] = ist[j];
    sha512_absorb(u, 128, (uint64_t)pre + slen + 4, [&](uint64_t pos) -> uint64_t {
        if (pos < pre) return (0x6d6e656d6f6e6963ull >> (56 - 8 * (uint32_t)pos)) & 0xFFu;   // "mnemonic"
        if (pos < pre + slen) return salt[pos - pre];
        return pos == (uint64_t)pre + slen + 3 ? 1u : 0u;                                    // the block index, big-endian
    });
    kdf_outer(u, ost);
    PLUME_UNROLL for (int j = 0; j < 8; j++) {
        ws[(size_t)j * a.n] = ist[j]; ws[(size_t)(8 + j) * a.n] = ost[j]; ws[(size_t)(16 + j) * a.n] = u[j]; ws[(size_t)(24 + j) * a.n] = u[j];
    }
}

// lane i of k_kdf_iter: a.iters rounds
PLUME_HD void kdf_iter_item(const KdfArgs& a, uint32_t i) {
    uint64_t* const ws = a.ws + i;
    uint64_t ist[8], ost[8], u[8], t[8];
    PLUME_UNROLL for (int j = 0; j < 8; j++) {
        ist[j] = ws[(size_t)j * a.n]; ost[j] = ws[(size_t)(8 + j) * a.n]; u[j] = ws[(size_t)(16 + j) * a.n]; t[j] = ws[(size_t)(24 + j) * a.n];
    }
    PLUME_NOUNROLL for (uint32_t r = 0; r < a.iters; r++) {
        uint64_t w[16];
        PLUME_UNROLL for (int j = 0; j < 16; j++) w[j] = j < 8 ? u[j] : 0ull;
        w[8] = 0x8000000000000000ull; w[15] = (128 + 64) * 8;
        PLUME_UNROLL for (int j = 0; j < 8; j++) u[j] = ist[j];
        sha512_compress_grouped(u, w);
        kdf_outer(u, ost);
        PLUME_UNROLL for (int j = 0; j < 8; j++) t[j] ^= u[j];
    }
    PLUME_UNROLL for (int j = 0; j < 8; j++) { ws[(size_t)(16 + j) * a.n] = u[j]; ws[(size_t)(24 + j) * a.n] = t[j]; }
}

// lane i of k_kdf_finish
PLUME_HD void kdf_finish_item(const KdfArgs& a, uint32_t i) {
    uint64_t lo, len;
    const bool ok = kdf_item_ok(a, i, lo, len);
    const uint64_t* const ws = a.ws + i;
    uint8_t* const out = a.out + (size_t)a.dklen * i;
    PLUME_UNROLL for (int j = 0; j < 8; j++) {
        const uint64_t t = ok ? ws[(size_t)(24 + j) * a.n] : 0ull;
        PLUME_UNROLL for (int q = 0; q < 8; q++)
            if ((uint32_t)(8 * j + q) < a.dklen) out[8 * j + q] = (uint8_t)(t >> (56 - 8 * q));
    }
    a.status[i] = ok ? 0 : (uint8_t)PLUME_ST_KDF_BAD_INPUT;
}

}  // namespace plume
