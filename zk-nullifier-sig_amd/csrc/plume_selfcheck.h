// The signer's self-check gate (plume_set_sign_selfcheck): with the check on, the sign kernels write the six records of every item into context-owned staging, always in
// the 64-byte form; the verifier's stages recompute both group equations and the challenge from those records (verify_non_zk); and k_sign_release -- this file's lane body --
// is the only thing that writes the caller's arrays: the records as staged (or SEC1-compressed, 02|03 || x, identity 00 + zeros), or zeros with status 8 for an item whose
// own status is 0 and whose verdict is not 1.  An item the signer itself flagged (status != 0) is released as staged, with that status.
// A pure copy: every value here is public (a withheld c, s is secret only in that it must not be RELEASED), so plain branches and vector stores, no masked selects.
// Work is cut by DESTINATION: lane g of record k owns the 16-byte quad number g of record k's caller array, counted from the array's address rounded down to 16 bytes, so
// consecutive lanes store consecutive quads whatever the record's stride (64, 33, 32 or the status byte) and whatever the array's alignment (the ABI promises 4 bytes for the
// 32/64-byte arrays, nothing for the 33-byte ones).  Quads that lie wholly inside the array are one 16-byte store; the at most two that straddle its ends are byte stores.
// When destination and staging are both 16-byte aligned and the record is not compressed the quad is one 16-byte load as well; a destination that is only 4-byte aligned
// takes four dword loads; everything else -- the 33-byte records, the status bytes, a 32/64-byte array at an odd address -- is gathered byte by byte, each byte looking up its
// item's status and verdict again, and the lane that owns a compressed record's tag byte reads the record's 64 staged bytes to tell the identity.  That path moves 0.14 GB of
// the 0.8 GB per 2^20 items in the SEC1 form and is what a caller with odd-address 64-byte arrays pays throughout; arrays from hipMalloc, torch or numpy never take it for
// the 64- and 32-byte records.
// Compiles as plain C++ for the host (tests/selfcheck), like the other headers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "plume_field.h"

#define PLUME_ST_SELFCHECK_FAILED 8u   // PLUME_STATUS_SELFCHECK_FAILED (include/plume_hip.h)
#define PLUME_RELEASE_RECORDS 7        // pk, nullifier, c, s, r_point, hashed_to_curve_r, status

namespace plume {

struct ReleaseArgs {
    uint32_t n;
    int out33;                   // 1: the four point records leave SEC1-compressed, stride 33
    const uint8_t* stage[6];     // staged records: pk, nul, c, s, rpt, hr -- 64, 64, 32, 32, 64, 64 bytes per item, 16-byte aligned arrays
    const uint8_t* stage_status; // the signer's own status, 1 B / item
    const uint8_t* verdict;      // the check's verdict, 1 B / item: 1 = the records verify
    uint8_t* out[6];             // the caller's arrays, same order; out[0] (pk) may be NULL
    uint8_t* status;             // the caller's status array
};

// bytes per item of record k in the staging / in the caller's array
PLUME_HD uint32_t release_stage_width(int k) { return (k == 2 || k == 3) ? 32u : 64u; }
PLUME_HD uint32_t release_out_width(const ReleaseArgs& a, int k) { return k == 6 ? 1u : (k == 2 || k == 3) ? 32u : (a.out33 ? 33u : 64u); }
// number of 16-byte quads record k's caller array touches (0 for an absent array): what the launcher sizes its grid by
PLUME_HD size_t release_quads(const ReleaseArgs& a, int k) {
    const uint8_t* dst = k == 6 ? a.status : a.out[k];
    if (!dst || !a.n) return 0;
    const size_t lead = (size_t)((uintptr_t)dst & 15u);
    return (lead + (size_t)a.n * release_out_width(a, k) + 15) / 16;
}

PLUME_HD bool release_withheld(const ReleaseArgs& a, size_t item) { return a.stage_status[item] == 0 && a.verdict[item] != 1; }

// byte b of record k's caller array
PLUME_HD uint8_t release_byte(const ReleaseArgs& a, int k, size_t b) {
    if (k == 6) return a.stage_status[b] ? a.stage_status[b] : (a.verdict[b] == 1 ? (uint8_t)0 : (uint8_t)PLUME_ST_SELFCHECK_FAILED);
    const uint32_t W = release_out_width(a, k);
    const size_t item = b / W;
    const uint32_t o = (uint32_t)(b - item * W);
    if (release_withheld(a, item)) return 0;
    if (W != 33) return a.stage[k][item * W + o];
    const uint8_t* p = a.stage[k] + 64 * item;
    if (o) return p[o - 1];
    uint32_t nz = 0;                                                            // the tag: the staged affine record is all zero exactly for the identity (store_affine_be)
    PLUME_UNROLL for (int j = 0; j < 16; j++) { uint32_t w; memcpy(&w, p + 4 * j, 4); nz |= w; }
    return nz ? (uint8_t)(2u + (p[63] & 1u)) : (uint8_t)0;
}

struct alignas(16) release_quad { uint32_t w[4]; };

// lane g of record k (0 .. PLUME_RELEASE_RECORDS - 1)
PLUME_HD void sign_release_lane(const ReleaseArgs& a, int k, size_t g) {
    uint8_t* dst = k == 6 ? a.status : a.out[k];
    if (g >= release_quads(a, k)) return;
    const uint32_t W = release_out_width(a, k);
    const size_t total = (size_t)a.n * W, lead = (size_t)((uintptr_t)dst & 15u);
    const size_t q0 = 16 * g, q1 = q0 + 16;                                     // the quad, in bytes from the rounded-down address
    const size_t lo = q0 < lead ? 0 : q0 - lead, hi = (q1 - lead < total) ? q1 - lead : total;   // ... and the array bytes [lo, hi) it holds (q1 > lead always)
    const bool full = q0 >= lead && q1 - lead <= total;
    if (full && lead == 0 && k < 6 && W != 33) {                                // aligned, uncompressed: one item, one 16-byte load
        release_quad v;
        if (release_withheld(a, lo / W)) v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0u;
        else v = *reinterpret_cast<const release_quad*>(a.stage[k] + lo);
        *reinterpret_cast<release_quad*>(dst + lo) = v;
        return;
    }
    if (full && (lead & 3u) == 0 && k < 6 && W != 33) {                         // 4-byte aligned (all the ABI promises), uncompressed: four dword loads; the quad may span two items
        release_quad v;
        PLUME_UNROLL for (int j = 0; j < 4; j++) {
            const size_t b = lo + 4 * j;
            uint32_t w = 0;
            if (!release_withheld(a, b / W)) memcpy(&w, a.stage[k] + b, 4);
            v.w[j] = w;
        }
        *reinterpret_cast<release_quad*>(dst + lo) = v;
        return;
    }
    if (full) {                                                                 // compressed records, the status bytes, arrays at odd addresses: gathered byte by byte
        release_quad v;
        PLUME_UNROLL for (int j = 0; j < 4; j++) {
            uint32_t w = 0;
            PLUME_UNROLL for (int e = 0; e < 4; e++) w |= (uint32_t)release_byte(a, k, lo + 4 * j + e) << (8 * e);
            v.w[j] = w;
        }
        *reinterpret_cast<release_quad*>(dst + lo) = v;
        return;
    }
    for (size_t b = lo; b < hi; b++) dst[b] = release_byte(a, k, b);
}

}  // namespace plume
