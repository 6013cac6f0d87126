// Recovery of a signature's V1-specific points (plume_recover_batch, include/plume_hip.h): r_point = s G - c pk and hashed_to_curve_r = s H - c nullifier are what the
// verifier's V2 pipeline computes on its way to the challenge (circuits/circom/verify_nullifier.circom:140-222 publishes them as plume_v2's outputs).  The call runs that
// pipeline unchanged -- ingest, scalars, tables, the multi-scalar kernel and its redo launch, the batched conversion to affine -- and ends it with this file's lane body in
// place of verify_finalize: one lane per item reads the two normalised results and affine H (row 0 of H's window table), hashes them the way the requested version does,
// and WRITES the three points in the requested record format, plus a status byte.
//     status 3 (PLUME_RECOVER_INVALID)   the ingest stage rejected the item (itemflags): every record of the item is all zero
//     status 1 (PLUME_RECOVER_MATCH)     c == SHA256(enc(nullifier), enc(R), enc(Hr)) mod n (version 2) / SHA256 over (G, pk, H, nullifier, R, Hr) (version 1)
//     status 0 (PLUME_RECOVER_MISMATCH)  the points are written all the same
// Every value here is public: plain branches.  Records are written with vector stores in plain C++: a 64-byte record at a 16-byte aligned address is four 16-byte stores;
// anything else (the 33-byte records, a 64-byte array the caller placed at a 4-byte boundary) is byte stores up to the first 16-byte boundary inside the record, 16-byte
// stores for the whole quads that follow (one or two of a 33-byte record), byte stores for the rest.  A lane touches only its own record's bytes.
// Compiles as plain C++ for the host (tests/recover, tests/hostsim), like the other headers.
#pragma once
#include "plume_stages.h"

#define PLUME_RCV_MISMATCH 0u          // PLUME_RECOVER_* (include/plume_hip.h)
#define PLUME_RCV_MATCH 1u
#define PLUME_RCV_INVALID 3u
#define PLUME_RCV_FMT_AFFINE64 0       // 64 B x || y big-endian, zeros = identity
#define PLUME_RCV_FMT_SEC1 1           // 33 B 02|03 || x, identity = 00 + 32 zero bytes
#define PLUME_RCV_FMT_REGISTERS 2      // 64 B = uint64_t[2][4]: x then y as four little-endian registers, zeros = identity

namespace plume {

struct RecoverArgs {
    int version;              // 1 | 2: which hash the status compares c with
    int format;               // PLUME_RCV_FMT_*
    uint32_t n;
    const uint8_t *pk, *nul, *c;      // the caller's arrays (the ingest stage validated them: itemflags)
    // what the V2 verify pipeline left in the workspace (VerifyArgs of the same slice)
    const uint8_t* itemflags;         // n
    const uint8_t* jobflags;          // 3n: job 3i + 1 = H of item i
    const uint32_t* tab;              // 3n window tables: row 0 = the base, affine
    const uint32_t* res;              // Jacobian SoA over 2n tasks, normalised: X, Y are the affine coordinates of R (task 2i) and Hr (task 2i + 1)
    const uint8_t* resinf;            // 2n
    // outputs, each optional
    uint8_t *rpt, *hr, *h;            // recover_width(format) bytes per item
    uint8_t* status;                  // 1 byte per item
};

PLUME_HD uint32_t recover_width(int format) { return format == PLUME_RCV_FMT_SEC1 ? 33u : 64u; }

struct alignas(16) recover_quad { uint32_t w[4]; };

// The record of a point in memory order: N = 16 words (64 bytes) or 9 words whose first 33 bytes count.  x, y canonical little-endian words; inf: the zero record
PLUME_HD void recover_record(uint32_t r[16], int format, const uint32_t xw[8], const uint32_t yw[8], bool inf) {
    PLUME_UNROLL for (int k = 0; k < 16; k++) r[k] = 0u;
    if (inf) return;
    if (format == PLUME_RCV_FMT_REGISTERS) {
        PLUME_UNROLL for (int k = 0; k < 8; k++) { r[k] = xw[k]; r[8 + k] = yw[k]; }
    } else if (format == PLUME_RCV_FMT_SEC1) {
        // byte 0 = tag, bytes 1 .. 32 = x big-endian: word k holds bytes 4k .. 4k + 3
        uint32_t be[9];
        PLUME_UNROLL for (int k = 0; k < 8; k++) be[k] = bswap32(xw[7 - k]);          // memory-order words of x big-endian
        be[8] = 0u;
        r[0] = (2u + (yw[0] & 1u)) | (be[0] << 8);
        PLUME_UNROLL for (int k = 1; k < 9; k++) r[k] = (be[k - 1] >> 24) | (be[k] << 8);
    } else {
        PLUME_UNROLL for (int k = 0; k < 8; k++) { r[k] = bswap32(xw[7 - k]); r[8 + k] = bswap32(yw[7 - k]); }
    }
}

// W bytes of the record r to a destination LEAD bytes in front of a 16-byte boundary: LEAD byte stores, the whole quads that follow, byte stores for the rest.  LEAD and W
// are template arguments so that every index into r is a constant once the loops are unrolled: the record stays in registers.  (A first version walked the record with a
// run-time byte offset; the compiler then kept it in memory -- 80 B of scratch per lane and a 16 KiB LDS array per workgroup.)
template <int LEAD, int W>
PLUME_HD void recover_store_at(uint8_t* dst, const uint32_t* r) {
    constexpr int NQ = (W - LEAD) / 16, TAIL = LEAD + 16 * NQ;
    PLUME_UNROLL for (int b = 0; b < LEAD; b++) dst[b] = (uint8_t)(r[b >> 2] >> (8 * (b & 3)));
    PLUME_UNROLL for (int q = 0; q < NQ; q++) {
        recover_quad v;
        PLUME_UNROLL for (int j = 0; j < 4; j++) {
            const int b = LEAD + 16 * q + 4 * j, sh = 8 * (b & 3);                      // bytes [b, b + 4) of the record: b + 4 <= W <= 64
            v.w[j] = sh == 0 ? r[b >> 2] : ((r[b >> 2] >> sh) | (r[((b >> 2) + 1) & 15] << ((32 - sh) & 31)));
        }
        *reinterpret_cast<recover_quad*>(dst + LEAD + 16 * q) = v;
    }
    PLUME_UNROLL for (int b = TAIL; b < W; b++) dst[b] = (uint8_t)(r[b >> 2] >> (8 * (b & 3)));
}
// ... for any destination: LEAD = 0 with W = 64 is four 16-byte stores, what arrays from hipMalloc, torch and numpy get
template <int W>
PLUME_HD void recover_store(uint8_t* dst, const uint32_t* r) {
    switch ((uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u)) {
        case 0: recover_store_at<0, W>(dst, r); break;
        case 1: recover_store_at<1, W>(dst, r); break;
        case 2: recover_store_at<2, W>(dst, r); break;
        case 3: recover_store_at<3, W>(dst, r); break;
        case 4: recover_store_at<4, W>(dst, r); break;
        case 5: recover_store_at<5, W>(dst, r); break;
        case 6: recover_store_at<6, W>(dst, r); break;
        case 7: recover_store_at<7, W>(dst, r); break;
        case 8: recover_store_at<8, W>(dst, r); break;
        case 9: recover_store_at<9, W>(dst, r); break;
        case 10: recover_store_at<10, W>(dst, r); break;
        case 11: recover_store_at<11, W>(dst, r); break;
        case 12: recover_store_at<12, W>(dst, r); break;
        case 13: recover_store_at<13, W>(dst, r); break;
        case 14: recover_store_at<14, W>(dst, r); break;
        default: recover_store_at<15, W>(dst, r); break;
    }
}

PLUME_HD void recover_put(uint8_t* base, size_t i, int format, fe x, fe y, bool inf) {
    if (!base) return;
    uint32_t xw[8], yw[8], r[16];
    fe_normalize(x); fe_normalize(y);
    fe_to_words(xw, x); fe_to_words(yw, y);
    recover_record(r, format, xw, yw, inf);
    if (format == PLUME_RCV_FMT_SEC1) recover_store<33>(base + 33 * i, r); else recover_store<64>(base + 64 * i, r);
}

// lane i of k_recover_finalize
PLUME_HD void recover_finalize(const RecoverArgs& a, uint32_t i) {
    const size_t nt = 2 * (size_t)a.n;
    if (a.itemflags[i]) {                                                               // no value of the reference's types: zero records, never a point
        const fe z = fe_zero();
        recover_put(a.rpt, i, a.format, z, z, true);
        recover_put(a.hr, i, a.format, z, z, true);
        recover_put(a.h, i, a.format, z, z, true);
        if (a.status) a.status[i] = (uint8_t)PLUME_RCV_INVALID;
        return;
    }
    jac rc, hc;
    ld_jac_soa(rc, a.res, nt, 2 * (size_t)i); rc.inf = a.resinf[2 * (size_t)i];
    ld_jac_soa(hc, a.res, nt, 2 * (size_t)i + 1); hc.inf = a.resinf[2 * (size_t)i + 1];
    recover_put(a.rpt, i, a.format, rc.x, rc.y, rc.inf != 0);
    recover_put(a.hr, i, a.format, hc.x, hc.y, hc.inf != 0);
    // affine H = row 0 of H's table; an identity H has no table (its job was built from G)
    const size_t jh = 3 * (size_t)i + 1;
    const bool hinf = job_state(a.jobflags[jh]) == PLUME_JOB_INF;
    fe Hx, Hy;
    ld_tab_xy(Hx, Hy, a.tab + jh * PLUME_TAB_WORDS, false);
    recover_put(a.h, i, a.format, Hx, Hy, hinf);
    if (!a.status) return;
    fe pkx, pky, nx, ny;
    const uint32_t fpk = reload_affine_be(pkx, pky, a.pk + 64 * (size_t)i);             // validated by verify_ingest_h2c (itemflags == 0 here)
    const uint32_t fnul = reload_affine_be(nx, ny, a.nul + 64 * (size_t)i);
    sc c;
    sc_from_be_aligned(c, a.c + 32 * (size_t)i);
    uint32_t dg[8];
    enc_pt pts[6];
    pts[3] = enc_of(nx, ny, fnul == PLUME_JOB_INF);
    pts[4] = enc_of(rc.x, rc.y, rc.inf != 0);
    pts[5] = enc_of(hc.x, hc.y, hc.inf != 0);
    if (a.version == 1) {
        pts[0] = enc_of(fe_gx(), fe_gy(), false);
        pts[1] = enc_of(pkx, pky, fpk == PLUME_JOB_INF);
        pts[2] = enc_of(Hx, Hy, hinf);
        c_hash<6>(dg, pts);                                                             // rust-k256/src/lib.rs:128-135
    } else {
        c_hash<3>(dg, pts + 3);                                                         // lib.rs:139-143
    }
    sc cc; bool canon;
    sc_from_digest_words(cc, dg, canon);                                                // Scalar::reduce
    uint32_t diff = 0;
    PLUME_UNROLL for (int k = 0; k < 8; k++) diff |= cc.v[k] ^ c.v[k];
    a.status[i] = (uint8_t)(diff == 0 ? PLUME_RCV_MATCH : PLUME_RCV_MISMATCH);
}

}  // namespace plume
