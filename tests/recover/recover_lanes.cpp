// k_recover_finalize's lane body (csrc/plume_recover.h) as a host loop, for tests/test_recover_lanes.py: g++ -fsanitize=address,undefined.
// usage: recover_lanes IN OUT.  IN: u32 n, u32 version, u32 format, u32 misalign (0..15), u32 present (bit k: output k is given; 0 r_point, 1 hashed_to_curve_r,
// 2 hashed_to_curve, 3 status), then per item 353 bytes: itemflag (1), pk (64), nullifier (64), c (32), R (64), Hr (64), H (64, zeros = the identity; R and Hr likewise).
// The workspace a V2 verify pipeline would have left is built from them: normalised results in the Jacobian SoA, H as row 0 of job 3i + 1's window table.
// OUT: for each output that is given, 32 guard bytes, the array, 32 guard bytes -- all pre-filled with 0xAA, the array placed `misalign` bytes behind a 16-byte
// boundary (the status array one byte further).  Every lane runs, in descending order.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "plume_recover.h"

using namespace plume;

static uint8_t* alloc16(size_t bytes) { void* p = nullptr; if (posix_memalign(&p, 16, bytes ? bytes : 1) != 0) std::abort(); return (uint8_t*)p; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t h[5];
    if (std::fread(h, 4, 5, f) != 5) return 2;
    const uint32_t n = h[0], version = h[1], format = h[2], mis = h[3] & 15u, present = h[4];
    std::vector<uint8_t> in((size_t)n * 353 + 1);
    if (n && std::fread(in.data(), 353, n, f) != n) return 2;
    std::fclose(f);
    uint8_t *pk = alloc16((size_t)n * 64), *nul = alloc16((size_t)n * 64), *c = alloc16((size_t)n * 32);
    std::vector<uint8_t> itemflags(n + 1), jobflags(3 * (size_t)n + 1), resinf(2 * (size_t)n + 1);
    uint32_t* tab = (uint32_t*)alloc16((size_t)n * 3 * PLUME_TAB_WORDS * 4);
    std::memset(tab, 0x5C, (size_t)n * 3 * PLUME_TAB_WORDS * 4);
    std::vector<uint32_t> res((size_t)PLUME_JAC_WORDS * 2 * n + 1, 0x5C5C5C5Cu);
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t* it = in.data() + (size_t)i * 353;
        itemflags[i] = it[0];
        std::memcpy(pk + 64 * (size_t)i, it + 1, 64); std::memcpy(nul + 64 * (size_t)i, it + 65, 64); std::memcpy(c + 32 * (size_t)i, it + 129, 32);
        alignas(16) uint8_t rec[64];
        for (int k = 0; k < 2; k++) {                                  // R, Hr: normalised results of tasks 2i, 2i + 1
            std::memcpy(rec, it + 161 + 64 * k, 64);
            jac p;
            const uint32_t fl = reload_affine_be(p.x, p.y, rec);
            p.z = fe_small(1); p.inf = fl == PLUME_JOB_INF ? 1 : 0;
            if (p.inf) { p.x = fe_small(7); p.y = fe_small(9); }         // an identity result's coordinates are whatever the chain left
            st_jac_soa(res.data(), 2 * (size_t)n, 2 * (size_t)i + (size_t)k, p);
            resinf[2 * (size_t)i + (size_t)k] = (uint8_t)p.inf;
        }
        std::memcpy(rec, it + 289, 64);
        fe hx, hy;
        const uint32_t fl = reload_affine_be(hx, hy, rec);
        jobflags[3 * (size_t)i] = jobflags[3 * (size_t)i + 2] = (uint8_t)(PLUME_JOB_OK | PLUME_JOB_AFFINE);
        jobflags[3 * (size_t)i + 1] = (uint8_t)(fl == PLUME_JOB_INF ? PLUME_JOB_INF : PLUME_JOB_OK);
        if (fl == PLUME_JOB_INF) { hx = fe_gx(); hy = fe_gy(); }        // the table of an identity base is built from G (tab_base)
        st_tab_entry(tab + (3 * (size_t)i + 1) * PLUME_TAB_WORDS, hx, hy, fe_zero());
    }
    RecoverArgs a;
    std::memset(&a, 0, sizeof a);
    a.version = (int)version; a.format = (int)format; a.n = n; a.pk = pk; a.nul = nul; a.c = c;
    a.itemflags = itemflags.data(); a.jobflags = jobflags.data(); a.tab = tab; a.res = res.data(); a.resinf = resinf.data();
    const size_t W = recover_width((int)format);
    uint8_t *raw[4], *arr[4];
    size_t len[4];
    for (int k = 0; k < 4; k++) {
        len[k] = (size_t)n * (k == 3 ? 1 : W);
        const size_t m = (mis + (k == 3 ? 1 : 0)) & 15u;
        raw[k] = alloc16(32 + 16 + len[k] + 32 + 16);                    // exact: ASan sees a store one byte past the guards
        std::memset(raw[k], 0xAA, 32 + 16 + len[k] + 32 + 16);
        arr[k] = raw[k] + 32 + m;
    }
    a.rpt = (present & 1u) ? arr[0] : nullptr; a.hr = (present & 2u) ? arr[1] : nullptr; a.h = (present & 4u) ? arr[2] : nullptr; a.status = (present & 8u) ? arr[3] : nullptr;
    for (uint32_t i = n; i-- > 0;) recover_finalize(a, i);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    for (int k = 0; k < 4; k++) {
        if (!(present & (1u << k))) { for (size_t b = 0; b < 32 + 16 + len[k] + 32 + 16; b++) if (raw[k][b] != 0xAA) return 3; continue; }
        std::fwrite(arr[k] - 32, 1, 32 + len[k] + 32, o);
    }
    std::fclose(o);
    std::free(pk); std::free(nul); std::free(c); std::free(tab);
    for (int k = 0; k < 4; k++) std::free(raw[k]);
    std::printf("recover_lanes ok\n");
    return 0;
}
