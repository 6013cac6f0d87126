// k_sign_release's lane body (csrc/plume_selfcheck.h) as a host loop, for tests/test_selfcheck_lanes.py: g++ -fsanitize=address,undefined.
// usage: release_lanes IN OUT.  IN: u32 n, u32 out33, u32 has_pk, u32 misalign (0..15), then the staging -- pk, nul, c, s, rpt, hr (64, 64, 32, 32, 64, 64 bytes per
// item), status (n), verdict (n).  OUT: for each of the seven caller arrays that exists, 32 guard bytes, the array, 32 guard bytes -- all pre-filled with 0xAA, the array
// placed `misalign` bytes behind a 16-byte boundary (the status array one byte further).  Every lane of every record runs, in descending order, plus lanes past the end.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "plume_selfcheck.h"

using namespace plume;

static uint8_t* alloc16(size_t bytes) { void* p = nullptr; if (posix_memalign(&p, 16, bytes ? bytes : 1) != 0) std::abort(); return (uint8_t*)p; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t h[4];
    if (std::fread(h, 4, 4, f) != 4) return 2;
    const uint32_t n = h[0], out33 = h[1], has_pk = h[2], mis = h[3] & 15u;
    static const uint32_t SW[6] = {64, 64, 32, 32, 64, 64};
    std::vector<uint8_t*> stage(6);
    for (int k = 0; k < 6; k++) {
        stage[k] = alloc16((size_t)n * SW[k]);
        if (n && std::fread(stage[k], SW[k], n, f) != n) return 2;
    }
    std::vector<uint8_t> st(n + 1), vd(n + 1);
    if (n && (std::fread(st.data(), 1, n, f) != n || std::fread(vd.data(), 1, n, f) != n)) return 2;
    std::fclose(f);
    ReleaseArgs a;
    std::memset(&a, 0, sizeof a);
    a.n = n; a.out33 = (int)out33; a.stage_status = st.data(); a.verdict = vd.data();
    for (int k = 0; k < 6; k++) a.stage[k] = stage[k];
    uint8_t* raw[7];
    size_t len[7];
    uint8_t* arr[7];
    for (int k = 0; k < 7; k++) {
        len[k] = (size_t)n * release_out_width(a, k);
        const size_t m = (mis + (k == 6 ? 1 : 0)) & 15u;
        raw[k] = alloc16(32 + 16 + len[k] + 32 + 16);   // exact: ASan sees a store one byte past the guards
        std::memset(raw[k], 0xAA, 32 + 16 + len[k] + 32 + 16);
        arr[k] = raw[k] + 32 + m;
        if (k < 6) a.out[k] = (k == 0 && !has_pk) ? nullptr : arr[k]; else a.status = arr[k];
    }
    for (int k = 0; k < PLUME_RELEASE_RECORDS; k++) {
        const size_t q = release_quads(a, k);
        for (size_t g = q + 300; g-- > 0;) sign_release_lane(a, k, g);
    }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    for (int k = 0; k < 7; k++) {
        if (k == 0 && !has_pk) { for (size_t b = 0; b < 32 + 16 + len[k] + 32 + 16; b++) if (raw[k][b] != 0xAA) return 3; continue; }
        std::fwrite(arr[k] - 32, 1, 32 + len[k] + 32, o);
    }
    std::fclose(o);
    for (int k = 0; k < 6; k++) std::free(stage[k]);
    for (int k = 0; k < 7; k++) std::free(raw[k]);
    std::printf("release_lanes ok\n");
    return 0;
}
