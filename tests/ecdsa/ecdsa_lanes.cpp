// The lane bodies of plume_ecdsa_recover_batch (csrc/plume_ecdsa.h) as host loops, for tests/test_ecdsa_lanes.py: g++ -fsanitize=address,undefined, -DPLUME_COMB_W=10
// (a CPU cannot build the 15 x 2^17-row comb per test run; the lane bodies are the same for every width).
// usage: ecdsa_lanes scinv IN OUT    IN: u32 count, count scalars of 32 big-endian bytes (canonical, non-zero).  OUT: their inverses mod n by sc_inv, the same way.
//        ecdsa_lanes feinv IN OUT    the same for the field: fe_inv (plume_field.h), values below p
//        ecdsa_lanes recover IN OUT  IN: u32 n, u32 flags, u32 pk_format, u32 addr_format, u32 misalign (0..15), u32 present (bit 0: pk is given, bit 1: address, bit 2:
//                                    status, bit 3: expect), then n hashes, n r, n s (32 bytes each), n v (1 byte), then (bit 3) n expected addresses of 20 bytes.
// recover runs the stages lane by lane the way the kernels do: ecdsa_prepare for every item (descending), the table builder three jobs per lane (one shared inversion),
// ecdsa_mul<false> for every item with a private digit area, ecdsa_mul<true> for whatever that filed, normalize_points eight per lane, ecdsa_finalize.
// Every caller array lies between 32 guard bytes pre-filled with 0xAA, `misalign` bytes behind a 16-byte boundary (r one byte further, s two, v three, expect one, status
// two).  OUT: u32 number of items the unchecked chain filed, then for each output that is given, the 32 guard bytes, the array, 32 guard bytes.  The harness itself checks
// that the inputs and their guards are unchanged and that an output that is not given was never written.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "plume_ecdsa.h"

using namespace plume;

constexpr size_t kGuard = 32;
struct Arr {
    uint8_t* raw;
    uint8_t* p;
    size_t len, total;
    Arr(size_t bytes, size_t mis, const uint8_t* src = nullptr) : len(bytes), total(kGuard + 16 + bytes + kGuard) {          // exact: ASan sees a store one byte past the guards
        void* q = nullptr;
        if (posix_memalign(&q, 16, total) != 0) std::abort();
        raw = (uint8_t*)q;
        std::memset(raw, 0xAA, total);
        p = raw + kGuard + (mis & 15u);
        if (src) std::memcpy(p, src, bytes);
    }
    ~Arr() { std::free(raw); }
    Arr(const Arr&) = delete;
    Arr& operator=(const Arr&) = delete;
    bool untouched_outside() const {
        for (uint8_t* b = raw; b < p; b++) if (*b != 0xAA) return false;
        for (uint8_t* b = p + len; b < raw + total; b++) if (*b != 0xAA) return false;
        return true;
    }
    bool all_fill() const { for (size_t b = 0; b < total; b++) if (raw[b] != 0xAA) return false; return true; }
    bool holds(const std::vector<uint8_t>& v) const { return std::memcmp(p, v.data(), len) == 0 && untouched_outside(); }
};
template <class T>
static T* aligned(size_t count) {
    void* q = nullptr;
    if (posix_memalign(&q, 128, (count ? count : 1) * sizeof(T)) != 0) std::abort();
    std::memset(q, 0, (count ? count : 1) * sizeof(T));
    return (T*)q;
}

static int inverses(bool field, FILE* f, const char* out) {
    uint32_t count = 0;
    if (std::fread(&count, 4, 1, f) != 1) return 2;
    std::vector<uint8_t> in(32 * (size_t)count + 1), res(32 * (size_t)count + 1);
    if (count && std::fread(in.data(), 32, count, f) != count) return 2;
    for (uint32_t i = 0; i < count; i++) {
        uint32_t w[8];
        if (field) {
            fe a, r;
            fe_from_be(a, &in[32 * (size_t)i]);
            fe_inv(r, a);
            fe_normalize(r);
            fe_to_words(w, r);
        } else {
            sc a, r;
            sc_from_be(a, &in[32 * (size_t)i]);
            sc_inv(r, a);
            if (!sc_lt_n(r)) return 5;                          // canonical
            for (int k = 0; k < 8; k++) w[k] = r.v[k];
        }
        words_to_be(&res[32 * (size_t)i], w);
    }
    FILE* o = std::fopen(out, "wb");
    if (!o) return 2;
    std::fwrite(res.data(), 32, count, o);
    std::fclose(o);
    std::printf("ecdsa_lanes ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    const std::string mode = argv[1];
    if (mode == "scinv" || mode == "feinv") { const int rc = inverses(mode == "feinv", f, argv[3]); std::fclose(f); return rc; }
    uint32_t h[6];
    if (std::fread(h, 4, 6, f) != 6) return 2;
    const uint32_t n = h[0], mis = h[4] & 15u, present = h[5];
    EcdsaArgs a;
    std::memset(&a, 0, sizeof a);
    a.flags = (int)h[1]; a.pk_format = (int)h[2]; a.addr_format = (int)h[3]; a.n = n;
    const size_t P = eth_pk_width(a.pk_format), W = eth_address_width(a.addr_format);
    std::vector<uint8_t> h0(32 * (size_t)n + 1), r0(32 * (size_t)n + 1), s0(32 * (size_t)n + 1), v0(n + 1), e0(20 * (size_t)n + 1);
    if (n && (std::fread(h0.data(), 32, n, f) != n || std::fread(r0.data(), 32, n, f) != n || std::fread(s0.data(), 32, n, f) != n || std::fread(v0.data(), 1, n, f) != n)) return 2;
    if (n && (present & 8u) && std::fread(e0.data(), 20, n, f) != n) return 2;
    std::fclose(f);
    Arr hs(32 * (size_t)n, mis, h0.data()), rs(32 * (size_t)n, mis + 1, r0.data()), ss(32 * (size_t)n, mis + 2, s0.data()), vs(n, mis + 3, v0.data()),
        ex(20 * (size_t)n, mis + 1, e0.data()), pk(P * n, mis), ad(W * n, mis), st(n, mis + 2);
    a.hash = hs.p; a.r = rs.p; a.s = ss.p; a.v = vs.p; a.expect = (present & 8u) ? ex.p : nullptr;
    a.pk = (present & 1u) ? pk.p : nullptr; a.address = (present & 2u) ? ad.p : nullptr; a.status = (present & 4u) ? st.p : nullptr;
    // workspace
    a.bases = aligned<uint32_t>((size_t)PLUME_BASE_WORDS * n); a.jobflags = aligned<uint8_t>(n); a.itemflags = aligned<uint8_t>(n);
    a.tab = aligned<uint32_t>((size_t)PLUME_TAB_WORDS * n); a.digs = aligned<int8_t>((size_t)PLUME_NPOS * n); a.u1 = aligned<uint32_t>(8 * (size_t)n);
    a.res = aligned<uint32_t>((size_t)PLUME_JAC_WORDS * n); a.resinf = aligned<uint8_t>(n); a.redo = aligned<uint32_t>(1 + (size_t)n);
    uint32_t* comb = aligned<uint32_t>(PLUME_COMB_WORDS);
    uint32_t* cb = aligned<uint32_t>((size_t)PLUME_COMB_WINDOWS * 2 * PLUME_FE_WORDS);
    for (uint32_t w = 0; w < PLUME_COMB_WINDOWS; w++) fixed_window_base(cb + (size_t)w * 2 * PLUME_FE_WORDS, PLUME_COMB_W * w);
    for (size_t lane = 0; lane < (size_t)PLUME_COMB_ENTRIES * PLUME_COMB_WINDOWS; lane++) fixed_table_lane(comb, cb, PLUME_COMB_ENTRIES, lane);
    a.gcomb = comb;
    // the stages
    for (uint32_t i = n; i-- > 0;) ecdsa_prepare(a, i);
    constexpr int L = 3;
    uint32_t* scr = aligned<uint32_t>((size_t)L * PLUME_TAB_SCR_WORDS);
    for (size_t j0 = 0; j0 < n; j0 += L) table_build(a.tab, a.bases, a.jobflags, n, j0, (int)(n - j0 < (size_t)L ? n - j0 : (size_t)L), scr, 1, 0);
    int8_t dig[PLUME_NPOS];
    for (uint32_t i = n; i-- > 0;) ecdsa_mul<false>(a, i, dig, 1);
    const uint32_t filed = a.redo[0];
    if (filed > n) return 5;
    for (uint32_t k = 0; k < filed; k++) ecdsa_mul<true>(a, a.redo[1 + k], dig, 1);
    const size_t nlanes = ((size_t)n + PLUME_NORM_K - 1) / PLUME_NORM_K;
    for (size_t lane = 0; lane < nlanes; lane++) normalize_points(a.res, a.resinf, n, lane, nlanes);
    for (uint32_t i = n; i-- > 0;) ecdsa_finalize(a, i);
    for (void* q : {(void*)a.bases, (void*)a.jobflags, (void*)a.itemflags, (void*)a.tab, (void*)a.digs, (void*)a.u1, (void*)a.res, (void*)a.resinf, (void*)a.redo, (void*)comb,
                    (void*)cb, (void*)scr})
        std::free(q);
    if (!hs.holds(h0) || !rs.holds(r0) || !ss.holds(s0) || !vs.holds(v0) || !ex.holds(e0)) return 3;
    if ((!(present & 1u) && !pk.all_fill()) || (!(present & 2u) && !ad.all_fill()) || (!(present & 4u) && !st.all_fill())) return 3;
    if (!pk.untouched_outside() || !ad.untouched_outside() || !st.untouched_outside()) return 4;
    FILE* o = std::fopen(argv[3], "wb");
    if (!o) return 2;
    std::fwrite(&filed, 4, 1, o);
    if (present & 1u) std::fwrite(pk.p - kGuard, 1, kGuard + pk.len + kGuard, o);
    if (present & 2u) std::fwrite(ad.p - kGuard, 1, kGuard + ad.len + kGuard, o);
    if (present & 4u) std::fwrite(st.p - kGuard, 1, kGuard + st.len + kGuard, o);
    std::fclose(o);
    std::printf("ecdsa_lanes ok\n");
    return 0;
}
