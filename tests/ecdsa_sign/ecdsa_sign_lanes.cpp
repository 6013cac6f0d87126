// The lane bodies of plume_ecdsa_sign_batch (csrc/plume_ecdsa_sign.h) and of plume_eth_message_hash_batch (csrc/plume_keccak.h) as host loops, for
// tests/test_ecdsa_sign_lanes.py: g++ -fsanitize=address,undefined, -DPLUME_COMB_W=10 (Makefile).
// usage: ecdsa_sign_lanes hash IN OUT     IN: u32 n, u32 mode, u32 misalign of msgs (0..15), u32 misalign of the digests, u64 msgs_bytes, n + 1 u64 offsets, the message
//                                         bytes.  msgs is an allocation of EXACTLY misalign + msgs_bytes bytes, so that ASan sees any load outside it.
//                                         OUT: 32 guard bytes, n digests, 32 guard bytes.
//        ecdsa_sign_lanes sign IN OUT     IN: u32 n, u32 flags, u32 uniform level, u32 misalign, u32 aux given, u32 self-check staging (1: sk G is computed and staged too),
//                                         then n hashes, n sk, (n aux) of 32 bytes.  The stages run lane by lane the way the kernels do: ecdsa_sign_nonce (descending),
//                                         ecdsa_sign_gmul at the level, normalize_points eight per lane, ecdsa_sign_finalize.  hash lies `misalign` bytes behind a
//                                         16-byte boundary, sk one byte further, aux two, r three, s one, v two, status three.
//                                         OUT: n u32 candidate counts of the nonce stage, the nonces (32 n bytes), then r, s, v, status (and, staged, 64 n bytes of sk G),
//                                         each between its 32 guard bytes.
//        ecdsa_sign_lanes rfromx IN OUT   IN: u32 count, count field elements of 32 big-endian bytes (below p).  OUT per value: r = x mod n (32 bytes), u32 status bits
//                                         of ecdsa_sign_r_from_x.
//        ecdsa_sign_lanes release IN OUT  IN: u32 n, u32 misalign, then the staging: r, s (32 n each), v, status (n each), sk G (64 n), the recovered keys (64 n), the
//                                         recover stages' status (n).  OUT: r, s, v, status as ecdsa_sign_release writes them, each between its guards.
// The harness itself checks that inputs and their guards are unchanged.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "plume_ecdsa_sign.h"

using namespace plume;

constexpr size_t kGuard = 32;
struct Arr {
    uint8_t* raw;
    uint8_t* p;
    size_t len, total;
    Arr(size_t bytes, size_t mis, const uint8_t* src = nullptr) : len(bytes), total(kGuard + 16 + bytes + kGuard) {
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
    bool holds(const std::vector<uint8_t>& v) const { return std::memcmp(p, v.data(), len) == 0 && untouched_outside(); }
    void dump(FILE* o) const { std::fwrite(p - kGuard, 1, kGuard + len + kGuard, o); }
};
template <class T>
static T* aligned(size_t count) {
    void* q = nullptr;
    if (posix_memalign(&q, 128, (count ? count : 1) * sizeof(T)) != 0) std::abort();
    std::memset(q, 0, (count ? count : 1) * sizeof(T));
    return (T*)q;
}
static bool rd(FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }

static int run_hash(FILE* f, const char* out) {
    uint32_t h[4]; uint64_t bytes = 0;
    if (!rd(f, h, 16) || !rd(f, &bytes, 8)) return 2;
    const uint32_t n = h[0];
    uint64_t* off = aligned<uint64_t>((size_t)n + 1);
    if (!rd(f, off, 8 * ((size_t)n + 1))) return 2;
    const size_t mis = h[2] & 15u;
    uint8_t* raw = (uint8_t*)std::malloc(mis + bytes + (mis + bytes ? 0 : 1));          // exact: a load past the last message byte is a heap overflow
    if (!raw || !rd(f, raw + mis, bytes)) return 2;
    std::vector<uint8_t> copy(raw + mis, raw + mis + bytes);
    Arr dg(32 * (size_t)n, h[3]);
    EthHashArgs a;
    a.mode = (int)h[1]; a.n = n; a.msgs = raw + mis; a.msg_off = off; a.msgs_bytes = bytes; a.hash = dg.p;
    for (uint32_t i = n; i-- > 0;) eth_message_hash_item(a, i);
    const bool same = bytes == 0 || std::memcmp(raw + mis, copy.data(), bytes) == 0;
    std::free(raw); std::free(off);
    if (!same) return 3;
    if (!dg.untouched_outside()) return 4;
    FILE* o = std::fopen(out, "wb");
    if (!o) return 2;
    dg.dump(o);
    std::fclose(o);
    return 0;
}

static int run_sign(FILE* f, const char* out) {
    uint32_t h[6];
    if (!rd(f, h, 24)) return 2;
    const uint32_t n = h[0], mis = h[3] & 15u;
    const bool has_aux = h[4] != 0, staged = h[5] != 0;
    const size_t T = staged ? 2 : 1;
    std::vector<uint8_t> h0(32 * (size_t)n + 1), k0(32 * (size_t)n + 1), a0(32 * (size_t)n + 1);
    if (!rd(f, h0.data(), 32 * (size_t)n) || !rd(f, k0.data(), 32 * (size_t)n) || (has_aux && !rd(f, a0.data(), 32 * (size_t)n))) return 2;
    Arr hs(32 * (size_t)n, mis, h0.data()), sk(32 * (size_t)n, mis + 1, k0.data()), ax(32 * (size_t)n, mis + 2, a0.data()), r(32 * (size_t)n, mis + 3), s(32 * (size_t)n, mis + 1),
        v(n, mis + 2), st(n, mis + 3), pk(64 * (size_t)n, mis);
    EcdsaSignArgs a;
    std::memset(&a, 0, sizeof a);
    a.flags = (int)h[1]; a.uniform = (int)h[2]; a.n = n; a.ntask = (uint32_t)T;
    a.hash = hs.p; a.sk = sk.p; a.aux = has_aux ? ax.p : nullptr; a.r = r.p; a.s = s.p; a.v = v.p; a.status = st.p; a.pkstage = staged ? pk.p : nullptr;
    a.k = aligned<uint8_t>(32 * (size_t)n); a.itemflags = aligned<uint8_t>(n);
    a.res = aligned<uint32_t>((size_t)PLUME_JAC_WORDS * T * n); a.resinf = aligned<uint8_t>(T * n);
    uint32_t* comb = aligned<uint32_t>(PLUME_COMB_WORDS);
    uint32_t* cb = aligned<uint32_t>((size_t)PLUME_COMB_WINDOWS * 2 * PLUME_FE_WORDS);
    for (uint32_t w = 0; w < PLUME_COMB_WINDOWS; w++) fixed_window_base(cb + (size_t)w * 2 * PLUME_FE_WORDS, PLUME_COMB_W * w);
    for (size_t lane = 0; lane < (size_t)PLUME_COMB_ENTRIES * PLUME_COMB_WINDOWS; lane++) fixed_table_lane(comb, cb, PLUME_COMB_ENTRIES, lane);
    uint32_t* scan = aligned<uint32_t>(PLUME_GSCAN_WORDS);
    uint32_t* sb = aligned<uint32_t>((size_t)PLUME_GSCAN_WINDOWS * 2 * PLUME_FE_WORDS);
    for (uint32_t w = 0; w < PLUME_GSCAN_WINDOWS; w++) fixed_window_base(sb + (size_t)w * 2 * PLUME_FE_WORDS, PLUME_GSCAN_W * w);
    for (size_t lane = 0; lane < (size_t)PLUME_GSCAN_ENTRIES * PLUME_GSCAN_WINDOWS; lane++) fixed_table_lane(scan, sb, PLUME_GSCAN_ENTRIES, lane);
    a.gcomb = comb; a.gscan = scan;
    std::vector<uint32_t> used(n + 1);
    for (uint32_t i = n; i-- > 0;) used[i] = ecdsa_sign_nonce(a, i);
    std::vector<uint8_t> nonces(32 * (size_t)n + 1);
    std::memcpy(nonces.data(), a.k, 32 * (size_t)n);
    for (uint32_t which = 0; which < T; which++)
        for (uint32_t i = n; i-- > 0;) {
            if (a.uniform == 2) ecdsa_sign_gmul<2>(a, i, which);
            else if (a.uniform == 1) ecdsa_sign_gmul<1>(a, i, which);
            else ecdsa_sign_gmul<0>(a, i, which);
        }
    const size_t npts = T * n, nlanes = (npts + PLUME_NORM_K - 1) / PLUME_NORM_K;
    for (size_t lane = 0; lane < nlanes; lane++) normalize_points(a.res, a.resinf, npts, lane, nlanes);
    for (uint32_t i = n; i-- > 0;) ecdsa_sign_finalize(a, i);
    for (void* q : {(void*)a.k, (void*)a.itemflags, (void*)a.res, (void*)a.resinf, (void*)comb, (void*)cb, (void*)scan, (void*)sb}) std::free(q);
    if (!hs.holds(h0) || !sk.holds(k0) || !ax.holds(a0)) return 3;
    if (!r.untouched_outside() || !s.untouched_outside() || !v.untouched_outside() || !st.untouched_outside() || !pk.untouched_outside()) return 4;
    FILE* o = std::fopen(out, "wb");
    if (!o) return 2;
    std::fwrite(used.data(), 4, n, o);
    std::fwrite(nonces.data(), 1, 32 * (size_t)n, o);
    r.dump(o); s.dump(o); v.dump(o); st.dump(o);
    if (staged) pk.dump(o);
    std::fclose(o);
    return 0;
}

static int run_rfromx(FILE* f, const char* out) {
    uint32_t count = 0;
    if (!rd(f, &count, 4)) return 2;
    std::vector<uint8_t> in(32 * (size_t)count + 1), res(36 * (size_t)count + 1);
    if (!rd(f, in.data(), 32 * (size_t)count)) return 2;
    for (uint32_t i = 0; i < count; i++) {
        fe x;
        fe_from_be(x, &in[32 * (size_t)i]);
        fe_normalize(x);
        uint32_t xw[8];
        fe_to_words(xw, x);
        sc r;
        const uint32_t st = ecdsa_sign_r_from_x(r, xw);
        words_to_be(&res[36 * (size_t)i], r.v);
        std::memcpy(&res[36 * (size_t)i + 32], &st, 4);
    }
    FILE* o = std::fopen(out, "wb");
    if (!o) return 2;
    std::fwrite(res.data(), 36, count, o);
    std::fclose(o);
    return 0;
}

static int run_release(FILE* f, const char* out) {
    uint32_t h[2];
    if (!rd(f, h, 8)) return 2;
    const size_t n = h[0];
    const uint32_t mis = h[1] & 15u;
    uint8_t* stg = aligned<uint8_t>(195 * n);                                    // the staging is 16-byte aligned in the library
    if (!rd(f, stg, 195 * n)) return 2;
    std::vector<uint8_t> copy(stg, stg + 195 * n);
    Arr r(32 * n, mis), s(32 * n, mis + 1), v(n, mis + 2), st(n, mis + 3);
    EcdsaSignReleaseArgs a;
    a.n = (uint32_t)n; a.stage_r = stg; a.stage_s = stg + 32 * n; a.stage_v = stg + 64 * n; a.stage_status = stg + 65 * n;
    uint8_t* pkbuf = aligned<uint8_t>(128 * n);
    std::memcpy(pkbuf, stg + 66 * n, 128 * n);                                   // sk G and the recovered keys are compared as words: 16-byte aligned, as the library's layout keeps them
    a.stage_pk = pkbuf; a.rec_pk = pkbuf + 64 * n; a.rec_status = stg + 194 * n;
    a.r = r.p; a.s = s.p; a.v = v.p; a.status = st.p;
    for (uint32_t i = (uint32_t)n; i-- > 0;) ecdsa_sign_release(a, i);
    const bool same = n == 0 || std::memcmp(stg, copy.data(), 195 * n) == 0;
    std::free(stg); std::free(pkbuf);
    if (!same) return 3;
    if (!r.untouched_outside() || !s.untouched_outside() || !v.untouched_outside() || !st.untouched_outside()) return 4;
    FILE* o = std::fopen(out, "wb");
    if (!o) return 2;
    r.dump(o); s.dump(o); v.dump(o); st.dump(o);
    std::fclose(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    const std::string mode = argv[1];
    const int rc = mode == "hash" ? run_hash(f, argv[3]) : mode == "sign" ? run_sign(f, argv[3]) : mode == "rfromx" ? run_rfromx(f, argv[3]) : mode == "release" ? run_release(f, argv[3]) : 2;
    std::fclose(f);
    if (rc == 0) std::printf("ecdsa_sign_lanes ok\n");
    return rc;
}
