// The lane bodies of plume_hd_master_batch, plume_hd_derive_priv_batch and plume_hd_derive_pub_batch (csrc/plume_hd.h, csrc/plume_sha512.h) as host loops, for
// tests/test_hd_lanes.py: g++ -fsanitize=address,undefined, -DPLUME_COMB_W=10 (Makefile).
// usage: hd_lanes sha512 IN OUT      IN: u32 count, then per record u32 kind (0: SHA-512 of the data, 1: HMAC by hmac_sha512_short, 2: HMAC by hmac_sha512_37), u32 key
//                                    length (<= 32), u32 data length (<= 111; 37 for kind 2), 32 key bytes (zero padded), the data in an allocation of exactly its
//                                    length.  OUT: 64 digest bytes per record.
//        hd_lanes master IN OUT      IN: u32 n, u32 seed_len, u32 misalign, the seeds (an allocation of exactly misalign + n seed_len bytes).  OUT: sk, chain, status, each
//                                    between its 32 guard bytes.
//        hd_lanes derive IN OUT      IN: u32 pub, n, flags, pk_format, addr_format, depth, uniform level, misalign, present (bit 0 chain, 1 pk, 2 address), order (0: lanes
//                                    descending, 1 ascending); the parents (1 or n records: sk, or pk in pk_format), their chain codes, the path (1 or n rows).  The stages run
//                                    lane by lane the way the kernels do.  OUT: sk (private form), chain, pk, address, status -- those present -- each between its guards.
//        hd_lanes privtweak IN OUT   IN: u32 count, per item IL, k_par (32 big-endian bytes each).  OUT per item: the child (32 bytes), u32 status bits.
//        hd_lanes pubtweak IN OUT    IN: u32 count, per item IL (32 bytes), K_par (64 bytes x || y).  OUT per item: the child as x || y (zero for the identity), u32 status bits.
// The harness itself checks that inputs and their guards are unchanged.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "plume_hd.h"

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

struct Tables {
    uint32_t *comb, *cb, *scan, *sb;
    Tables() {
        comb = aligned<uint32_t>(PLUME_COMB_WORDS);
        cb = aligned<uint32_t>((size_t)PLUME_COMB_WINDOWS * 2 * PLUME_FE_WORDS);
        for (uint32_t w = 0; w < PLUME_COMB_WINDOWS; w++) fixed_window_base(cb + (size_t)w * 2 * PLUME_FE_WORDS, PLUME_COMB_W * w);
        for (size_t lane = 0; lane < (size_t)PLUME_COMB_ENTRIES * PLUME_COMB_WINDOWS; lane++) fixed_table_lane(comb, cb, PLUME_COMB_ENTRIES, lane);
        scan = aligned<uint32_t>(PLUME_GSCAN_WORDS);
        sb = aligned<uint32_t>((size_t)PLUME_GSCAN_WINDOWS * 2 * PLUME_FE_WORDS);
        for (uint32_t w = 0; w < PLUME_GSCAN_WINDOWS; w++) fixed_window_base(sb + (size_t)w * 2 * PLUME_FE_WORDS, PLUME_GSCAN_W * w);
        for (size_t lane = 0; lane < (size_t)PLUME_GSCAN_ENTRIES * PLUME_GSCAN_WINDOWS; lane++) fixed_table_lane(scan, sb, PLUME_GSCAN_ENTRIES, lane);
    }
    ~Tables() { for (void* q : {(void*)comb, (void*)cb, (void*)scan, (void*)sb}) std::free(q); }
};

static void put64(uint8_t* o, const uint64_t d[8]) {
    for (int j = 0; j < 8; j++) for (int b = 0; b < 8; b++) o[8 * j + b] = (uint8_t)(d[j] >> (56 - 8 * b));
}
static int run_sha512(FILE* f, const char* out) {
    uint32_t count = 0;
    if (!rd(f, &count, 4)) return 2;
    std::vector<uint8_t> res(64 * (size_t)count + 1);
    for (uint32_t r = 0; r < count; r++) {
        uint32_t h[3]; uint8_t key[32];
        if (!rd(f, h, 12) || !rd(f, key, 32) || h[1] > 32 || h[2] > 111) return 2;
        uint8_t* data = (uint8_t*)std::malloc(h[2] ? h[2] : 1);                  // exact: a load past the last byte is a heap overflow
        if (!data || !rd(f, data, h[2])) return 2;
        uint64_t kw[4], d[8];
        for (int j = 0; j < 4; j++) { kw[j] = 0; for (int b = 0; b < 8; b++) kw[j] = (kw[j] << 8) | key[8 * j + b]; }
        Hmac512Key hk;
        hmac_sha512_key(hk, kw);
        const uint32_t len = h[2];
        if (h[0] == 0) { sha512_init(d); sha512_one_block(d, 0, len, [&](uint32_t pos) -> uint64_t { return data[pos]; }); }
        else if (h[0] == 1) hmac_sha512_short(d, hk, len, [&](uint32_t pos) -> uint64_t { return data[pos]; });
        else {
            if (len != 37) return 2;
            uint32_t body[8];
            for (int j = 0; j < 8; j++) body[j] = ((uint32_t)data[1 + 4 * j] << 24) | ((uint32_t)data[2 + 4 * j] << 16) | ((uint32_t)data[3 + 4 * j] << 8) | data[4 + 4 * j];
            const uint32_t idx = ((uint32_t)data[33] << 24) | ((uint32_t)data[34] << 16) | ((uint32_t)data[35] << 8) | data[36];
            uint32_t k32[8];
            for (int j = 0; j < 8; j++) k32[j] = ((uint32_t)key[4 * j] << 24) | ((uint32_t)key[4 * j + 1] << 16) | ((uint32_t)key[4 * j + 2] << 8) | key[4 * j + 3];
            hmac_sha512_key32(hk, k32);
            hmac_sha512_37(d, hk, data[0], body, idx);
        }
        put64(&res[64 * (size_t)r], d);
        std::free(data);
    }
    FILE* o = std::fopen(out, "wb");
    if (!o) return 2;
    std::fwrite(res.data(), 1, 64 * (size_t)count, o);
    std::fclose(o);
    return 0;
}

static int run_master(FILE* f, const char* out) {
    uint32_t h[3];
    if (!rd(f, h, 12)) return 2;
    const uint32_t n = h[0], sl = h[1], mis = h[2] & 15u;
    const size_t bytes = (size_t)n * sl;
    uint8_t* raw = (uint8_t*)std::malloc(mis + bytes + (mis + bytes ? 0 : 1));
    if (!raw || !rd(f, raw + mis, bytes)) return 2;
    std::vector<uint8_t> copy(raw + mis, raw + mis + bytes);
    Arr sk(32 * (size_t)n, mis + 1), ch(32 * (size_t)n, mis + 2), st(n, mis + 3);
    HdArgs a;
    std::memset(&a, 0, sizeof a);
    a.n = n; a.seed_len = sl; a.parent = raw + mis; a.child_sk = sk.p; a.child_chain = ch.p; a.status = st.p;
    for (uint32_t i = n; i-- > 0;) hd_master_item(a, i);
    const bool same = bytes == 0 || std::memcmp(raw + mis, copy.data(), bytes) == 0;
    std::free(raw);
    if (!same) return 3;
    if (!sk.untouched_outside() || !ch.untouched_outside() || !st.untouched_outside()) return 4;
    FILE* o = std::fopen(out, "wb");
    if (!o) return 2;
    sk.dump(o); ch.dump(o); st.dump(o);
    std::fclose(o);
    return 0;
}

static int run_derive(FILE* f, const char* out) {
    uint32_t h[10];
    if (!rd(f, h, 40)) return 2;
    const bool pub = h[0] != 0;
    const uint32_t n = h[1], depth = h[5], mis = h[7] & 15u, present = h[8];
    const int flags = (int)h[2], pkf = (int)h[3], adf = (int)h[4];
    const size_t pw = pub ? eth_pk_width(pkf) : 32, np = (flags & PLUME_HDK_SHARED_PARENT) ? 1 : n, nr = (flags & PLUME_HDK_SHARED_PATH) ? 1 : n;
    std::vector<uint8_t> p0(pw * np + 1), c0(32 * np + 1), t0(4 * (size_t)depth * nr + 1);
    if (!rd(f, p0.data(), pw * np) || !rd(f, c0.data(), 32 * np) || !rd(f, t0.data(), 4 * (size_t)depth * nr)) return 2;
    Arr par(pw * np, mis, p0.data()), pch(32 * np, mis + 1, c0.data()), path(4 * (size_t)depth * nr, mis + 2, t0.data());
    Arr sk(32 * (size_t)n, mis + 3), ch(32 * (size_t)n, mis + 1), pk((size_t)eth_pk_width(pkf) * n, mis + 2), ad((size_t)eth_address_width(adf) * n, mis + 3), st(n, mis + 1);
    Tables tb;
    HdArgs a;
    std::memset(&a, 0, sizeof a);
    a.flags = flags; a.pk_format = pkf; a.addr_format = adf; a.uniform = (int)h[6]; a.n = n; a.depth = depth;
    a.parent = par.p; a.parent_chain = pch.p; a.path = path.p;
    a.child_sk = pub ? nullptr : sk.p; a.child_chain = (present & 1u) ? ch.p : nullptr; a.child_pk = (present & 2u) ? pk.p : nullptr; a.address = (present & 4u) ? ad.p : nullptr;
    a.status = st.p;
    a.k = aligned<uint8_t>(32 * (size_t)n); a.chain = aligned<uint8_t>(32 * (size_t)n); a.st = aligned<uint8_t>(n);
    a.res = aligned<uint32_t>((size_t)PLUME_JAC_WORDS * n); a.resinf = aligned<uint8_t>(n);
    a.gcomb = tb.comb; a.gscan = tb.scan;
    const bool up = h[9] != 0;
    auto each = [&](auto body) { if (up) { for (uint32_t i = 0; i < n; i++) body(i); } else { for (uint32_t i = n; i-- > 0;) body(i); } };
    auto affine = [&]() { const size_t nl = ((size_t)n + PLUME_NORM_K - 1) / PLUME_NORM_K; for (size_t lane = 0; lane < nl; lane++) normalize_points(a.res, a.resinf, n, lane, nl); };
    if (pub) {
        each([&](uint32_t i) { hd_pub_load(a, i); });
        for (uint32_t j = 0; j < depth; j++) { a.level = j; each([&](uint32_t i) { hd_pub_step(a, i); }); affine(); }
    } else {
        each([&](uint32_t i) { hd_priv_load(a, i); });
        for (uint32_t j = 0; j <= depth; j++) {
            each([&](uint32_t i) { if (a.uniform == 2) hd_gmul<2>(a, i); else if (a.uniform == 1) hd_gmul<1>(a, i); else hd_gmul<0>(a, i); });
            affine();
            if (j == depth) break;
            a.level = j;
            each([&](uint32_t i) { hd_priv_step(a, i); });
        }
    }
    each([&](uint32_t i) { hd_finish(a, i); });
    for (void* q : {(void*)a.k, (void*)a.chain, (void*)a.st, (void*)a.res, (void*)a.resinf}) std::free(q);
    if (!par.holds(p0) || !pch.holds(c0) || !path.holds(t0)) return 3;
    if (!sk.untouched_outside() || !ch.untouched_outside() || !pk.untouched_outside() || !ad.untouched_outside() || !st.untouched_outside()) return 4;
    // an output that was not asked for is not written at all
    auto blank = [](const Arr& x) { for (size_t b = 0; b < x.len; b++) if (x.p[b] != 0xAA) return false; return true; };
    if ((pub && !blank(sk)) || (!(present & 1u) && !blank(ch)) || (!(present & 2u) && !blank(pk)) || (!(present & 4u) && !blank(ad))) return 5;
    FILE* o = std::fopen(out, "wb");
    if (!o) return 2;
    if (!pub) sk.dump(o);
    if (present & 1u) ch.dump(o);
    if (present & 2u) pk.dump(o);
    if (present & 4u) ad.dump(o);
    st.dump(o);
    std::fclose(o);
    return 0;
}

static int run_privtweak(FILE* f, const char* out) {
    uint32_t count = 0;
    if (!rd(f, &count, 4)) return 2;
    std::vector<uint8_t> in(64 * (size_t)count + 1), res(36 * (size_t)count + 1);
    if (!rd(f, in.data(), 64 * (size_t)count)) return 2;
    for (uint32_t i = 0; i < count; i++) {
        sc il, kp, kc;
        sc_from_be(il, &in[64 * (size_t)i]); sc_from_be(kp, &in[64 * (size_t)i + 32]);
        const uint32_t st = hd_priv_tweak(kc, il, kp);
        for (int j = 0; j < 8; j++) for (int b = 0; b < 4; b++) res[36 * (size_t)i + 4 * j + b] = (uint8_t)(kc.v[7 - j] >> (24 - 8 * b));
        std::memcpy(&res[36 * (size_t)i + 32], &st, 4);
    }
    FILE* o = std::fopen(out, "wb");
    if (!o) return 2;
    std::fwrite(res.data(), 1, 36 * (size_t)count, o);
    std::fclose(o);
    return 0;
}
static int run_pubtweak(FILE* f, const char* out) {
    uint32_t count = 0;
    if (!rd(f, &count, 4)) return 2;
    std::vector<uint8_t> in(96 * (size_t)count + 1), res(68 * (size_t)count + 1);
    if (!rd(f, in.data(), 96 * (size_t)count)) return 2;
    Tables tb;
    for (uint32_t i = 0; i < count; i++) {
        sc il;
        fe x, y;
        sc_from_be(il, &in[96 * (size_t)i]);
        fe_from_be(x, &in[96 * (size_t)i + 32]); fe_from_be(y, &in[96 * (size_t)i + 64]);
        jac c;
        const uint32_t st = hd_pub_tweak(c, il, x, y, tb.comb);
        std::memset(&res[68 * (size_t)i], 0, 64);
        if (!c.inf) {
            fe zi, zi2, ax, ay;
            fe_inv(zi, c.z); fe_sqr(zi2, zi);
            fe_mul(ax, c.x, zi2); fe_mul(zi2, zi2, zi); fe_mul(ay, c.y, zi2);
            fe_normalize(ax); fe_normalize(ay);
            fe_to_be(&res[68 * (size_t)i], ax); fe_to_be(&res[68 * (size_t)i + 32], ay);
        }
        std::memcpy(&res[68 * (size_t)i + 64], &st, 4);
    }
    FILE* o = std::fopen(out, "wb");
    if (!o) return 2;
    std::fwrite(res.data(), 1, 68 * (size_t)count, o);
    std::fclose(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: hd_lanes sha512|master|derive|privtweak|pubtweak IN OUT\n"); return 2; }
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    const std::string mode = argv[1];
    int rc = 2;
    if (mode == "sha512") rc = run_sha512(f, argv[3]);
    else if (mode == "master") rc = run_master(f, argv[3]);
    else if (mode == "derive") rc = run_derive(f, argv[3]);
    else if (mode == "privtweak") rc = run_privtweak(f, argv[3]);
    else if (mode == "pubtweak") rc = run_pubtweak(f, argv[3]);
    std::fclose(f);
    if (rc == 0) std::printf("hd_lanes ok\n");
    return rc;
}
