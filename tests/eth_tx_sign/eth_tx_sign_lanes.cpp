// The lane bodies of plume_eth_tx_sign_batch (csrc/plume_eth_tx_sign.h) as host loops, for tests/test_eth_tx_sign_lanes.py; built by the Makefile beside it with g++ under
// AddressSanitizer + UBSan and -Werror.  The signature between the two bodies comes from the test (the restatement's numbers, or chosen values no signer produces).
// usage: eth_tx_sign_lanes batch IN OUT
//   IN:  u32 n, u32 misalign of txs (0..15), u32 misalign of out and the records, u32 present (bit 0 hash, 1 r, 2 s, 3 v, 4 chain_id, 5 tx_type), u64 txs_bytes, u64 out_bytes,
//        n + 1 u64 offsets, the bytes, then the staged r (32 n), s (32 n), v (n), status (n).
//        txs lies `misalign` bytes into an allocation that ends with its last byte, out likewise into one that ends with byte out_bytes: an access past either is a heap
//        overflow.  The bytes in front of out are 0xAA and checked.
//   OUT: what the frame staged -- chain (8 n), frame word (8 n), hash (32 n) --, out (out_bytes), then out_len (4 n), status (n) and the records present, each of these
//        between its guards of 32 bytes 0xAA.
//   The lanes run twice, last item first and first item first, into buffers of their own, and both runs must agree: a lane that leaves its slot is either still visible in
//   its neighbour's or changes what that neighbour wrote.
// usage: eth_tx_sign_lanes each IN OUT    the same IN.  Every item alone, as a batch of one, its slot at each of the eight start residues between guard bytes, the input
//   in an allocation that begins and ends with the item.  OUT: for residue 0 .. 7, for every item: its slot (len + 68 bytes), out_len (4), status (1).
// The harness itself checks that the input bytes are unchanged.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "plume_eth_tx_sign.h"

using namespace plume;

constexpr size_t kGuard = 32;
struct Arr {
    uint8_t* raw;
    uint8_t* p;
    size_t len, total;
    Arr(size_t bytes, size_t mis, size_t align = 1) : len(bytes), total(kGuard + 16 + bytes + kGuard) {
        void* q = nullptr;
        if (posix_memalign(&q, 16, total) != 0) std::abort();
        raw = (uint8_t*)q;
        std::memset(raw, 0xAA, total);
        p = raw + kGuard + ((mis & 15u) / align) * align;
    }
    ~Arr() { std::free(raw); }
    Arr(const Arr&) = delete;
    Arr& operator=(const Arr&) = delete;
    bool untouched_outside() const {
        for (uint8_t* b = raw; b < p; b++) if (*b != 0xAA) return false;
        for (uint8_t* b = p + len; b < raw + total; b++) if (*b != 0xAA) return false;
        return true;
    }
    void dump(FILE* o) const { std::fwrite(p - kGuard, 1, kGuard + len + kGuard, o); }
};
static bool rd(FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }

struct Input {
    uint32_t n = 0, mis = 0, mis_out = 0, present = 0;
    uint64_t bytes = 0, out_bytes = 0;
    std::vector<uint64_t> off;
    std::vector<uint8_t> data, r, s, v, st;
    bool read(FILE* f) {
        uint32_t h[4];
        if (!rd(f, h, 16) || !rd(f, &bytes, 8) || !rd(f, &out_bytes, 8)) return false;
        n = h[0]; mis = h[1] & 15u; mis_out = h[2] & 15u; present = h[3];
        off.resize((size_t)n + 1);
        data.resize(bytes); r.resize(32 * (size_t)n); s.resize(32 * (size_t)n); v.resize(n); st.resize(n);
        return rd(f, off.data(), 8 * off.size()) && rd(f, data.data(), bytes) && rd(f, r.data(), r.size()) && rd(f, s.data(), s.size()) && rd(f, v.data(), n) && rd(f, st.data(), n);
    }
};

// the staging of n items, laid out as the library lays it out
struct Staging {
    std::vector<uint64_t> buf;
    uint8_t* b;
    size_t n;
    explicit Staging(size_t n_) : buf((PLUME_ETHTXK_SIGN_STAGE * n_ + 7) / 8 + 1), b((uint8_t*)buf.data()), n(n_) {}
    void point(EthTxSignArgs& a) {
        a.st_chain = (uint64_t*)b; a.st_frame = (uint64_t*)(b + 8 * n); a.st_hash = b + 16 * n; a.st_r = b + 48 * n; a.st_s = b + 80 * n; a.st_v = b + 112 * n; a.st_status = b + 113 * n;
    }
    void sign(const uint8_t* r, const uint8_t* s, const uint8_t* v, const uint8_t* st, size_t cnt) {
        if (!cnt) return;
        std::memcpy(b + 48 * n, r, 32 * cnt); std::memcpy(b + 80 * n, s, 32 * cnt); std::memcpy(b + 112 * n, v, cnt); std::memcpy(b + 113 * n, st, cnt);
    }
};

struct OutBuf {                                                             // out: mis bytes of 0xAA, then out_bytes that end with the allocation
    uint8_t* raw;
    size_t mis, len;
    OutBuf(size_t mis_, size_t len_) : raw((uint8_t*)std::malloc(mis_ + len_ + (mis_ + len_ ? 0 : 1))), mis(mis_), len(len_) {
        if (!raw) std::abort();
        std::memset(raw, 0xAA, mis); std::memset(raw + mis, 0x55, len);
    }
    ~OutBuf() { std::free(raw); }
    uint8_t* p() const { return raw + mis; }
    bool front_untouched() const { for (size_t k = 0; k < mis; k++) if (raw[k] != 0xAA) return false; return true; }
};

static int run_batch(const Input& in, const char* out) {
    const size_t n = in.n;
    uint8_t* raw = (uint8_t*)std::malloc(in.mis + in.bytes + (in.mis + in.bytes ? 0 : 1));
    if (!raw) return 2;
    if (in.bytes) std::memcpy(raw + in.mis, in.data.data(), in.bytes);
    Staging stg(n);
    OutBuf o1(in.mis_out, in.out_bytes), o2(in.mis_out, in.out_bytes);
    Arr len1(4 * n, 4 * (in.mis_out & 3u), 4), len2(4 * n, 0, 4), st1(n, in.mis_out + 5), st2(n, 1);
    Arr hs(32 * n, in.mis_out), r(32 * n, in.mis_out + 1), s(32 * n, in.mis_out + 2), v(n, in.mis_out + 7), chain(8 * n, 8 * (in.mis_out & 1u), 8), type(n, in.mis_out + 3);
    EthTxSignArgs a;
    std::memset(&a, 0, sizeof a);
    a.n = in.n; a.txs = raw + in.mis; a.tx_off = in.off.data(); a.txs_bytes = in.bytes;
    stg.point(a);
    for (uint32_t i = in.n; i-- > 0;) eth_tx_sign_frame_item(a, i);
    FILE* o = std::fopen(out, "wb");
    if (!o) return 2;
    std::fwrite(stg.b, 1, 48 * n, o);
    stg.sign(in.r.data(), in.s.data(), in.v.data(), in.st.data(), n);
    a.out_bytes = in.out_bytes;
    a.hash = (in.present & 1u) ? hs.p : nullptr; a.r = (in.present & 2u) ? r.p : nullptr; a.s = (in.present & 4u) ? s.p : nullptr; a.v = (in.present & 8u) ? v.p : nullptr;
    a.chain_id = (in.present & 16u) ? (uint64_t*)chain.p : nullptr; a.tx_type = (in.present & 32u) ? type.p : nullptr;
    a.out = o1.p(); a.out_len = (uint32_t*)len1.p; a.status = st1.p;
    for (uint32_t i = in.n; i-- > 0;) eth_tx_sign_assemble_item(a, i);
    a.out = o2.p(); a.out_len = (uint32_t*)len2.p; a.status = st2.p;
    for (uint32_t i = 0; i < in.n; i++) eth_tx_sign_assemble_item(a, i);
    const bool same = in.bytes == 0 || std::memcmp(raw + in.mis, in.data.data(), in.bytes) == 0;
    std::free(raw);
    int rc = same ? 0 : 3;
    if (!o1.front_untouched() || !o2.front_untouched()) rc = 4;
    if (in.out_bytes && std::memcmp(o1.p(), o2.p(), in.out_bytes) != 0) rc = 5;
    if (std::memcmp(len1.p, len2.p, 4 * n) != 0 || std::memcmp(st1.p, st2.p, n) != 0) rc = 5;
    std::fwrite(o1.p(), 1, in.out_bytes, o);
    for (const Arr* x : {&len1, &st1}) { if (!x->untouched_outside()) rc = 4; x->dump(o); }
    const Arr* rec[6] = {&hs, &r, &s, &v, &chain, &type};
    for (int k = 0; k < 6; k++) if ((in.present >> k) & 1u) { if (!rec[k]->untouched_outside()) rc = 4; rec[k]->dump(o); }
    if (!len2.untouched_outside() || !st2.untouched_outside()) rc = 4;
    std::fclose(o);
    return rc;
}

static int run_each(const Input& in, const char* out) {
    const size_t n = in.n;
    FILE* o = std::fopen(out, "wb");
    if (!o) return 2;
    for (uint32_t m = 0; m < 8; m++) {
        for (size_t i = 0; i < n; i++) {
            if (in.off[i + 1] < in.off[i] || in.off[i + 1] > in.bytes) return 2;
            const size_t len = (size_t)(in.off[i + 1] - in.off[i]);
            uint8_t* raw = (uint8_t*)std::malloc(len ? len : 1);
            if (!raw) return 2;
            if (len) std::memcpy(raw, in.data.data() + in.off[i], len);
            const uint64_t off[2] = {0, len};
            Staging stg(1);
            Arr slot(len + PLUME_ETHTXK_SIGN_GROWTH, m);
            uint32_t out_len = 0xAAAAAAAAu;
            uint8_t st = 0xAA;
            EthTxSignArgs a;
            std::memset(&a, 0, sizeof a);
            a.n = 1; a.txs = raw; a.tx_off = off; a.txs_bytes = len;
            stg.point(a);
            eth_tx_sign_frame_item(a, 0);
            stg.sign(in.r.data() + 32 * i, in.s.data() + 32 * i, in.v.data() + i, in.st.data() + i, 1);
            a.out = slot.p; a.out_bytes = slot.len; a.out_len = &out_len; a.status = &st;
            eth_tx_sign_assemble_item(a, 0);
            const bool same = len == 0 || std::memcmp(raw, in.data.data() + in.off[i], len) == 0;
            std::free(raw);
            if (!same) return 3;
            if (!slot.untouched_outside()) return 4;
            std::fwrite(slot.p, 1, slot.len, o); std::fwrite(&out_len, 4, 1, o); std::fwrite(&st, 1, 1, o);
        }
    }
    std::fclose(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: eth_tx_sign_lanes batch|each IN OUT\n"); return 2; }
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    Input in;
    const bool ok = in.read(f);
    std::fclose(f);
    if (!ok) return 2;
    const std::string mode = argv[1];
    const int rc = mode == "batch" ? run_batch(in, argv[3]) : mode == "each" ? run_each(in, argv[3]) : 2;
    if (rc == 0) std::printf("eth_tx_sign_lanes ok\n");
    return rc;
}
