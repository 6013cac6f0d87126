// The lane body of plume_eth_tx_parse_batch (csrc/plume_eth_tx.h, over the stream of csrc/plume_keccak.h) as host loops, for tests/test_eth_tx_lanes.py; built by the
// Makefile beside it with g++ under AddressSanitizer + UBSan and -Werror.
// usage: eth_tx_lanes parse IN OUT   IN: u32 n, u32 misalign of txs (0..15), u32 misalign of the outputs, u32 present (bit 0 chain_id, 1 tx_type, 2 status), u64 txs_bytes,
//                                    n + 1 u64 offsets, the bytes.  txs lies `misalign` bytes into an allocation that ends with its last byte: a load past it is a heap
//                                    overflow.  OUT: hash, r, s, v, then the arrays present (chain_id, tx_type, status), each between its guards of 32 bytes 0xAA.
//        eth_tx_lanes each IN OUT    the same IN.  Every item alone, as a batch of one, at each of the eight start residues in an allocation that ends with the item's last
//                                    byte (and, at residue 0, begins with its first).  OUT: for residue 0 .. 7: hash, r, s (32 n each), v (n), chain_id (8 n), tx_type, status.
// The harness itself checks that the input bytes are unchanged.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "plume_eth_tx.h"

using namespace plume;

constexpr size_t kGuard = 32;
struct Arr {
    uint8_t* raw;
    uint8_t* p;
    size_t len, total;
    Arr(size_t bytes, size_t mis) : len(bytes), total(kGuard + 16 + bytes + kGuard) {
        void* q = nullptr;
        if (posix_memalign(&q, 16, total) != 0) std::abort();
        raw = (uint8_t*)q;
        std::memset(raw, 0xAA, total);
        p = raw + kGuard + (mis & 15u);
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
    uint64_t bytes = 0;
    std::vector<uint64_t> off;
    std::vector<uint8_t> data;
    bool read(FILE* f) {
        uint32_t h[4];
        if (!rd(f, h, 16) || !rd(f, &bytes, 8)) return false;
        n = h[0]; mis = h[1] & 15u; mis_out = h[2]; present = h[3];
        off.resize((size_t)n + 1);
        data.resize(bytes);
        return rd(f, off.data(), 8 * off.size()) && rd(f, data.data(), bytes);
    }
};

static int run_parse(const Input& in, const char* out) {
    const size_t n = in.n;
    uint8_t* raw = (uint8_t*)std::malloc(in.mis + in.bytes + (in.mis + in.bytes ? 0 : 1));
    if (!raw) return 2;
    if (in.bytes) std::memcpy(raw + in.mis, in.data.data(), in.bytes);
    Arr hs(32 * n, in.mis_out), r(32 * n, in.mis_out + 1), s(32 * n, in.mis_out + 2), v(n, in.mis_out), chain(8 * n, 8 * (in.mis_out & 1u)), type(n, in.mis_out + 3), st(n, in.mis_out + 5);
    EthTxArgs a;
    a.n = in.n; a.txs = raw + in.mis; a.tx_off = in.off.data(); a.txs_bytes = in.bytes; a.hash = hs.p; a.r = r.p; a.s = s.p; a.v = v.p;
    a.chain_id = (in.present & 1u) ? (uint64_t*)chain.p : nullptr; a.tx_type = (in.present & 2u) ? type.p : nullptr; a.status = (in.present & 4u) ? st.p : nullptr;
    for (uint32_t i = in.n; i-- > 0;) eth_tx_parse_item(a, i);
    const bool same = in.bytes == 0 || std::memcmp(raw + in.mis, in.data.data(), in.bytes) == 0;
    std::free(raw);
    if (!same) return 3;
    FILE* o = std::fopen(out, "wb");
    if (!o) return 2;
    int rc = 0;
    for (const Arr* x : {&hs, &r, &s, &v}) { if (!x->untouched_outside()) rc = 4; x->dump(o); }
    if (in.present & 1u) { if (!chain.untouched_outside()) rc = 4; chain.dump(o); }
    if (in.present & 2u) { if (!type.untouched_outside()) rc = 4; type.dump(o); }
    if (in.present & 4u) { if (!st.untouched_outside()) rc = 4; st.dump(o); }
    std::fclose(o);
    return rc;
}

static int run_each(const Input& in, const char* out) {
    const size_t n = in.n;
    FILE* o = std::fopen(out, "wb");
    if (!o) return 2;
    for (uint32_t m = 0; m < 8; m++) {
        std::vector<uint8_t> hs(32 * n), r(32 * n), s(32 * n), v(n), type(n), st(n);
        std::vector<uint64_t> chain(n);
        for (size_t i = 0; i < n; i++) {
            if (in.off[i + 1] < in.off[i] || in.off[i + 1] > in.bytes) return 2;
            const size_t len = (size_t)(in.off[i + 1] - in.off[i]);
            uint8_t* raw = (uint8_t*)std::malloc(m + len + (m + len ? 0 : 1));
            if (!raw) return 2;
            if (len) std::memcpy(raw + m, in.data.data() + in.off[i], len);
            const uint64_t off[2] = {0, len};
            EthTxArgs a;
            a.n = 1; a.txs = raw + m; a.tx_off = off; a.txs_bytes = len; a.hash = hs.data() + 32 * i; a.r = r.data() + 32 * i; a.s = s.data() + 32 * i; a.v = v.data() + i;
            a.chain_id = chain.data() + i; a.tx_type = type.data() + i; a.status = st.data() + i;
            eth_tx_parse_item(a, 0);
            const bool same = len == 0 || std::memcmp(raw + m, in.data.data() + in.off[i], len) == 0;
            std::free(raw);
            if (!same) return 3;
        }
        std::fwrite(hs.data(), 1, hs.size(), o); std::fwrite(r.data(), 1, r.size(), o); std::fwrite(s.data(), 1, s.size(), o); std::fwrite(v.data(), 1, v.size(), o);
        std::fwrite(chain.data(), 8, chain.size(), o); std::fwrite(type.data(), 1, type.size(), o); std::fwrite(st.data(), 1, st.size(), o);
    }
    std::fclose(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: eth_tx_lanes parse|each IN OUT\n"); return 2; }
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    Input in;
    const bool ok = in.read(f);
    std::fclose(f);
    if (!ok) return 2;
    const std::string mode = argv[1];
    const int rc = mode == "parse" ? run_parse(in, argv[3]) : mode == "each" ? run_each(in, argv[3]) : 2;
    if (rc == 0) std::printf("eth_tx_lanes ok\n");
    return rc;
}
