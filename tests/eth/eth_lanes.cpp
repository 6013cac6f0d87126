// k_eth_address's lane body (csrc/plume_keccak.h) as a host loop, for tests/test_eth_lanes.py: g++ -fsanitize=address,undefined.
// usage: eth_lanes IN OUT.  IN: u32 n, u32 pk_format, u32 addr_format, u32 misalign (0..15), u32 present (bit 0: address is given, bit 1: status, bit 2: expect), then
// n keys of 64 / 33 bytes, then (bit 2) n expected addresses of 20 bytes.
// Every array -- pk, expect, address, status -- lies between 32 guard bytes pre-filled with 0xAA, `misalign` bytes behind a 16-byte boundary (expect one byte further,
// status two), so misalign 0 takes the 16-byte loads and stores and every other value the byte paths.  OUT: for each output that is given, the 32 guard bytes, the array,
// 32 guard bytes.  The harness itself checks that the inputs and their guards are unchanged and that an output that is not given was never written.  Every lane runs, in
// descending order.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "plume_keccak.h"

using namespace plume;

constexpr size_t kGuard = 32;
struct Arr {
    uint8_t* raw;
    uint8_t* p;
    size_t len, total;
    Arr(size_t bytes, size_t mis) : len(bytes), total(kGuard + 16 + bytes + kGuard) {          // exact: ASan sees a store one byte past the guards
        void* q = nullptr;
        if (posix_memalign(&q, 16, total) != 0) std::abort();
        raw = (uint8_t*)q;
        std::memset(raw, 0xAA, total);
        p = raw + kGuard + (mis & 15u);
    }
    ~Arr() { std::free(raw); }
    bool untouched_outside() const {
        for (uint8_t* b = raw; b < p; b++) if (*b != 0xAA) return false;
        for (uint8_t* b = p + len; b < raw + total; b++) if (*b != 0xAA) return false;
        return true;
    }
    bool all_fill() const { for (size_t b = 0; b < total; b++) if (raw[b] != 0xAA) return false; return true; }
};

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t h[5];
    if (std::fread(h, 4, 5, f) != 5) return 2;
    const uint32_t n = h[0], mis = h[3] & 15u, present = h[4];
    EthArgs a;
    std::memset(&a, 0, sizeof a);
    a.pk_format = (int)h[1]; a.addr_format = (int)h[2]; a.n = n;
    const size_t P = eth_pk_width(a.pk_format), W = eth_address_width(a.addr_format);
    std::vector<uint8_t> pk0(P * n + 1), ex0(20 * (size_t)n + 1);
    if (n && std::fread(pk0.data(), P, n, f) != n) return 2;
    if (n && (present & 4u) && std::fread(ex0.data(), 20, n, f) != n) return 2;
    std::fclose(f);
    Arr pk(P * n, mis), ex(20 * (size_t)n, mis + 1), ad(W * n, mis), st(n, mis + 2);
    std::memcpy(pk.p, pk0.data(), P * n);
    std::memcpy(ex.p, ex0.data(), 20 * (size_t)n);
    a.pk = pk.p; a.expect = (present & 4u) ? ex.p : nullptr; a.address = (present & 1u) ? ad.p : nullptr; a.status = (present & 2u) ? st.p : nullptr;
    for (uint32_t i = n; i-- > 0;) eth_address_item(a, i);
    if (std::memcmp(pk.p, pk0.data(), P * n) != 0 || std::memcmp(ex.p, ex0.data(), 20 * (size_t)n) != 0 || !pk.untouched_outside() || !ex.untouched_outside()) return 3;
    if (!(present & 1u) && !ad.all_fill()) return 3;
    if (!(present & 2u) && !st.all_fill()) return 3;
    if (!ad.untouched_outside() || !st.untouched_outside()) return 4;
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    if (present & 1u) std::fwrite(ad.p - kGuard, 1, kGuard + ad.len + kGuard, o);
    if (present & 2u) std::fwrite(st.p - kGuard, 1, kGuard + st.len + kGuard, o);
    std::fclose(o);
    std::printf("eth_lanes ok\n");
    return 0;
}
