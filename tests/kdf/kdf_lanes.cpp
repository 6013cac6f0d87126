// The lane bodies of plume_pbkdf2_sha512_batch (csrc/plume_kdf.h, csrc/plume_sha512.h) as host loops, for tests/test_kdf_lanes.py: g++ -fsanitize=address,undefined
// (Makefile).
// usage: kdf_lanes IN OUT     IN: u32 count, then per case u32 n, flags, salt_len, iterations, dklen, misalign, order (0: lanes descending, 1 ascending), u64 pw_bytes,
//                             n + 1 u64 offsets, pw_bytes password bytes, the salt (1 or n records of salt_len bytes).  The password buffer and the salt are allocations
//                             that END with their last byte and start `misalign` bytes into them: a load past either is a heap overflow.  The stages run lane by
//                             lane the way the kernels do: key, the remaining iterations in slices of PLUME_KDF_SLICE, finish.
//                             OUT: per case out (n x dklen) and status (n), each between its 32 guard bytes.
// The harness itself checks that the inputs and the guards are unchanged.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "plume_kdf.h"

using namespace plume;

constexpr size_t kGuard = 32;
struct Arr {                                             // an output off its alignment between guard bytes
    uint8_t* raw;
    uint8_t* p;
    size_t len, total;
    Arr(size_t bytes, size_t mis) : len(bytes), total(kGuard + 16 + bytes + kGuard) {
        raw = (uint8_t*)std::malloc(total);
        if (!raw) std::abort();
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
struct Exact {                                           // an input that ends with the last byte of its allocation
    uint8_t* raw;
    uint8_t* p;
    size_t len;
    std::vector<uint8_t> copy;
    Exact(size_t bytes, size_t mis) : len(bytes), copy(bytes) {
        raw = (uint8_t*)std::malloc((mis & 15u) + bytes + ((mis & 15u) + bytes ? 0 : 1));
        if (!raw) std::abort();
        p = raw + (mis & 15u);
    }
    ~Exact() { std::free(raw); }
    Exact(const Exact&) = delete;
    Exact& operator=(const Exact&) = delete;
    bool read(FILE* f) {
        if (len && std::fread(p, 1, len, f) != len) return false;
        if (len) std::memcpy(copy.data(), p, len);
        return true;
    }
    bool unchanged() const { return len == 0 || std::memcmp(p, copy.data(), len) == 0; }
};

static int run_case(FILE* f, FILE* o) {
    uint32_t h[7];
    uint64_t pw_bytes = 0;
    if (std::fread(h, 4, 7, f) != 7 || std::fread(&pw_bytes, 8, 1, f) != 1) return 2;
    const uint32_t n = h[0], flags = h[1], salt_len = h[2], iterations = h[3], dklen = h[4], mis = h[5], order = h[6];
    if (!n || salt_len > PLUME_KDFK_MAX_SALT || !iterations || dklen < 1 || dklen > 64 || pw_bytes > ((uint64_t)1 << 30)) return 2;
    std::vector<uint64_t> off(n + 1);
    if (std::fread(off.data(), 8, n + 1, f) != n + 1) return 2;
    const std::vector<uint64_t> off0 = off;
    Exact pw((size_t)pw_bytes, mis), salt((size_t)salt_len * ((flags & PLUME_KDFK_SHARED_SALT) ? 1 : n), mis + 3);
    if (!pw.read(f) || !salt.read(f)) return 2;
    Arr out((size_t)dklen * n, mis + 5), status(n, mis + 9);
    std::vector<uint64_t> ws((size_t)PLUME_KDFK_WS_WORDS * n);
    KdfArgs a;
    std::memset(&a, 0, sizeof a);
    a.flags = (int)flags; a.n = n; a.salt_len = salt_len; a.dklen = dklen;
    a.pw = pw_bytes ? pw.p : nullptr; a.pw_off = off.data(); a.pw_bytes = pw_bytes; a.salt = salt_len ? salt.p : nullptr; a.out = out.p; a.status = status.p; a.ws = ws.data();
    auto lanes = [&](auto body) {
        if (order) { for (uint32_t i = 0; i < n; i++) body(i); } else { for (uint32_t i = n; i-- > 0;) body(i); }
    };
    lanes([&](uint32_t i) { kdf_key_item(a, i); });
    for (uint32_t left = iterations - 1; left;) {
        a.iters = left < PLUME_KDF_SLICE ? left : PLUME_KDF_SLICE;
        lanes([&](uint32_t i) { kdf_iter_item(a, i); });
        left -= a.iters;
    }
    lanes([&](uint32_t i) { kdf_finish_item(a, i); });
    if (!pw.unchanged() || !salt.unchanged() || off != off0 || !out.untouched_outside() || !status.untouched_outside()) return 3;
    out.dump(o); status.dump(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    FILE* o = std::fopen(argv[2], "wb");
    if (!f || !o) return 2;
    uint32_t count = 0;
    if (std::fread(&count, 4, 1, f) != 1) return 2;
    for (uint32_t c = 0; c < count; c++) {
        if (int rc = run_case(f, o)) { std::fprintf(stderr, "kdf_lanes: case %u: %d\n", c, rc); return rc; }
    }
    uint8_t extra;
    if (std::fread(&extra, 1, 1, f) != 0) return 2;
    std::fclose(f);
    if (std::fclose(o) != 0) return 2;
    std::printf("kdf_lanes ok\n");
    return 0;
}
