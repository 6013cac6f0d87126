// TEST INFRASTRUCTURE ONLY.  plume_ecdsa_recover_batch* on the library's host side (csrc/plume_ecdsa_capi.hip) on the mock HIP runtime, under the sanitizers (tests/test_ecdsa_hostsim.py).
// usage: ecdsa_driver VECTORS SEED.  VECTORS is written by the test from the Python restatement (tests/_ecdsa.py): u32 n, then n hashes, n r, n s (32 bytes each), n v
// (1 byte), n status bytes (1 recovered / 3 invalid), n keys of 64 bytes, n raw addresses, n EIP-55 records of 42 bytes (zeros for an invalid item).  Every call must
// reproduce those bytes: the host form with chunks of 1, 64 and n, pageable and page-locked arrays, expect absent / matching / wrong, each output NULL, the device form on
// a caller stream (which must not have run anything when the call returns, under the lazy scheduler) with and without sub-batches, a plume_init_multi context over eight
// mock devices.  Then the argument errors, and every allocation of a host-form call failing in turn: an error code, the outputs of a repeated call right, nothing leaked.
// A context that only ever did this builds the comb and no window table.
#define DRIVER_NAME "ecdsa_driver"
#include "driver_prelude.h"

static const size_t kPk[2] = {64, 33}, kWidth[3] = {20, 64, 42};

static size_t g_n = 0;
static std::vector<uint8_t> g_hash, g_r, g_s, g_v, g_status, g_pk, g_raw, g_eip;

static void read_vectors(const char* path) {
    FILE* f = std::fopen(path, "rb");
    REQUIRE(f);
    uint32_t n = 0;
    REQUIRE(std::fread(&n, 4, 1, f) == 1 && n >= 100);
    g_n = n;
    g_hash.resize(32 * g_n); g_r.resize(32 * g_n); g_s.resize(32 * g_n); g_v.resize(g_n); g_status.resize(g_n); g_pk.resize(64 * g_n); g_raw.resize(20 * g_n); g_eip.resize(42 * g_n);
    REQUIRE(std::fread(g_hash.data(), 32, n, f) == n && std::fread(g_r.data(), 32, n, f) == n && std::fread(g_s.data(), 32, n, f) == n && std::fread(g_v.data(), 1, n, f) == n &&
            std::fread(g_status.data(), 1, n, f) == n && std::fread(g_pk.data(), 64, n, f) == n && std::fread(g_raw.data(), 20, n, f) == n && std::fread(g_eip.data(), 42, n, f) == n);
    std::fclose(f);
}

// items [lo, lo + n) of the vectors; expect_mode 0 absent, 1 matching, 2 every third item wrong in one bit of byte (i % 20); outs: bit 0 pk, bit 1 address, bit 2 status
struct Call {
    int pf, af, expect_mode, kind, outs;
    size_t lo, n;
    std::vector<uint8_t> want_pk, want_addr, want_status, expect0;
    Arr hash, r, s, v, expect, pk, address, status;
    Call(int pf_, int af_, size_t lo_, size_t n_, int expect_mode_, int outs_, int k)
        : pf(pf_), af(af_), expect_mode(expect_mode_), kind(k), outs(outs_), lo(lo_), n(n_), hash(32 * n_, k, g_hash.data() + 32 * lo_), r(32 * n_, k, g_r.data() + 32 * lo_),
          s(32 * n_, k, g_s.data() + 32 * lo_), v(n_, k, g_v.data() + lo_), expect(20 * n_, k), pk(kPk[pf_] * n_, k), address(kWidth[af_] * n_, k), status(n_, k) {
        const size_t P = kPk[pf], W = kWidth[af];
        want_pk.assign(P * n, 0); want_addr.assign(W * n, 0); want_status.assign(n, 0); expect0.assign(20 * n, 0);
        for (size_t i = 0; i < n; i++) {
            const uint8_t* raw = &g_raw[20 * (lo + i)];
            const uint8_t* key = &g_pk[64 * (lo + i)];
            const bool valid = g_status[lo + i] == PLUME_ECDSA_MATCH;
            REQUIRE(valid || (g_status[lo + i] == PLUME_ECDSA_INVALID && all_of(raw, 20, 0) && all_of(key, 64, 0)));
            if (valid) {
                if (pf == PLUME_ETH_PK_AFFINE64) std::memcpy(&want_pk[P * i], key, 64);
                else { want_pk[P * i] = (uint8_t)(2 + (key[63] & 1)); std::memcpy(&want_pk[P * i + 1], key, 32); }
            }
            if (af == PLUME_ETH_ADDR_RAW20) std::memcpy(&want_addr[W * i], raw, 20);
            else if (af == PLUME_ETH_ADDR_RECORD64) std::memcpy(&want_addr[W * i + 44], raw, 20);
            else std::memcpy(&want_addr[W * i], &g_eip[42 * (lo + i)], 42);
            std::memcpy(&expect0[20 * i], raw, 20);
            const bool wrong = expect_mode == 2 && (lo + i) % 3 == 0;
            if (wrong) expect0[20 * i + (lo + i) % 20] ^= (uint8_t)(1u << ((lo + i) % 8));
            want_status[i] = (uint8_t)(!valid ? PLUME_ECDSA_INVALID : wrong ? PLUME_ECDSA_MISMATCH : PLUME_ECDSA_MATCH);
        }
        std::memcpy(expect.p, expect0.data(), 20 * n);
    }
    int run(plume_ctx* ctx, hipStream_t st) {
        const uint8_t* e = expect_mode ? expect.p : nullptr;
        uint8_t *k = (outs & 1) ? pk.p : nullptr, *a = (outs & 2) ? address.p : nullptr, *t = (outs & 4) ? status.p : nullptr;
        if (kind == 2) return plume_ecdsa_recover_batch_device(ctx, 0, pf, af, n, hash.p, r.p, s.p, v.p, e, k, a, t, st);
        return plume_ecdsa_recover_batch(ctx, 0, pf, af, n, hash.p, r.p, s.p, v.p, e, k, a, t);
    }
    bool untouched() const { return all_of(pk.p, pk.bytes, kFill) && all_of(address.p, address.bytes, kFill) && all_of(status.p, status.bytes, kFill); }
    void check() {                                        // (the mock's device memory is host memory)
        if (outs & 1) REQUIRE(std::memcmp(pk.p, want_pk.data(), want_pk.size()) == 0); else REQUIRE(all_of(pk.p, pk.bytes, kFill));
        if (outs & 2) REQUIRE(std::memcmp(address.p, want_addr.data(), want_addr.size()) == 0); else REQUIRE(all_of(address.p, address.bytes, kFill));
        if (outs & 4) REQUIRE(std::memcmp(status.p, want_status.data(), n) == 0); else REQUIRE(all_of(status.p, status.bytes, kFill));
        REQUIRE(std::memcmp(hash.p, g_hash.data() + 32 * lo, 32 * n) == 0 && std::memcmp(r.p, g_r.data() + 32 * lo, 32 * n) == 0 && std::memcmp(s.p, g_s.data() + 32 * lo, 32 * n) == 0 &&
                std::memcmp(v.p, g_v.data() + lo, n) == 0 && std::memcmp(expect.p, expect0.data(), 20 * n) == 0);
    }
};

static void group(plume_ctx* ctx, const char* what, int calls, bool device_form, size_t chunk) {
    const bool lazy = std::getenv("PLUME_MOCK_SCHED") == nullptr;
    hipStream_t st = nullptr;
    if (device_form) REQUIRE(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
    if (chunk) REQUIRE(plume_set_chunk(ctx, chunk) == 0);
    for (int k = 0; k < calls; k++) {
        const int pf = k & 1, af = (k / 2) % 3, mode = k < 3 ? k : (int)(rng() % 3);
        const size_t n = k < 2 ? g_n : 1 + rng() % g_n, lo = rng() % (g_n - n + 1);
        const int outs = k < 3 ? 7 : 1 + (int)(rng() % 7);
        g_what = std::string(what) + " call " + std::to_string(k) + ": n " + std::to_string(n) + " from " + std::to_string(lo) + ", pk format " + std::to_string(pf) +
                 ", address format " + std::to_string(af) + ", expect " + std::to_string(mode) + ", outputs " + std::to_string(outs) + ", chunk " + std::to_string(chunk);
        Call c(pf, af, lo, n, mode, outs, device_form ? 2 : (int)(rng() & 1));
        REQUIRE(c.run(ctx, st) == 0);
        if (device_form) {
            if (lazy) REQUIRE(c.untouched());                                      // enqueued, not run: the device form does not synchronise
            REQUIRE(hipStreamSynchronize(st) == hipSuccess);
        }
        c.check();
    }
    if (st) REQUIRE(hipStreamDestroy(st) == hipSuccess);
}

// two calls queued back to back on one caller stream and a third on another stream of the same context (the workspace event orders it), compared after the synchronises
static void group_streams(plume_ctx* ctx) {
    g_what = "calls on two caller streams";
    hipStream_t st = nullptr, st2 = nullptr;
    REQUIRE(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess && hipStreamCreateWithFlags(&st2, hipStreamNonBlocking) == hipSuccess);
    Call a(0, 2, 0, g_n, 2, 7, 2), b(1, 1, 3, g_n - 3, 1, 7, 2), c(1, 0, 10, 70, 0, 7, 2);
    REQUIRE(a.run(ctx, st) == 0 && b.run(ctx, st) == 0 && c.run(ctx, st2) == 0);
    REQUIRE(hipStreamSynchronize(st2) == hipSuccess && hipStreamSynchronize(st) == hipSuccess);
    a.check(); b.check(); c.check();
    REQUIRE(hipStreamDestroy(st) == hipSuccess && hipStreamDestroy(st2) == hipSuccess);
}

static void group_arguments(plume_ctx* ctx) {
    g_what = "arguments";
    std::vector<uint8_t> o(64 * 4, kFill), a(64 * 4, kFill), t(4, kFill);
    auto call = [&](plume_ctx* c, int flags, int pf, int af, size_t n, const uint8_t* h, const uint8_t* v, uint8_t* pk, uint8_t* ad, uint8_t* st) {
        return plume_ecdsa_recover_batch(c, flags, pf, af, n, h, g_r.data(), g_s.data(), v, nullptr, pk, ad, st);
    };
    const uint8_t *h = g_hash.data(), *v = g_v.data();
    REQUIRE(call(nullptr, 0, 0, 0, 4, h, v, o.data(), a.data(), t.data()) == PLUME_ERR_ARG);
    REQUIRE(call(ctx, 2, 0, 0, 4, h, v, o.data(), a.data(), t.data()) == PLUME_ERR_ARG && call(ctx, 3, 0, 0, 4, h, v, o.data(), a.data(), t.data()) == PLUME_ERR_ARG &&
            call(ctx, -1, 0, 0, 4, h, v, o.data(), a.data(), t.data()) == PLUME_ERR_ARG);
    REQUIRE(call(ctx, 0, 2, 0, 4, h, v, o.data(), a.data(), t.data()) == PLUME_ERR_ARG && call(ctx, 0, -1, 0, 4, h, v, o.data(), a.data(), t.data()) == PLUME_ERR_ARG);
    REQUIRE(call(ctx, 0, 0, 3, 4, h, v, o.data(), a.data(), t.data()) == PLUME_ERR_ARG && call(ctx, 0, 0, -1, 4, h, v, o.data(), a.data(), t.data()) == PLUME_ERR_ARG);
    REQUIRE(call(ctx, 0, 0, 0, 4, nullptr, v, o.data(), a.data(), t.data()) == PLUME_ERR_ARG && call(ctx, 0, 0, 0, 4, h, nullptr, o.data(), a.data(), t.data()) == PLUME_ERR_ARG);
    REQUIRE(call(ctx, 0, 0, 0, 4, h, v, nullptr, nullptr, nullptr) == PLUME_ERR_ARG && std::string(plume_last_error()) == "no output array");
    REQUIRE(call(ctx, 1, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);              // an empty batch is a successful no-op
    REQUIRE(all_of(o.data(), o.size(), kFill) && all_of(a.data(), a.size(), kFill) && all_of(t.data(), t.size(), kFill));
    plume_ctx* multi = nullptr;
    int ids[2] = {0, 1};
    REQUIRE(plume_init_multi(&multi, ids, 2) == 0);
    Call d(0, 0, 0, 8, 0, 7, 2);
    REQUIRE(d.run(multi, nullptr) == PLUME_ERR_ARG);                                   // device pointers belong to one GPU
    plume_destroy(multi);
    REQUIRE(plume_set_chunk(ctx, 3) == 0);                                             // the device form is one call of at most a chunk, as for verify
    REQUIRE(d.run(ctx, nullptr) == PLUME_ERR_ARG && d.untouched());
    REQUIRE(plume_set_chunk(ctx, (size_t)1 << 20) == 0);
    REQUIRE(d.run(ctx, nullptr) == 0);
    plume_destroy(ctx);                                                                // waits for the call: it used the context's workspace
    d.check();
}

// every allocation of one host-form call fails in turn.  A second context stays open meanwhile, so that the comb (shared per device) is built once
static void group_failing_allocations() {
    plume_ctx* keeper = nullptr;
    REQUIRE(plume_init(&keeper, 0) == 0);
    { Call c(0, 0, 0, 4, 0, 7, 0); g_what = "allocations: the comb"; REQUIRE(c.run(keeper, nullptr) == 0); c.check(); }
    const Outstanding before;
    plume_ctx* ctx = nullptr;
    REQUIRE(plume_init(&ctx, 0) == 0);
    (void)mockhip::fail_allocation(-1);
    { Call c(0, 2, 0, 50, 1, 7, 0); g_what = "allocations: counting call"; REQUIRE(c.run(ctx, nullptr) == 0); c.check(); }
    const long made = mockhip::fail_allocation(-1);
    REQUIRE(made == 18);                                                               // 8 staging buffers, 10 workspace buffers -- and no table: the comb is there already
    plume_destroy(ctx);
    for (long k = 0; k < made; k++) {
        g_what = "allocations: number " + std::to_string(k) + " fails";
        REQUIRE(plume_init(&ctx, 0) == 0);
        Call c(1, 1, 2, 50, 2, 7, (int)(k & 1));
        (void)mockhip::fail_allocation(k);
        REQUIRE(c.run(ctx, nullptr) == PLUME_ERR_HIP && std::string(plume_last_error()).find("hipMalloc") != std::string::npos);
        REQUIRE(c.untouched());
        (void)mockhip::fail_allocation(-1);
        REQUIRE(c.run(ctx, nullptr) == 0);                                             // the context is usable afterwards
        c.check();
        plume_destroy(ctx);
    }
    REQUIRE(Outstanding() == before);
    plume_destroy(keeper);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    read_vectors(argv[1]);
    const unsigned long long seed = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1;
    rng.seed(seed);
    plume_ctx* ctx = nullptr;
    REQUIRE(plume_init(&ctx, 0) == 0);
    REQUIRE(std::string(plume_version()).find("plume_hip 0.12 ") == 0);
    group(ctx, "one device, host form, one chunk", 5, false, g_n);
    group(ctx, "one device, host form, chunks of 64", 4, false, 64);
    group(ctx, "one device, host form, chunks of 1", 2, false, 1);
    REQUIRE(plume_set_chunk(ctx, (size_t)1 << 20) == 0);
    group(ctx, "one device, device form", 6, true, 0);
    REQUIRE(plume_set_sub_batches(ctx, 3) == 0);
    group(ctx, "one device, device form, three sub-batches", 3, true, 0);
    REQUIRE(plume_set_sub_batches(ctx, 1) == 0);
    group_streams(ctx);
    {
        plume_ctx* multi = nullptr;
        int ids[8] = {0, 1, 2, 3, 4, 5, 6, 7};
        REQUIRE(plume_init_multi(&multi, ids, 8) == 0);
        REQUIRE(plume_num_shards(multi) == 8);
        group(multi, "eight devices, host form", 4, false, 0);
        group(multi, "eight devices, host form, chunks of 5", 2, false, 5);
        plume_destroy(multi);
    }
    group_arguments(ctx);                                                              // (destroys ctx)
    group_failing_allocations();
    REQUIRE(mockhip::outstanding(0) == 0 && mockhip::outstanding(2) == 0 && mockhip::outstanding(3) == 0);
    std::printf("ecdsa_driver seed %llu: ok\n", seed);
    return 0;
}
