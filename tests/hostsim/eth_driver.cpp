// TEST INFRASTRUCTURE ONLY.  plume_eth_address_batch* on the library's host side (csrc/plume_eth_capi.hip) on the mock HIP runtime, under the sanitizers (tests/test_eth_hostsim.py).
// usage: eth_driver VECTORS SEED.  VECTORS is written by the test from the Python restatement (tests/_keccak.py), for each key format (64-byte, then SEC1): u32 n, the n
// keys, n status bytes (1 valid / 3 no key), n raw addresses (zeros for an invalid key), n EIP-55 records (42 bytes, zeros likewise).  Every call must reproduce those
// bytes: the host form with chunks smaller than n, pageable and page-locked arrays, expect absent / matching / wrong, NULL address / NULL status, the device form on a
// caller stream (which must not have run anything when the call returns, under the lazy scheduler), plume_init_multi contexts over three and eight mock devices.  Then every
// allocation of a host-form call fails in turn: an error code, the outputs of a repeated call right, nothing leaked.  A context that only ever did this builds no table.
#define DRIVER_NAME "eth_driver"
#include "driver_prelude.h"

static const size_t kPk[2] = {64, 33}, kWidth[3] = {20, 64, 42};

struct Vectors {
    size_t n = 0;
    std::vector<uint8_t> pk, status, raw, eip;
};
static Vectors g_vec[2];

static void read_vectors(const char* path) {
    FILE* f = std::fopen(path, "rb");
    REQUIRE(f);
    for (int pf = 0; pf < 2; pf++) {
        uint32_t n = 0;
        REQUIRE(std::fread(&n, 4, 1, f) == 1 && n >= 60);
        Vectors& v = g_vec[pf];
        v.n = n; v.pk.resize(kPk[pf] * n); v.status.resize(n); v.raw.resize(20 * (size_t)n); v.eip.resize(42 * (size_t)n);
        REQUIRE(std::fread(v.pk.data(), kPk[pf], n, f) == n && std::fread(v.status.data(), 1, n, f) == n && std::fread(v.raw.data(), 20, n, f) == n &&
                std::fread(v.eip.data(), 42, n, f) == n);
    }
    std::fclose(f);
}

// items [lo, lo + n) of a key format's vectors; expect_mode 0 absent, 1 matching, 2 every third valid item wrong in one bit of byte (i % 20)
struct Call {
    int pf, af, expect_mode, kind;
    size_t lo, n;
    bool with_address, with_status;
    std::vector<uint8_t> want_addr, want_status, expect0;
    Arr pk, expect, address, status;
    Call(int pf_, int af_, size_t lo_, size_t n_, int expect_mode_, bool wa, bool ws, int k)
        : pf(pf_), af(af_), expect_mode(expect_mode_), kind(k), lo(lo_), n(n_), with_address(wa), with_status(ws), pk(kPk[pf_] * n_, k, g_vec[pf_].pk.data() + kPk[pf_] * lo_),
          expect(20 * n_, k), address(kWidth[af_] * n_, k), status(n_, k) {
        const Vectors& v = g_vec[pf];
        const size_t W = kWidth[af];
        want_addr.assign(W * n, 0); want_status.assign(n, 0); expect0.assign(20 * n, 0);
        for (size_t i = 0; i < n; i++) {
            const uint8_t* raw = &v.raw[20 * (lo + i)];
            const bool valid = v.status[lo + i] == PLUME_ETH_MATCH;
            REQUIRE(valid || (v.status[lo + i] == PLUME_ETH_INVALID && all_of(raw, 20, 0)));
            if (af == PLUME_ETH_ADDR_RAW20) std::memcpy(&want_addr[W * i], raw, 20);
            else if (af == PLUME_ETH_ADDR_RECORD64) std::memcpy(&want_addr[W * i + 44], raw, 20);
            else std::memcpy(&want_addr[W * i], &v.eip[42 * (lo + i)], 42);
            std::memcpy(&expect0[20 * i], raw, 20);
            bool wrong = expect_mode == 2 && (lo + i) % 3 == 0;
            if (wrong) expect0[20 * i + (lo + i) % 20] ^= (uint8_t)(1u << ((lo + i) % 8));
            want_status[i] = (uint8_t)(!valid ? PLUME_ETH_INVALID : wrong ? PLUME_ETH_MISMATCH : PLUME_ETH_MATCH);
        }
        std::memcpy(expect.p, expect0.data(), 20 * n);
    }
    int run(plume_ctx* ctx, hipStream_t st) {
        const uint8_t* e = expect_mode ? expect.p : nullptr;
        uint8_t *a = with_address ? address.p : nullptr, *s = with_status ? status.p : nullptr;
        if (kind == 2) return plume_eth_address_batch_device(ctx, pf, af, n, pk.p, e, a, s, st);
        return plume_eth_address_batch(ctx, pf, af, n, pk.p, e, a, s);
    }
    bool untouched() const { return all_of(address.p, address.bytes, kFill) && all_of(status.p, status.bytes, kFill); }
    void check() {                                        // (the mock's device memory is host memory)
        if (with_address) REQUIRE(std::memcmp(address.p, want_addr.data(), want_addr.size()) == 0); else REQUIRE(all_of(address.p, address.bytes, kFill));
        if (with_status) REQUIRE(std::memcmp(status.p, want_status.data(), n) == 0); else REQUIRE(all_of(status.p, status.bytes, kFill));
        REQUIRE(std::memcmp(pk.p, g_vec[pf].pk.data() + kPk[pf] * lo, pk.bytes) == 0 && std::memcmp(expect.p, expect0.data(), 20 * n) == 0);
    }
};

static void group(plume_ctx* ctx, const char* what, int calls, bool device_form, size_t chunk) {
    const bool lazy = std::getenv("PLUME_MOCK_SCHED") == nullptr;
    hipStream_t st = nullptr;
    if (device_form) REQUIRE(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
    if (chunk) REQUIRE(plume_set_chunk(ctx, chunk) == 0);
    for (int k = 0; k < calls; k++) {
        const int pf = k & 1, af = (k / 2) % 3, mode = k < 6 ? k % 3 : (int)(rng() % 3);
        const size_t total = g_vec[pf].n, n = k < 6 ? total : 1 + rng() % total, lo = rng() % (total - n + 1);
        const int outs = k < 6 ? 3 : mode == 0 ? 1 + 2 * (int)(rng() & 1) : 1 + (int)(rng() % 3);          // bit 0 address, bit 1 status; status alone only with expect
        g_what = std::string(what) + " call " + std::to_string(k) + ": n " + std::to_string(n) + " from " + std::to_string(lo) + ", pk format " + std::to_string(pf) +
                 ", address format " + std::to_string(af) + ", expect " + std::to_string(mode) + ", outputs " + std::to_string(outs) + ", chunk " + std::to_string(chunk);
        Call c(pf, af, lo, n, mode, (outs & 1) != 0, (outs & 2) != 0, device_form ? 2 : (int)(rng() & 1));
        REQUIRE(c.run(ctx, st) == 0);
        if (device_form) {
            if (lazy) REQUIRE(c.untouched());                                      // enqueued, not run: the device form does not synchronise
            REQUIRE(hipStreamSynchronize(st) == hipSuccess);
        }
        c.check();
    }
    if (st) REQUIRE(hipStreamDestroy(st) == hipSuccess);
}

// two calls queued back to back on one caller stream, compared after one synchronise
static void group_back_to_back(plume_ctx* ctx) {
    g_what = "two calls on one caller stream";
    hipStream_t st = nullptr;
    REQUIRE(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
    Call a(0, 2, 0, g_vec[0].n, 2, true, true, 2), b(1, 1, 3, g_vec[1].n - 3, 1, true, true, 2);
    REQUIRE(a.run(ctx, st) == 0 && b.run(ctx, st) == 0);
    REQUIRE(hipStreamSynchronize(st) == hipSuccess);
    a.check(); b.check();
    REQUIRE(hipStreamDestroy(st) == hipSuccess);
}

static void group_arguments(plume_ctx* ctx) {
    g_what = "arguments";
    const Vectors& v = g_vec[0];
    std::vector<uint8_t> o(64 * 4, kFill), s(4, kFill);
    auto call = [&](plume_ctx* c, int pf, int af, size_t n, const uint8_t* pk, const uint8_t* e, uint8_t* a, uint8_t* st) { return plume_eth_address_batch(c, pf, af, n, pk, e, a, st); };
    REQUIRE(call(nullptr, 0, 0, 4, v.pk.data(), nullptr, o.data(), s.data()) == PLUME_ERR_ARG);
    REQUIRE(call(ctx, 2, 0, 4, v.pk.data(), nullptr, o.data(), s.data()) == PLUME_ERR_ARG && call(ctx, -1, 0, 4, v.pk.data(), nullptr, o.data(), s.data()) == PLUME_ERR_ARG);
    REQUIRE(call(ctx, 0, 3, 4, v.pk.data(), nullptr, o.data(), s.data()) == PLUME_ERR_ARG && call(ctx, 0, -1, 4, v.pk.data(), nullptr, o.data(), s.data()) == PLUME_ERR_ARG);
    REQUIRE(call(ctx, 0, 0, 4, nullptr, nullptr, o.data(), s.data()) == PLUME_ERR_ARG);
    REQUIRE(call(ctx, 0, 0, 4, v.pk.data(), v.raw.data(), nullptr, nullptr) == PLUME_ERR_ARG && std::string(plume_last_error()) == "no output array");
    REQUIRE(call(ctx, 0, 0, 0, nullptr, nullptr, nullptr, nullptr) == 0);              // an empty batch is no error, as for verify
    REQUIRE(all_of(o.data(), o.size(), kFill) && all_of(s.data(), s.size(), kFill));
    plume_ctx* multi = nullptr;
    int ids[2] = {0, 1};
    REQUIRE(plume_init_multi(&multi, ids, 2) == 0);
    Call d(0, 0, 0, 8, 0, true, true, 2);
    REQUIRE(d.run(multi, nullptr) == PLUME_ERR_ARG);                                   // device pointers belong to one GPU
    plume_destroy(multi);
    REQUIRE(plume_set_chunk(ctx, 3) == 0);                                             // the device form is one launch whatever the chunk size is
    REQUIRE(d.run(ctx, nullptr) == 0);
    REQUIRE(plume_set_chunk(ctx, (size_t)1 << 20) == 0);
    plume_destroy(ctx);                                                                // (waits for nothing of this call: it used no workspace)
    REQUIRE(hipDeviceSynchronize() == hipSuccess);
    d.check();
}

// every allocation of one host-form call fails in turn
static void group_failing_allocations() {
    const Outstanding before;
    plume_ctx* ctx = nullptr;
    REQUIRE(plume_init(&ctx, 0) == 0);
    (void)mockhip::fail_allocation(-1);
    { Call c(0, 2, 0, 50, 1, true, true, 0); g_what = "allocations: counting call"; REQUIRE(c.run(ctx, nullptr) == 0); c.check(); }
    const long made = mockhip::fail_allocation(-1);
    REQUIRE(made == 4);                                                                // pk, expect, address, status staging -- and no table
    plume_destroy(ctx);
    for (long k = 0; k < made; k++) {
        g_what = "allocations: number " + std::to_string(k) + " fails";
        REQUIRE(plume_init(&ctx, 0) == 0);
        Call c(1, 1, 2, 50, 2, true, true, (int)(k & 1));
        (void)mockhip::fail_allocation(k);
        REQUIRE(c.run(ctx, nullptr) == PLUME_ERR_HIP && std::string(plume_last_error()).find("hipMalloc") != std::string::npos);
        REQUIRE(c.untouched());
        (void)mockhip::fail_allocation(-1);
        REQUIRE(c.run(ctx, nullptr) == 0);                                             // the context is usable afterwards
        c.check();
        plume_destroy(ctx);
    }
    REQUIRE(Outstanding() == before);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    read_vectors(argv[1]);
    const unsigned long long seed = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1;
    rng.seed(seed);
    plume_ctx* ctx = nullptr;
    REQUIRE(plume_init(&ctx, 0) == 0);
    const long dev_after_init = mockhip::outstanding(0);
    group(ctx, "one device, host form, one chunk", 6, false, 0);
    group(ctx, "one device, host form, chunks of 7", 10, false, 7);
    group(ctx, "one device, host form, chunks of 1", 2, false, 1);
    REQUIRE(plume_set_chunk(ctx, (size_t)1 << 20) == 0);
    group(ctx, "one device, device form", 10, true, 0);
    group_back_to_back(ctx);
    g_what = "no table";
    REQUIRE(mockhip::outstanding(0) <= dev_after_init + 4);                            // the four staging buffers of the host form: no table, no workspace
    for (int devices : {3, 8}) {
        plume_ctx* multi = nullptr;
        int ids[8] = {0, 1, 2, 3, 4, 5, 6, 7};
        REQUIRE(plume_init_multi(&multi, ids, devices) == 0);
        REQUIRE(plume_num_shards(multi) == devices);
        group(multi, devices == 3 ? "three devices, host form" : "eight devices, host form", 8, false, devices == 3 ? 5 : 0);
        plume_destroy(multi);
    }
    group_arguments(ctx);                                                              // (destroys ctx)
    group_failing_allocations();
    REQUIRE(mockhip::outstanding(0) == 0 && mockhip::outstanding(2) == 0 && mockhip::outstanding(3) == 0);
    std::printf("eth_driver seed %llu: ok\n", seed);
    return 0;
}
