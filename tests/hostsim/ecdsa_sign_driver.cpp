// TEST INFRASTRUCTURE ONLY.  plume_ecdsa_sign_batch* and plume_eth_message_hash_batch* on the library's host side (csrc/plume_ecdsa_sign_capi.hip, csrc/plume_eth_hash_capi.hip) on the mock HIP runtime, under the sanitizers (tests/test_ecdsa_sign_hostsim.py).
// usage: ecdsa_sign_driver VECTORS SEED.  VECTORS is written by the test from the Python restatement (tests/_ecdsa_sign.py): u32 n, n hashes, n sk, n aux (32 bytes each),
// then what the call gives without aux and with it -- n r, n s (32 bytes), n v in {0, 1}, n status bytes, twice; then u32 m, m + 1 u64 message offsets, the message bytes,
// m digests of mode 0 and m of mode 1.  Every call must reproduce those bytes: the host form with chunks smaller than n, pageable and page-locked arrays, the device form
// on a caller stream (which must not have run anything when the call returns, under the lazy scheduler), the three uniform levels, sub-batches, the self-check on (same
// bytes, the stage list of the header), plume_init_multi contexts over three and eight mock devices, argument errors; then every allocation of a call fails in turn -- an
// error code, a repeated call right, nothing leaked; and after every sign call no device allocation holds a nonce of the batch.
#define DRIVER_NAME "ecdsa_sign_driver"
#include "driver_prelude.h"

static size_t g_n = 0, g_m = 0;
static std::vector<uint8_t> g_hash, g_sk, g_aux, g_r[2], g_s[2], g_v[2], g_st[2], g_msgs, g_dg[2];
static std::vector<uint64_t> g_off;

static void read_vectors(const char* path) {
    FILE* f = std::fopen(path, "rb");
    REQUIRE(f);
    uint32_t n = 0, m = 0;
    REQUIRE(std::fread(&n, 4, 1, f) == 1 && n >= 40);
    g_n = n;
    for (std::vector<uint8_t>* v : {&g_hash, &g_sk, &g_aux}) { v->resize(32 * g_n); REQUIRE(std::fread(v->data(), 32, n, f) == n); }
    for (int h = 0; h < 2; h++) {
        g_r[h].resize(32 * g_n); g_s[h].resize(32 * g_n); g_v[h].resize(g_n); g_st[h].resize(g_n);
        REQUIRE(std::fread(g_r[h].data(), 32, n, f) == n && std::fread(g_s[h].data(), 32, n, f) == n && std::fread(g_v[h].data(), 1, n, f) == n && std::fread(g_st[h].data(), 1, n, f) == n);
    }
    REQUIRE(std::fread(&m, 4, 1, f) == 1 && m >= 20);
    g_m = m;
    g_off.resize(g_m + 1);
    REQUIRE(std::fread(g_off.data(), 8, g_m + 1, f) == g_m + 1);
    g_msgs.resize((size_t)g_off[g_m] + 16);
    REQUIRE(std::fread(g_msgs.data(), 1, (size_t)g_off[g_m], f) == (size_t)g_off[g_m]);
    for (int mode = 0; mode < 2; mode++) { g_dg[mode].resize(32 * g_m); REQUIRE(std::fread(g_dg[mode].data(), 32, m, f) == m); }
    std::fclose(f);
}

// items [lo, lo + n) signed with or without aux, v as 0 / 1 or 27 / 28
struct SignCall {
    size_t lo, n;
    bool hedged, v27;
    int kind;
    Arr hash, sk, aux, r, s, v, st;
    SignCall(size_t lo_, size_t n_, bool hedged_, bool v27_, int k)
        : lo(lo_), n(n_), hedged(hedged_), v27(v27_), kind(k), hash(32 * n_, k, &g_hash[32 * lo_]), sk(32 * n_, k, &g_sk[32 * lo_]), aux(32 * n_, k, &g_aux[32 * lo_]), r(32 * n_, k),
          s(32 * n_, k), v(n_, k), st(n_, k) {}
    int run(plume_ctx* ctx, hipStream_t stream) {
        const int flags = v27 ? PLUME_ECDSA_SIGN_V27 : 0;
        const uint8_t* a = hedged ? aux.p : nullptr;
        if (kind == 2) return plume_ecdsa_sign_batch_device(ctx, flags, n, hash.p, sk.p, a, r.p, s.p, v.p, st.p, stream);
        return plume_ecdsa_sign_batch(ctx, flags, n, hash.p, sk.p, a, r.p, s.p, v.p, st.p);
    }
    bool untouched() const { return all_of(r.p, r.bytes, kFill) && all_of(s.p, s.bytes, kFill) && all_of(v.p, v.bytes, kFill) && all_of(st.p, st.bytes, kFill); }
    void check() {                                        // (the mock's device memory is host memory)
        const int h = hedged ? 1 : 0;
        REQUIRE(std::memcmp(st.p, &g_st[h][lo], n) == 0);
        REQUIRE(std::memcmp(r.p, &g_r[h][32 * lo], 32 * n) == 0 && std::memcmp(s.p, &g_s[h][32 * lo], 32 * n) == 0);
        for (size_t i = 0; i < n; i++) REQUIRE(v.p[i] == (g_st[h][lo + i] ? 0 : g_v[h][lo + i] + (v27 ? 27 : 0)));
        REQUIRE(std::memcmp(hash.p, &g_hash[32 * lo], 32 * n) == 0 && std::memcmp(sk.p, &g_sk[32 * lo], 32 * n) == 0 && std::memcmp(aux.p, &g_aux[32 * lo], 32 * n) == 0);
    }
};

static void sign_group(plume_ctx* ctx, const char* what, int calls, bool device_form, size_t chunk) {
    const bool lazy = std::getenv("PLUME_MOCK_SCHED") == nullptr;
    hipStream_t st = nullptr;
    if (device_form) REQUIRE(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
    if (chunk) REQUIRE(plume_set_chunk(ctx, chunk) == 0);
    for (int k = 0; k < calls; k++) {
        const size_t n = k < 2 ? g_n : 1 + rng() % g_n, lo = rng() % (g_n - n + 1);
        const bool hedged = (k & 1) != 0, v27 = ((k >> 1) & 1) != 0;
        g_what = std::string(what) + " call " + std::to_string(k) + ": n " + std::to_string(n) + " from " + std::to_string(lo) + (hedged ? ", hedged" : "") + (v27 ? ", v27" : "") +
                 ", chunk " + std::to_string(chunk);
        SignCall c(lo, n, hedged, v27, device_form ? 2 : (int)(rng() & 1));
        REQUIRE(c.run(ctx, st) == 0);
        if (device_form) {
            if (lazy) REQUIRE(c.untouched());                                      // enqueued, not run: the device form does not synchronise
            REQUIRE(hipStreamSynchronize(st) == hipSuccess);
        }
        c.check();
    }
    if (st) REQUIRE(hipStreamDestroy(st) == hipSuccess);
}

static void hash_group(plume_ctx* ctx, const char* what, bool device_form, size_t chunk) {
    hipStream_t st = nullptr;
    if (device_form) REQUIRE(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
    if (chunk) REQUIRE(plume_set_chunk(ctx, chunk) == 0);
    for (int mode = 0; mode < 2; mode++) {
        g_what = std::string(what) + ", mode " + std::to_string(mode) + ", chunk " + std::to_string(chunk);
        const int kind = device_form ? 2 : mode;
        Arr msgs(g_msgs.size(), kind, g_msgs.data()), off(8 * (g_m + 1), kind, g_off.data()), out(32 * g_m, kind);
        if (device_form) {
            REQUIRE(plume_eth_message_hash_batch_device(ctx, mode, g_m, msgs.p, (const uint64_t*)off.p, (size_t)g_off[g_m], out.p, st) == 0);
            if (std::getenv("PLUME_MOCK_SCHED") == nullptr) REQUIRE(all_of(out.p, out.bytes, kFill));
            REQUIRE(hipStreamSynchronize(st) == hipSuccess);
        } else {
            REQUIRE(plume_eth_message_hash_batch(ctx, mode, g_m, msgs.p, (const uint64_t*)off.p, out.p) == 0);
        }
        REQUIRE(std::memcmp(out.p, g_dg[mode].data(), 32 * g_m) == 0);
        REQUIRE(std::memcmp(msgs.p, g_msgs.data(), g_msgs.size()) == 0);
    }
    if (st) REQUIRE(hipStreamDestroy(st) == hipSuccess);
}

static std::vector<std::string> stages_of_a_device_call(plume_ctx* ctx) {
    hipStream_t st = nullptr;
    REQUIRE(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
    REQUIRE(plume_set_stage_timing(ctx, 1) == 0);
    SignCall c(0, g_n, false, true, 2);
    REQUIRE(c.run(ctx, st) == 0 && hipStreamSynchronize(st) == hipSuccess);
    c.check();
    const std::vector<std::string> names = last_stage_names(ctx);
    REQUIRE(plume_set_stage_timing(ctx, 0) == 0);
    REQUIRE(hipStreamDestroy(st) == hipSuccess);
    return names;
}

static void group_arguments(plume_ctx* ctx) {
    g_what = "arguments";
    SignCall c(0, 4, false, false, 0);
    for (int flags : {2, 3, 0x100, -1}) REQUIRE(plume_ecdsa_sign_batch(ctx, flags, 4, c.hash.p, c.sk.p, nullptr, c.r.p, c.s.p, c.v.p, c.st.p) == PLUME_ERR_ARG);
    REQUIRE(plume_ecdsa_sign_batch(ctx, 0, 4, nullptr, c.sk.p, nullptr, c.r.p, c.s.p, c.v.p, c.st.p) == PLUME_ERR_ARG);
    REQUIRE(plume_ecdsa_sign_batch(ctx, 0, 4, c.hash.p, c.sk.p, nullptr, c.r.p, c.s.p, nullptr, c.st.p) == PLUME_ERR_ARG);
    REQUIRE(plume_ecdsa_sign_batch(nullptr, 0, 4, c.hash.p, c.sk.p, nullptr, c.r.p, c.s.p, c.v.p, c.st.p) == PLUME_ERR_ARG);
    REQUIRE(c.untouched());
    REQUIRE(plume_ecdsa_sign_batch(ctx, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    REQUIRE(plume_ecdsa_sign_batch_device(ctx, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    uint8_t out[32];
    const uint64_t off[2] = {0, 3};
    for (int mode : {2, -1}) REQUIRE(plume_eth_message_hash_batch(ctx, mode, 1, (const uint8_t*)"abc", off, out) == PLUME_ERR_ARG);
    REQUIRE(plume_eth_message_hash_batch(ctx, 0, 1, (const uint8_t*)"abc", nullptr, out) == PLUME_ERR_ARG);
    REQUIRE(plume_eth_message_hash_batch(ctx, 0, 0, nullptr, nullptr, nullptr) == 0);
    const uint64_t down[3] = {2, 1, 3};
    uint8_t out2[64];
    REQUIRE(plume_eth_message_hash_batch(ctx, 0, 2, (const uint8_t*)"abc", down, out2) == PLUME_ERR_ARG);      // the host form refuses decreasing offsets
    REQUIRE(plume_set_chunk(ctx, 8) == 0);
    {
        SignCall d(0, 9, false, false, 2);                                           // the device form takes at most a chunk
        REQUIRE(plume_ecdsa_sign_batch_device(ctx, 0, 9, d.hash.p, d.sk.p, nullptr, d.r.p, d.s.p, d.v.p, d.st.p, nullptr) == PLUME_ERR_ARG && d.untouched());
    }
    REQUIRE(plume_set_chunk(ctx, (size_t)1 << 20) == 0);
}

// every allocation of a host-form call fails in turn: an error code, nothing released, the call right when repeated, nothing leaked
static void group_failing_allocations() {
    plume_ctx* keeper = nullptr;                                                     // keeps the device's shared tables alive: the counted calls build none
    REQUIRE(plume_init(&keeper, 0) == 0);
    { g_what = "allocations: tables"; SignCall c(0, 8, false, false, 0); REQUIRE(c.run(keeper, nullptr) == 0); c.check(); }
    const Outstanding before;
    for (int selfcheck = 0; selfcheck < 2; selfcheck++) {
        plume_ctx* ctx = nullptr;
        REQUIRE(plume_init(&ctx, 0) == 0 && plume_set_sign_selfcheck(ctx, selfcheck) == 0);
        (void)mockhip::fail_allocation(-1);
        { g_what = "allocations: counting call"; SignCall c(0, g_n, true, true, 0); REQUIRE(c.run(ctx, nullptr) == 0); c.check(); }
        const long made = mockhip::fail_allocation(-1);
        REQUIRE(made >= 10 && made < 60);
        plume_destroy(ctx);
        for (long k = 0; k < made; k++) {
            g_what = "allocations: number " + std::to_string(k) + " fails, self-check " + std::to_string(selfcheck);
            REQUIRE(plume_init(&ctx, 0) == 0 && plume_set_sign_selfcheck(ctx, selfcheck) == 0);
            SignCall c(0, g_n, true, true, (int)(k & 1));
            (void)mockhip::fail_allocation(k);
            REQUIRE(c.run(ctx, nullptr) == PLUME_ERR_HIP);
            REQUIRE(c.untouched());
            (void)mockhip::fail_allocation(-1);
            REQUIRE(c.run(ctx, nullptr) == 0);                                       // the context is usable afterwards
            c.check();
            plume_destroy(ctx);
        }
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
    sign_group(ctx, "one device, host form, one chunk", 4, false, g_n);
    sign_group(ctx, "one device, host form, chunks of 7", 4, false, 7);
    sign_group(ctx, "one device, host form, chunks of 1", 2, false, 1);
    hash_group(ctx, "one device, host form, chunks of 5", false, 5);
    REQUIRE(plume_set_chunk(ctx, (size_t)1 << 20) == 0);
    hash_group(ctx, "one device, host form", false, 0);
    hash_group(ctx, "one device, device form", true, 0);
    sign_group(ctx, "one device, device form", 5, true, 0);
    for (int level : {0, 2, 1}) {
        REQUIRE(plume_set_sign_uniform(ctx, level) == 0);
        sign_group(ctx, ("uniform level " + std::to_string(level)).c_str(), 3, true, 0);
    }
    REQUIRE(plume_set_sub_batches(ctx, 3) == 0);
    sign_group(ctx, "one device, device form, three sub-batches", 3, true, 0);
    REQUIRE(plume_set_sub_batches(ctx, 1) == 0);
    {
        const std::vector<std::string> off = stages_of_a_device_call(ctx);
        REQUIRE((off == std::vector<std::string>{"ecdsa_sign_nonce", "ecdsa_sign_gmul", "to_affine", "ecdsa_sign_finalize"}));
        REQUIRE(plume_set_sign_selfcheck(ctx, 1) == 0 && plume_get_sign_selfcheck(ctx) == 1);
        const std::vector<std::string> on = stages_of_a_device_call(ctx);
        REQUIRE((on == std::vector<std::string>{"ecdsa_sign_nonce", "ecdsa_sign_gmul", "to_affine", "ecdsa_sign_finalize", "ecdsa_prepare", "tables", "ecdsa_mul", "to_affine",
                                                "ecdsa_finalize", "ecdsa_sign_release"}));
        sign_group(ctx, "self-check, device form", 4, true, 0);
        sign_group(ctx, "self-check, host form, chunks of 9", 4, false, 9);
        REQUIRE(plume_set_chunk(ctx, (size_t)1 << 20) == 0 && plume_set_sub_batches(ctx, 2) == 0 && plume_set_sign_uniform(ctx, 2) == 0);
        sign_group(ctx, "self-check, level 2, two sub-batches", 2, true, 0);
        REQUIRE(plume_set_sub_batches(ctx, 1) == 0 && plume_set_sign_uniform(ctx, 1) == 0 && plume_set_sign_selfcheck(ctx, 0) == 0);
        REQUIRE(plume_set_chunk(ctx, (size_t)1 << 20) == 0);
    }
    for (int devices : {3, 8}) {
        plume_ctx* multi = nullptr;
        int ids[8] = {0, 1, 2, 3, 4, 5, 6, 7};
        REQUIRE(plume_init_multi(&multi, ids, devices) == 0 && plume_num_shards(multi) == devices);
        sign_group(multi, "several devices, host form", 3, false, 0);
        hash_group(multi, "several devices, host form", false, 0);
        REQUIRE(plume_set_sign_selfcheck(multi, 1) == 0);
        sign_group(multi, "several devices, host form, self-check, chunks of 5", 2, false, 5);
        plume_destroy(multi);
    }
    group_arguments(ctx);
    plume_destroy(ctx);
    group_failing_allocations();
    REQUIRE(mockhip::outstanding(0) == 0 && mockhip::outstanding(2) == 0 && mockhip::outstanding(3) == 0);
    std::printf("ecdsa_sign_driver seed %llu: ok\n", seed);
    return 0;
}
