// TEST INFRASTRUCTURE ONLY.  plume_pbkdf2_sha512_batch* on the library's host side (csrc/plume_kdf_capi.hip) on the mock HIP runtime, under the sanitizers (tests/test_kdf_hostsim.py).
// usage: kdf_driver VECTORS SEED.  VECTORS is written by the test from the Python restatement (tests/_kdf.py): u32 n, salt_len, iterations, dklen, n_long; u64 pw_bytes;
// n + 1 u64 offsets; the passwords; n salts; then what the calls give: per-item salts (flags 0), PLUME_KDF_BIP39 | PLUME_KDF_SHARED_SALT with record 0, PLUME_KDF_BIP39
// with a NULL salt, the first n_long items at 2048 iterations and 64 bytes (BIP39, shared record 0); then n + 1 offsets with unsound items planted and what the device form
// gives for them (out, status).  Every call must reproduce those bytes: the host form with chunks that cut the batch into 1, 2 and many pieces and on sub-ranges, pageable
// and page-locked arrays; the shared salt uploaded for every piece and never advanced; the NULL salt; the device form on a caller stream (which must not have run
// anything when the call returns, under the lazy scheduler); the stage lists with their slice counts; plume_init_multi contexts over two and eight mock devices; argument
// errors; decreasing offsets; then every allocation of a call fails in turn -- an error code, a repeated call right, nothing leaked; and after every call, failed ones
// included, no device allocation other than the caller's own holds eight bytes in a row of a password, a salt, a midstate, a U or T, or an output of the batch.
#include <mutex>
#include <set>
#include <unordered_set>

#define DRIVER_NAME "kdf_driver"
#include "driver_prelude.h"
#include "plume_kdf.h"

static size_t g_n = 0, g_salt_len = 0, g_iterations = 0, g_dklen = 0, g_long = 0, g_pw_bytes = 0;
static std::vector<uint64_t> g_off, g_off_bad;
static std::vector<uint8_t> g_pw, g_salt, g_bad_out, g_bad_st;
struct Variant { int flags; bool null_salt; uint32_t iterations; size_t dklen; std::vector<uint8_t> want; };
static Variant g_var[4] = {{0, false, 0, 0, {}}, {PLUME_KDF_BIP39 | PLUME_KDF_SHARED_SALT, false, 0, 0, {}}, {PLUME_KDF_BIP39, true, 0, 0, {}},
                           {PLUME_KDF_BIP39 | PLUME_KDF_SHARED_SALT, false, 2048, 64, {}}};

static void rd(FILE* f, std::vector<uint8_t>& v, size_t bytes) { v.resize(bytes + 1); REQUIRE(bytes == 0 || std::fread(v.data(), 1, bytes, f) == bytes); }
static void read_vectors(const char* path) {
    FILE* f = std::fopen(path, "rb");
    REQUIRE(f);
    uint32_t h[5];
    uint64_t pwb;
    REQUIRE(std::fread(h, 4, 5, f) == 5 && std::fread(&pwb, 8, 1, f) == 1 && h[0] >= 30 && h[1] >= 8 && h[1] <= 256 && h[2] >= 2 && h[3] >= 8 && h[3] <= 64 && h[4] >= 1 && h[4] <= h[0]);
    g_n = h[0]; g_salt_len = h[1]; g_iterations = h[2]; g_dklen = h[3]; g_long = h[4]; g_pw_bytes = (size_t)pwb;
    g_off.resize(g_n + 1); g_off_bad.resize(g_n + 1);
    REQUIRE(std::fread(g_off.data(), 8, g_n + 1, f) == g_n + 1 && g_off[g_n] == g_pw_bytes);
    rd(f, g_pw, g_pw_bytes); rd(f, g_salt, g_salt_len * g_n);
    for (int k = 0; k < 3; k++) { g_var[k].iterations = (uint32_t)g_iterations; g_var[k].dklen = g_dklen; rd(f, g_var[k].want, g_dklen * g_n); }
    rd(f, g_var[3].want, 64 * g_long);
    REQUIRE(std::fread(g_off_bad.data(), 8, g_n + 1, f) == g_n + 1);
    rd(f, g_bad_out, g_dklen * g_n); rd(f, g_bad_st, g_n);
    uint8_t extra;
    REQUIRE(std::fread(&extra, 1, 1, f) == 0);
    std::fclose(f);
}

// eight bytes in a row of anything secret, as a 64-bit word in memory order
static std::unordered_set<uint64_t> g_words;
static void add_word(uint64_t w) { if (w != 0 && w != 0xAAAAAAAAAAAAAAAAull && w != ~0ull) g_words.insert(w); }
static void add_windows(const uint8_t* p, size_t bytes) {
    for (size_t o = 0; o + 8 <= bytes; o++) { uint64_t w; std::memcpy(&w, p + o, 8); add_word(w); }
}
// the workspace words of every item of one variant, behind the key stage and behind the last slice, from the lane bodies themselves; checks the recorded output on the way
static void collect_variant(const Variant& v, size_t n) {
    using namespace plume;
    std::vector<uint64_t> ws(PLUME_KDFK_WS_WORDS * n);
    std::vector<uint8_t> out(v.dklen * n), st(n);
    KdfArgs a;
    std::memset(&a, 0, sizeof a);
    a.flags = v.flags; a.n = (uint32_t)n; a.salt_len = v.null_salt ? 0 : (uint32_t)g_salt_len; a.dklen = (uint32_t)v.dklen;
    a.pw = g_pw.data(); a.pw_off = g_off.data(); a.pw_bytes = g_pw_bytes; a.salt = v.null_salt ? nullptr : g_salt.data(); a.out = out.data(); a.status = st.data(); a.ws = ws.data();
    for (uint32_t i = 0; i < n; i++) kdf_key_item(a, i);
    for (uint64_t w : ws) add_word(w);
    a.iters = v.iterations - 1;
    for (uint32_t i = 0; i < n; i++) { kdf_iter_item(a, i); kdf_finish_item(a, i); }
    for (uint64_t w : ws) add_word(w);
    REQUIRE(std::memcmp(out.data(), v.want.data(), v.dklen * n) == 0 && all_of(st.data(), n, 0));
    add_windows(out.data(), out.size());
}
static void collect_secrets() {
    g_what = "the lane bodies against the recorded outputs";
    add_windows(g_pw.data(), g_pw_bytes);
    for (size_t i = 0; i < g_n; i++) add_windows(&g_salt[g_salt_len * i], g_salt_len);
    for (int k = 0; k < 3; k++) collect_variant(g_var[k], g_n);
    collect_variant(g_var[3], g_long);
    add_windows(g_bad_out.data(), g_dklen * g_n);
}
static void check_no_secrets(const std::set<const void*>& skip = {}) {
    mockhip::State& s = mockhip::st();
    std::lock_guard<std::mutex> lk(s.m);
    for (const auto& kv : s.ranges) {
        if (kv.second.type != hipMemoryTypeDevice || skip.count(kv.first)) continue;
        const uint8_t* p = (const uint8_t*)kv.first;
        for (size_t o = 0; o + 8 <= kv.second.bytes; o++) {
            uint64_t w;
            std::memcpy(&w, p + o, 8);
            REQUIRE(!g_words.count(w));
        }
    }
}

// items [lo, lo + n) of one of the recorded calls; bad: the planted offsets (device form)
struct Call {
    const Variant& v;
    size_t lo, n;
    int kind;
    bool bad;
    size_t salt_len;
    Arr pw, off, salt, out, st;
    Call(const Variant& v_, size_t lo_, size_t n_, int k, bool bad_ = false)
        : v(v_), lo(lo_), n(n_), kind(k), bad(bad_), salt_len(v_.null_salt ? 0 : g_salt_len),
          pw(g_pw_bytes, k, g_pw.data()), off(8 * (n_ + 1), k, &(bad_ ? g_off_bad : g_off)[lo_]),
          salt(salt_len * ((v_.flags & PLUME_KDF_SHARED_SALT) ? 1 : n_), k, &g_salt[(v_.flags & PLUME_KDF_SHARED_SALT) ? 0 : g_salt_len * lo_]),
          out(v_.dklen * n_, k), st(n_, k) {}
    int run(plume_ctx* ctx, hipStream_t stream) {
        const uint8_t* sp = salt_len ? salt.p : nullptr;
        if (kind == 2) return plume_pbkdf2_sha512_batch_device(ctx, v.flags, n, pw.p, (const uint64_t*)off.p, g_pw_bytes, sp, salt_len, v.iterations, v.dklen, out.p, st.p, stream);
        return plume_pbkdf2_sha512_batch(ctx, v.flags, n, pw.p, (const uint64_t*)off.p, sp, salt_len, v.iterations, v.dklen, out.p, st.p);
    }
    bool untouched() const { return out.untouched() && st.untouched(); }
    void check() {                                        // (the mock's device memory is host memory)
        if (bad) {
            REQUIRE(std::memcmp(out.p, &g_bad_out[v.dklen * lo], v.dklen * n) == 0 && std::memcmp(st.p, &g_bad_st[lo], n) == 0);
            for (size_t i = 0; i < n; i++) REQUIRE(!st.p[i] || (st.p[i] == PLUME_STATUS_KDF_BAD_INPUT && all_of(out.p + v.dklen * i, v.dklen, 0)));
            return;
        }
        REQUIRE(std::memcmp(out.p, &v.want[v.dklen * lo], v.dklen * n) == 0 && all_of(st.p, n, 0));
    }
    std::set<const void*> own() const { return {pw.p, off.p, salt.p, out.p, st.p}; }
};

static void group(plume_ctx* ctx, const char* what, int calls, bool device_form, size_t chunk) {
    const bool lazy = std::getenv("PLUME_MOCK_SCHED") == nullptr;
    hipStream_t st = nullptr;
    if (device_form) REQUIRE(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
    if (chunk) REQUIRE(plume_set_chunk(ctx, chunk) == 0);
    for (int k = 0; k < calls; k++) {
        // the recorded calls in turn: per-item salts, the shared salt, the NULL salt; the whole batch first, then sub-ranges (a shared salt stays record 0)
        const Variant& v = g_var[k % 3];
        const size_t n = k < 3 ? g_n : 1 + rng() % g_n, lo = rng() % (g_n - n + 1);
        const bool bad = device_form && k % 3 == 0 && k >= 3;                      // the device form meets unsound offsets among sound ones
        g_what = std::string(what) + " call " + std::to_string(k) + ": n " + std::to_string(n) + " from " + std::to_string(lo) + ", flags " + std::to_string(v.flags) +
                 (bad ? ", planted offsets" : "") + ", chunk " + std::to_string(chunk);
        Call c(v, lo, n, device_form ? 2 : (int)(rng() & 1), bad);
        REQUIRE(c.run(ctx, st) == 0);
        if (device_form) {
            if (lazy) REQUIRE(c.untouched());                                      // enqueued, not run: the device form does not synchronise
            REQUIRE(hipStreamSynchronize(st) == hipSuccess);
        }
        c.check();
        check_no_secrets(device_form ? c.own() : std::set<const void*>{});
    }
    if (st) REQUIRE(hipStreamDestroy(st) == hipSuccess);
}

// the stage list of a device-form call of `iterations` on three items; the 2048 run is the recorded one and is checked
static void stages(plume_ctx* ctx, uint32_t iterations, size_t slices) {
    g_what = "stages of " + std::to_string(iterations) + " iterations";
    hipStream_t st = nullptr;
    REQUIRE(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
    REQUIRE(plume_set_stage_timing(ctx, 1) == 0);
    Variant v = g_var[1];
    v.iterations = iterations;
    if (iterations == 2048) {
        Call c(g_var[3], 0, g_long, 2);
        REQUIRE(c.run(ctx, st) == 0 && hipStreamSynchronize(st) == hipSuccess);
        c.check();
        check_no_secrets(c.own());
    } else {
        Call c(v, 0, 3, 2);
        REQUIRE(c.run(ctx, st) == 0 && hipStreamSynchronize(st) == hipSuccess);
        REQUIRE(all_of(c.st.p, 3, 0) && !c.out.untouched());
        if (iterations == g_iterations) c.check();
    }
    std::vector<std::string> want = {"kdf_key"};
    for (size_t k = 0; k < slices; k++) want.push_back("kdf_iter");
    want.push_back("kdf_finish");
    REQUIRE(last_stage_names(ctx) == want);
    REQUIRE(plume_set_stage_timing(ctx, 0) == 0);
    REQUIRE(hipStreamDestroy(st) == hipSuccess);
}

static void group_arguments(plume_ctx* ctx) {
    g_what = "arguments";
    Call c(g_var[0], 0, 4, 0);
    const uint64_t* off = (const uint64_t*)c.off.p;
    const uint32_t it = 2;
    for (uint32_t bad_it : {0u, PLUME_KDF_MAX_ITERATIONS + 1u, 0xFFFFFFFFu})
        REQUIRE(plume_pbkdf2_sha512_batch(ctx, 0, 4, c.pw.p, off, c.salt.p, g_salt_len, bad_it, g_dklen, c.out.p, c.st.p) == PLUME_ERR_ARG);
    for (size_t dk : {(size_t)0, (size_t)65, (size_t)128, (size_t)1 << 33})
        REQUIRE(plume_pbkdf2_sha512_batch(ctx, 0, 4, c.pw.p, off, c.salt.p, g_salt_len, it, dk, c.out.p, c.st.p) == PLUME_ERR_ARG);
    for (size_t sl : {(size_t)257, (size_t)1 << 33})
        REQUIRE(plume_pbkdf2_sha512_batch(ctx, 0, 4, c.pw.p, off, c.salt.p, sl, it, g_dklen, c.out.p, c.st.p) == PLUME_ERR_ARG);
    for (int flags : {4, 0x100, -1})
        REQUIRE(plume_pbkdf2_sha512_batch(ctx, flags, 4, c.pw.p, off, c.salt.p, g_salt_len, it, g_dklen, c.out.p, c.st.p) == PLUME_ERR_ARG);
    REQUIRE(plume_pbkdf2_sha512_batch(ctx, 0, 4, nullptr, off, c.salt.p, g_salt_len, it, g_dklen, c.out.p, c.st.p) == PLUME_ERR_ARG);
    REQUIRE(plume_pbkdf2_sha512_batch(ctx, 0, 4, c.pw.p, nullptr, c.salt.p, g_salt_len, it, g_dklen, c.out.p, c.st.p) == PLUME_ERR_ARG);
    REQUIRE(plume_pbkdf2_sha512_batch(ctx, 0, 4, c.pw.p, off, nullptr, g_salt_len, it, g_dklen, c.out.p, c.st.p) == PLUME_ERR_ARG);
    REQUIRE(plume_pbkdf2_sha512_batch(ctx, 0, 4, c.pw.p, off, c.salt.p, g_salt_len, it, g_dklen, nullptr, c.st.p) == PLUME_ERR_ARG);
    REQUIRE(plume_pbkdf2_sha512_batch(ctx, 0, 4, c.pw.p, off, c.salt.p, g_salt_len, it, g_dklen, c.out.p, nullptr) == PLUME_ERR_ARG);
    REQUIRE(plume_pbkdf2_sha512_batch(nullptr, 0, 4, c.pw.p, off, c.salt.p, g_salt_len, it, g_dklen, c.out.p, c.st.p) == PLUME_ERR_ARG);
    {
        // decreasing offsets anywhere: the host form refuses the whole call before anything is staged or written, whatever the chunk
        for (size_t chunk : {(size_t)1 << 20, (size_t)5}) {
            REQUIRE(plume_set_chunk(ctx, chunk) == 0);
            Call d(g_var[0], 0, g_n, 0, true);
            REQUIRE(d.run(ctx, nullptr) == PLUME_ERR_ARG && d.untouched());
            check_no_secrets();
        }
        REQUIRE(plume_set_chunk(ctx, (size_t)1 << 20) == 0);
    }
    REQUIRE(c.untouched());
    REQUIRE(plume_pbkdf2_sha512_batch(ctx, 0, 0, nullptr, nullptr, nullptr, 0, 1, 1, nullptr, nullptr) == 0);
    REQUIRE(plume_pbkdf2_sha512_batch_device(ctx, 0, 0, nullptr, nullptr, 0, nullptr, 0, 1, 1, nullptr, nullptr, nullptr) == 0);
    {
        Call d(g_var[0], 0, 4, 2);                                                   // the device form: a null password buffer that the offsets give bytes, a chunk
        REQUIRE(plume_pbkdf2_sha512_batch_device(ctx, 0, 4, nullptr, (const uint64_t*)d.off.p, g_pw_bytes, d.salt.p, g_salt_len, it, g_dklen, d.out.p, d.st.p, nullptr) == PLUME_ERR_ARG);
        REQUIRE(plume_set_chunk(ctx, 3) == 0);
        REQUIRE(d.run(ctx, nullptr) == PLUME_ERR_ARG && d.untouched());
        REQUIRE(plume_set_chunk(ctx, (size_t)1 << 20) == 0);
    }
}

// every allocation of a host-form call fails in turn: an error code, the call right when repeated, nothing leaked, and nothing secret left staged
static void group_failing_allocations() {
    const Outstanding before;
    for (int which = 0; which < 3; which++) {
        plume_ctx* ctx = nullptr;
        REQUIRE(plume_init(&ctx, 0) == 0 && plume_set_chunk(ctx, 11) == 0);
        (void)mockhip::fail_allocation(-1);
        { g_what = "allocations: counting call"; Call c(g_var[which], 0, g_n, 0); REQUIRE(c.run(ctx, nullptr) == 0); c.check(); }
        const long made = mockhip::fail_allocation(-1);
        REQUIRE(made >= 5 && made < 40);
        plume_destroy(ctx);
        for (long k = 0; k < made; k++) {
            g_what = "allocations: number " + std::to_string(k) + " fails, variant " + std::to_string(which);
            REQUIRE(plume_init(&ctx, 0) == 0 && plume_set_chunk(ctx, 11) == 0);
            Call c(g_var[which], 0, g_n, (int)(k & 1));
            (void)mockhip::fail_allocation(k);
            REQUIRE(c.run(ctx, nullptr) == PLUME_ERR_HIP);
            check_no_secrets();                                                      // nothing secret stays staged behind a failed call
            (void)mockhip::fail_allocation(-1);
            REQUIRE(c.run(ctx, nullptr) == 0);                                       // the context is usable afterwards
            c.check();
            check_no_secrets();
            plume_destroy(ctx);
        }
    }
    REQUIRE(Outstanding() == before);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    read_vectors(argv[1]);
    collect_secrets();
    const unsigned long long seed = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1;
    rng.seed(seed);
    plume_ctx* ctx = nullptr;
    REQUIRE(plume_init(&ctx, 0) == 0);
    group(ctx, "one device, host form, one piece", 3, false, g_n);
    group(ctx, "one device, host form, two pieces", 3, false, (g_n + 1) / 2);
    group(ctx, "one device, host form, chunks of 7", 12, false, 7);
    group(ctx, "one device, host form, chunks of 1", 3, false, 1);
    REQUIRE(plume_set_chunk(ctx, (size_t)1 << 20) == 0);
    group(ctx, "one device, device form", 12, true, 0);
    stages(ctx, 1, 0); stages(ctx, 256, 1); stages(ctx, 257, 1); stages(ctx, 2048, 8);
    for (int devices : {2, 8}) {
        plume_ctx* multi = nullptr;
        int ids[8] = {0, 1, 2, 3, 4, 5, 6, 7};
        REQUIRE(plume_init_multi(&multi, ids, devices) == 0 && plume_num_shards(multi) == devices);
        group(multi, "several devices, host form", 9, false, 0);
        group(multi, "several devices, host form, chunks of 3", 6, false, 3);
        {
            g_what = "several devices: the device form needs a single-device context";
            Call d(g_var[0], 0, 4, 2);
            REQUIRE(d.run(multi, nullptr) == PLUME_ERR_ARG && d.untouched());
        }
        plume_destroy(multi);
    }
    group_arguments(ctx);
    plume_destroy(ctx);
    group_failing_allocations();
    REQUIRE(mockhip::outstanding(0) == 0 && mockhip::outstanding(2) == 0 && mockhip::outstanding(3) == 0);
    std::printf("kdf_driver seed %llu: ok\n", seed);
    return 0;
}
