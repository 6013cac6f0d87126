// TEST INFRASTRUCTURE ONLY.  The derived-nonce signer's host side (csrc/plume_nonce_capi.hip + the hook in plume_capi.hip) on the mock HIP runtime, under the
// sanitizers (tests/test_nonce_hostsim.py).  Every call's outputs are compared with the C oracle's sign given the nonces of the lane body (csrc/plume_nonce.h, run
// here directly); after every call no device allocation may still hold a derived nonce, a staged secret key or a staged hedging input.  Host-pointer form on one
// device and on a plume_init_multi context over eight mock devices, pieces of 5-64 items, pageable and page-locked caller arrays (two lanes), the device form on a
// caller stream, an allocation failure at every allocation of a derived-nonce call, argument errors.
//   nonce_driver <seed>
#include <array>
#include <set>

#define DRIVER_NAME "nonce_driver"
#include "driver_prelude.h"
#include "plume_nonce.h"

extern "C" {
int oracle_sign_batch(int version, size_t n, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* sk, const uint8_t* r, const uint8_t* pk_in, uint8_t* pk,
                      uint8_t* nullifier, uint8_t* c, uint8_t* s, uint8_t* r_point, uint8_t* hashed_to_curve_r, uint8_t* h_out, uint8_t* status, int nthreads);
}

using Rec = std::array<uint8_t, 32>;

struct Batch {
    int version = 1;
    size_t n = 0;
    bool with_pk = false, with_aux = false;
    std::vector<uint8_t> msgs, sk, aux, pk;
    std::vector<uint64_t> off;
    std::vector<uint8_t> r;          // the lane body's nonces
    std::vector<uint8_t> want[7];    // the oracle's pk, nullifier, c, s, r_point, hashed_to_curve_r, status
};
static const size_t kW[7] = {64, 64, 32, 32, 64, 64, 1};

// the lane body's nonces, then the oracle's sign with them (pk_in: the oracle's own pk of a first pass)
static void expect(Batch& b) {
    const size_t n = b.n;
    std::vector<uint8_t> tmp[7];
    for (int k = 0; k < 7; k++) { b.want[k].assign(kW[k] * n, 0); tmp[k].assign(kW[k] * n, 0); }
    if (b.with_pk) {
        REQUIRE(oracle_sign_batch(1, n, b.msgs.data(), b.off.data(), b.sk.data(), b.sk.data(), nullptr, tmp[0].data(), tmp[1].data(), tmp[2].data(), tmp[3].data(), tmp[4].data(),
                                  tmp[5].data(), nullptr, tmp[6].data(), 1) == 0);
        b.pk = tmp[0];
    }
    b.r.assign(32 * n, 0);
    plume::NonceArgs a;
    a.version = b.version; a.n = (uint32_t)n; a.msgs = b.msgs.data(); a.msg_off = b.off.data(); a.msgs_bytes = b.msgs.size(); a.sk = b.sk.data();
    a.aux = b.with_aux ? b.aux.data() : nullptr; a.pk_in = b.with_pk ? b.pk.data() : nullptr; a.r = b.r.data();
    for (uint32_t i = 0; i < n; i++) REQUIRE(plume::sign_nonce(a, i) == 1);
    REQUIRE(oracle_sign_batch(b.version, n, b.msgs.data(), b.off.data(), b.sk.data(), b.r.data(), b.with_pk ? b.pk.data() : nullptr, b.want[0].data(), b.want[1].data(),
                              b.want[2].data(), b.want[3].data(), b.want[4].data(), b.want[5].data(), nullptr, b.want[6].data(), 1) == 0);
}

static Batch make_batch(size_t n) {
    Batch b;
    b.n = n;
    b.version = 1 + (int)(rng() & 1);
    b.with_pk = rng() & 1;
    b.with_aux = rng() & 1;
    b.off.push_back(0);
    for (size_t i = 0; i < n; i++) {
        const size_t len = rng() % 121;
        for (size_t k = 0; k < len; k++) b.msgs.push_back((uint8_t)rng());
        b.off.push_back(b.msgs.size());
    }
    b.msgs.resize(b.msgs.size() + 16, 0);
    b.sk.resize(32 * n);
    b.aux.resize(32 * n);
    for (size_t i = 0; i < 32 * n; i++) { b.sk[i] = (uint8_t)rng(); b.aux[i] = (uint8_t)rng(); }
    for (size_t i = 0; i < n; i++) { b.sk[32 * i] &= 0x7F; b.sk[32 * i + 31] |= 1; }
    expect(b);
    return b;
}

// No device allocation other than `skip` (the caller's own device arrays) holds a derived nonce, a secret key or a hedging input of the batch at a 32-byte
// boundary: the workspace nonce buffer and the staged copies were wiped
static void check_no_secrets(const Batch& b, const std::set<const void*>& skip = {}) {
    std::set<Rec> sec;
    for (size_t i = 0; i < b.n; i++) {
        Rec r;
        std::memcpy(r.data(), &b.r[32 * i], 32); sec.insert(r);
        std::memcpy(r.data(), &b.sk[32 * i], 32); sec.insert(r);
        if (b.with_aux) { std::memcpy(r.data(), &b.aux[32 * i], 32); sec.insert(r); }
    }
    mockhip::State& s = mockhip::st();
    std::lock_guard<std::mutex> lk(s.m);
    for (const auto& kv : s.ranges) {
        if (kv.second.type != hipMemoryTypeDevice || skip.count(kv.first)) continue;
        const uint8_t* p = (const uint8_t*)kv.first;
        for (size_t o = 0; o + 32 <= kv.second.bytes; o += 32) {
            Rec r;
            std::memcpy(r.data(), p + o, 32);
            REQUIRE(!sec.count(r));
        }
    }
}

static void host_call(plume_ctx* ctx, const Batch& b, bool pinned) {
    Arr m(b.msgs.size(), pinned), off(8 * b.off.size(), pinned), sk(32 * b.n, pinned), aux(32 * b.n, pinned), pk(64 * b.n, pinned);
    std::memcpy(m.p, b.msgs.data(), m.bytes); std::memcpy(off.p, b.off.data(), off.bytes); std::memcpy(sk.p, b.sk.data(), sk.bytes);
    std::memcpy(aux.p, b.aux.data(), aux.bytes);
    if (b.with_pk) std::memcpy(pk.p, b.pk.data(), pk.bytes);
    std::vector<Arr*> out;
    for (int k = 0; k < 7; k++) out.push_back(new Arr(kW[k] * b.n, pinned));
    REQUIRE(plume_sign_batch_rfc6979(ctx, b.version, b.n, m.p, (const uint64_t*)off.p, sk.p, b.with_aux ? aux.p : nullptr, b.with_pk ? pk.p : nullptr, out[0]->p, out[1]->p,
                                     out[2]->p, out[3]->p, out[4]->p, out[5]->p, out[6]->p) == 0);
    for (int k = 0; k < 7; k++) { REQUIRE(std::memcmp(out[k]->p, b.want[k].data(), b.want[k].size()) == 0); delete out[k]; }
    check_no_secrets(b);
}

struct DevCall {
    uint8_t *msgs = nullptr, *sk = nullptr, *aux = nullptr, *pk = nullptr, *out[7] = {};
    uint64_t* off = nullptr;
    std::set<const void*> mine() const { std::set<const void*> s{msgs, sk, aux, pk, off}; for (auto* o : out) s.insert(o); return s; }
    void release() { for (void* q : {(void*)msgs, (void*)sk, (void*)aux, (void*)pk, (void*)off}) (void)hipFree(q); for (auto* o : out) (void)hipFree(o); }
};
static void dev_alloc(void** p, const void* src, size_t bytes) {
    REQUIRE(hipMalloc(p, bytes ? bytes : 1) == hipSuccess);
    if (src && bytes) REQUIRE(hipMemcpy(*p, src, bytes, hipMemcpyHostToDevice) == hipSuccess);
}
static void device_call(plume_ctx* ctx, const Batch& b, hipStream_t st) {
    DevCall d;
    dev_alloc((void**)&d.msgs, b.msgs.data(), b.msgs.size()); dev_alloc((void**)&d.off, b.off.data(), 8 * b.off.size()); dev_alloc((void**)&d.sk, b.sk.data(), 32 * b.n);
    dev_alloc((void**)&d.aux, b.aux.data(), 32 * b.n); dev_alloc((void**)&d.pk, b.with_pk ? b.pk.data() : nullptr, 64 * b.n);
    for (int k = 0; k < 7; k++) dev_alloc((void**)&d.out[k], nullptr, kW[k] * b.n);
    REQUIRE(plume_sign_batch_rfc6979_device(ctx, b.version, b.n, d.msgs, d.off, b.msgs.size(), d.sk, b.with_aux ? d.aux : nullptr, b.with_pk ? d.pk : nullptr, d.out[0], d.out[1],
                                            d.out[2], d.out[3], d.out[4], d.out[5], d.out[6], st) == 0);
    REQUIRE(hipStreamSynchronize(st) == hipSuccess);
    for (int k = 0; k < 7; k++) {
        std::vector<uint8_t> h(kW[k] * b.n);
        REQUIRE(hipMemcpy(h.data(), d.out[k], h.size(), hipMemcpyDeviceToHost) == hipSuccess);
        REQUIRE(h == b.want[k]);
    }
    check_no_secrets(b, d.mine());
    d.release();
}

static void group_calls(plume_ctx* ctx, const char* what, int calls, bool device_form) {
    hipStream_t st = nullptr;
    if (device_form) REQUIRE(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
    for (int k = 0; k < calls; k++) {
        const size_t piece = 5 + rng() % 60, n = 1 + rng() % 200;
        if (!device_form) REQUIRE(plume_set_host_piece(ctx, piece) == 0);
        const bool pinned = rng() & 1;
        Batch b = make_batch(n);
        g_what = std::string(what) + " call " + std::to_string(k) + ": n " + std::to_string(n) + ", piece " + std::to_string(piece) + (pinned ? ", page-locked" : ", pageable") +
                 ", v" + std::to_string(b.version) + (b.with_pk ? ", pk given" : "") + (b.with_aux ? ", hedged" : "");
        if (device_form) device_call(ctx, b, st);
        else host_call(ctx, b, pinned);
    }
    if (st) REQUIRE(hipStreamDestroy(st) == hipSuccess);
}

// an allocation failure at every allocation a derived-nonce call makes on a fresh context: PLUME_ERR_HIP, nothing leaked, nothing secret left, and the context still signs
static void group_alloc_failures() {                    // (the caller keeps a context of device 0 alive: it holds the generator tables every context there shares)
    int failures = 0;
    for (long k = 0;; k++) {
        g_what = "allocation failure " + std::to_string(k);
        const long base = mockhip::outstanding(0);
        plume_ctx* ctx = nullptr;
        REQUIRE(plume_init(&ctx, 0) == 0);
        REQUIRE(plume_set_host_piece(ctx, 16) == 0);
        Batch b = make_batch(40);
        std::vector<uint8_t> o[7];
        for (int j = 0; j < 7; j++) o[j].assign(kW[j] * b.n, 0);
        mockhip::fail_allocation(k);
        int rc = plume_sign_batch_rfc6979(ctx, b.version, b.n, b.msgs.data(), b.off.data(), b.sk.data(), b.with_aux ? b.aux.data() : nullptr, b.with_pk ? b.pk.data() : nullptr,
                                          o[0].data(), o[1].data(), o[2].data(), o[3].data(), o[4].data(), o[5].data(), o[6].data());
        mockhip::fail_allocation(-1);
        const bool done = rc == 0;
        if (!done) {
            failures++;
            REQUIRE(rc == PLUME_ERR_HIP);
            check_no_secrets(b);
            rc = plume_sign_batch_rfc6979(ctx, b.version, b.n, b.msgs.data(), b.off.data(), b.sk.data(), b.with_aux ? b.aux.data() : nullptr, b.with_pk ? b.pk.data() : nullptr,
                                          o[0].data(), o[1].data(), o[2].data(), o[3].data(), o[4].data(), o[5].data(), o[6].data());
            REQUIRE(rc == 0);
        }
        for (int j = 0; j < 7; j++) REQUIRE(o[j] == b.want[j]);
        check_no_secrets(b);
        plume_destroy(ctx);
        REQUIRE(mockhip::outstanding(0) == base);                 // nothing leaked
        if (done) break;
    }
    g_what = "allocation failures: " + std::to_string(failures);
    REQUIRE(failures >= 10);
}

static void group_args(plume_ctx* ctx) {
    g_what = "argument errors";
    Batch b = make_batch(3);
    std::vector<uint8_t> o[7];
    for (int j = 0; j < 7; j++) o[j].assign(kW[j] * b.n, 0);
    auto call = [&](plume_ctx* c, int version, const uint8_t* sk, uint8_t* nul, uint8_t* st) {
        return plume_sign_batch_rfc6979(c, version, b.n, b.msgs.data(), b.off.data(), sk, nullptr, nullptr, o[0].data(), nul, o[2].data(), o[3].data(), o[4].data(), o[5].data(), st);
    };
    REQUIRE(call(nullptr, 1, b.sk.data(), o[1].data(), o[6].data()) == PLUME_ERR_ARG);
    REQUIRE(call(ctx, 3, b.sk.data(), o[1].data(), o[6].data()) == PLUME_ERR_ARG);
    REQUIRE(call(ctx, 1, nullptr, o[1].data(), o[6].data()) == PLUME_ERR_ARG);
    REQUIRE(call(ctx, 1, b.sk.data(), nullptr, o[6].data()) == PLUME_ERR_ARG);
    REQUIRE(call(ctx, 1, b.sk.data(), o[1].data(), nullptr) == PLUME_ERR_ARG);
    REQUIRE(plume_sign_batch_rfc6979_device(ctx, 1, b.n, b.msgs.data(), nullptr, 0, b.sk.data(), nullptr, nullptr, o[0].data(), o[1].data(), o[2].data(), o[3].data(), o[4].data(),
                                            o[5].data(), o[6].data(), nullptr) == PLUME_ERR_ARG);
    REQUIRE(plume_sign_batch_rfc6979(ctx, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    REQUIRE(plume_sign_batch_rfc6979_device(ctx, 2, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
}

int main(int argc, char** argv) {
    const unsigned long long seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
    rng.seed(seed);
    plume_ctx* ctx = nullptr;
    REQUIRE(plume_init(&ctx, 0) == 0);
    group_args(ctx);
    group_calls(ctx, "one device, host form", 10, false);
    group_calls(ctx, "one device, device form", 6, true);
    plume_ctx* multi = nullptr;
    int ids[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    REQUIRE(plume_init_multi(&multi, ids, 8) == 0);
    group_calls(multi, "eight devices, host form", 6, false);
    plume_destroy(multi);
    group_alloc_failures();
    plume_destroy(ctx);
    std::printf("nonce_driver seed %llu: ok\n", seed);
    return 0;
}
