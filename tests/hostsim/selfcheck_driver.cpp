// TEST INFRASTRUCTURE ONLY.  The signer's self-check on the library's host side (the gate in csrc/plume_capi.hip's sign_device + csrc/plume_selfcheck_capi.hip) on the mock
// HIP runtime, under the sanitizers (tests/test_selfcheck_hostsim.py).  Batches carry planted wrong public keys (a neighbour's: on the curve, not sk G) and items the signer
// rejects itself (r = 0).  What must come out is the C oracle's: its sign, then its verify_non_zk of what it signed -- an item with oracle status 0 and verdict != 1 is all
// zero with status 8, every other item is the oracle's bytes and status.  After every call no device allocation (the caller's own device arrays included) holds the c or
// the s of a withheld item: the staging was wiped and nothing unchecked was released.  Host-pointer form (64- and 33-byte records) on one device and on a plume_init_multi
// context over eight mock devices, pieces of 5-64 items, pageable and page-locked caller arrays, the device forms on a caller stream, with and without derived nonces, an
// allocation failure at every allocation of a call.
//   selfcheck_driver <seed>            the checks above
//   selfcheck_driver <seed> prefill    for a build whose release launcher writes nothing: after every device-form call the caller's arrays still hold their pre-fill
#include <array>
#include <set>

#define DRIVER_NAME "selfcheck_driver"
#include "driver_prelude.h"

extern "C" {
int oracle_sign_batch(int version, size_t n, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* sk, const uint8_t* r, const uint8_t* pk_in, uint8_t* pk,
                      uint8_t* nullifier, uint8_t* c, uint8_t* s, uint8_t* r_point, uint8_t* hashed_to_curve_r, uint8_t* h_out, uint8_t* status, int nthreads);
int oracle_verify_non_zk_batch(int version, size_t n, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* pk, const uint8_t* nullifier, const uint8_t* s,
                               const uint8_t* r_point, const uint8_t* hashed_to_curve_r, const uint8_t* digest_private, uint8_t* ok, int nthreads);
size_t oracle_sec1_compress(const uint8_t p[64], uint8_t out[33]);
}

static bool g_prefill_mode = false;
using Rec = std::array<uint8_t, 32>;

struct Batch {
    int version = 1;
    size_t n = 0;
    bool with_pk = true;
    std::vector<uint8_t> msgs, sk, r, pk;
    std::vector<uint64_t> off;
    std::vector<uint8_t> signed_[7];   // the oracle's sign: pk, nullifier, c, s, r_point, hashed_to_curve_r, status
    std::vector<uint8_t> want[7];      // ... gated by the oracle's verify_non_zk
    std::vector<uint8_t> want33[7];    // ... and with SEC1-compressed points
    std::vector<uint8_t> withheld;     // per item
    size_t n_withheld = 0;
};
static const size_t kW[7] = {64, 64, 32, 32, 64, 64, 1};
static const size_t kW33[7] = {33, 33, 32, 32, 33, 33, 1};

static void expect(Batch& b) {
    const size_t n = b.n;
    for (int k = 0; k < 7; k++) b.signed_[k].assign(kW[k] * n, 0);
    REQUIRE(oracle_sign_batch(b.version, n, b.msgs.data(), b.off.data(), b.sk.data(), b.r.data(), b.with_pk ? b.pk.data() : nullptr, b.signed_[0].data(), b.signed_[1].data(),
                              b.signed_[2].data(), b.signed_[3].data(), b.signed_[4].data(), b.signed_[5].data(), nullptr, b.signed_[6].data(), 1) == 0);
    std::vector<uint8_t> ok(n, 0);
    REQUIRE(oracle_verify_non_zk_batch(b.version, n, b.msgs.data(), b.off.data(), b.signed_[0].data(), b.signed_[1].data(), b.signed_[3].data(), b.signed_[4].data(),
                                       b.signed_[5].data(), b.signed_[2].data(), ok.data(), 1) == 0);
    b.withheld.assign(n, 0);
    b.n_withheld = 0;
    for (int k = 0; k < 7; k++) { b.want[k] = b.signed_[k]; b.want33[k].assign(kW33[k] * n, 0); }
    for (size_t i = 0; i < n; i++) {
        if (b.signed_[6][i] == 0 && ok[i] != 1) {
            b.withheld[i] = 1; b.n_withheld++;
            for (int k = 0; k < 6; k++) std::memset(&b.want[k][kW[k] * i], 0, kW[k]);
            b.want[6][i] = PLUME_STATUS_SELFCHECK_FAILED;
        }
        for (int k = 0; k < 7; k++) {
            if (kW33[k] != 33) { std::memcpy(&b.want33[k][kW33[k] * i], &b.want[k][kW[k] * i], kW[k]); continue; }
            (void)oracle_sec1_compress(&b.want[k][64 * i], &b.want33[k][33 * i]);      // the identity: 00, the other 32 bytes stay zero
        }
    }
}

static Batch make_batch(size_t n, bool with_pk) {
    Batch b;
    b.n = n;
    b.version = 1 + (int)(rng() & 1);
    b.with_pk = with_pk;
    b.off.push_back(0);
    for (size_t i = 0; i < n; i++) {
        const size_t len = rng() % 121;
        for (size_t k = 0; k < len; k++) b.msgs.push_back((uint8_t)rng());
        b.off.push_back(b.msgs.size());
    }
    b.msgs.resize(b.msgs.size() + 16, 0);
    b.sk.resize(32 * n);
    b.r.resize(32 * n);
    for (size_t i = 0; i < 32 * n; i++) { b.sk[i] = (uint8_t)rng(); b.r[i] = (uint8_t)rng(); }
    for (size_t i = 0; i < n; i++) { b.sk[32 * i] &= 0x7F; b.sk[32 * i + 31] |= 1; b.r[32 * i] &= 0x7F; b.r[32 * i + 31] |= 1; }
    if (with_pk) {
        std::vector<uint8_t> t[7];
        for (int k = 0; k < 7; k++) t[k].assign(kW[k] * n, 0);
        REQUIRE(oracle_sign_batch(1, n, b.msgs.data(), b.off.data(), b.sk.data(), b.sk.data(), nullptr, t[0].data(), t[1].data(), t[2].data(), t[3].data(), t[4].data(), t[5].data(),
                                  nullptr, t[6].data(), 1) == 0);
        b.pk = t[0];
        for (size_t i = 0; i < n; i++)                                          // planted: the neighbour's key, about one item in four, and both ends
            if (n > 1 && (i == 0 || i == n - 1 || rng() % 4 == 0)) std::memcpy(&b.pk[64 * i], &t[0][64 * ((i + 1) % n)], 64);
    }
    if (n > 2 && (rng() & 1)) std::memset(&b.r[32 * (rng() % n)], 0, 32);       // an item the signer rejects itself
    expect(b);
    return b;
}

// the c and the s of every withheld item, at 32-byte boundaries of every live device allocation
static void check_nothing_withheld_lingers(const Batch& b) {
    std::set<Rec> sec;
    for (size_t i = 0; i < b.n; i++) {
        if (!b.withheld[i]) continue;
        Rec r;
        std::memcpy(r.data(), &b.signed_[2][32 * i], 32); sec.insert(r);
        std::memcpy(r.data(), &b.signed_[3][32 * i], 32); sec.insert(r);
    }
    mockhip::State& s = mockhip::st();
    std::lock_guard<std::mutex> lk(s.m);
    for (const auto& kv : s.ranges) {
        if (kv.second.type != hipMemoryTypeDevice) continue;
        const uint8_t* p = (const uint8_t*)kv.first;
        for (size_t o = 0; o + 32 <= kv.second.bytes; o += 32) {
            Rec r;
            std::memcpy(r.data(), p + o, 32);
            REQUIRE(!sec.count(r));
        }
    }
}

static bool all_fill(const uint8_t* p, size_t bytes) { for (size_t i = 0; i < bytes; i++) if (p[i] != kFill) return false; return true; }

static void check_outputs(const Batch& b, uint8_t* const got[7], bool sec1, bool has_pk) {
    const size_t* W = sec1 ? kW33 : kW;
    for (int k = 0; k < 7; k++) {
        if (k == 0 && !has_pk) continue;
        if (g_prefill_mode) { REQUIRE(all_fill(got[k], W[k] * b.n)); continue; }
        REQUIRE(std::memcmp(got[k], (sec1 ? b.want33 : b.want)[k].data(), W[k] * b.n) == 0);
    }
}

static void host_call(plume_ctx* ctx, const Batch& b, bool pinned, bool sec1, bool has_pk) {
    const size_t* W = sec1 ? kW33 : kW;
    Arr m(b.msgs.size(), pinned), off(8 * b.off.size(), pinned), sk(32 * b.n, pinned), r(32 * b.n, pinned), pk(64 * b.n, pinned);
    std::memcpy(m.p, b.msgs.data(), m.bytes); std::memcpy(off.p, b.off.data(), off.bytes); std::memcpy(sk.p, b.sk.data(), sk.bytes); std::memcpy(r.p, b.r.data(), r.bytes);
    if (b.with_pk) std::memcpy(pk.p, b.pk.data(), pk.bytes);
    std::vector<Arr*> out;
    uint8_t* o[7];
    for (int k = 0; k < 7; k++) { out.push_back(new Arr(W[k] * b.n, pinned)); o[k] = out[k]->p; }
    auto fn = sec1 ? plume_sign_batch_sec1 : plume_sign_batch;
    REQUIRE(fn(ctx, b.version, b.n, m.p, (const uint64_t*)off.p, sk.p, r.p, b.with_pk ? pk.p : nullptr, has_pk ? o[0] : nullptr, o[1], o[2], o[3], o[4], o[5], o[6]) == 0);
    check_outputs(b, o, sec1, has_pk);
    check_nothing_withheld_lingers(b);
    for (Arr* a : out) delete a;
}

static void dev_alloc(void** p, const void* src, size_t bytes, int fill = -1) {
    REQUIRE(hipMalloc(p, bytes ? bytes : 1) == hipSuccess);
    if (src && bytes) REQUIRE(hipMemcpy(*p, src, bytes, hipMemcpyHostToDevice) == hipSuccess);
    if (fill >= 0 && bytes) { const std::vector<uint8_t> f(bytes, (uint8_t)fill); REQUIRE(hipMemcpy(*p, f.data(), bytes, hipMemcpyHostToDevice) == hipSuccess); }
}
static void device_call(plume_ctx* ctx, const Batch& b, hipStream_t st, bool sec1) {
    const size_t* W = sec1 ? kW33 : kW;
    uint8_t *msgs, *sk, *r, *pk, *out[7];
    uint64_t* off;
    dev_alloc((void**)&msgs, b.msgs.data(), b.msgs.size()); dev_alloc((void**)&off, b.off.data(), 8 * b.off.size()); dev_alloc((void**)&sk, b.sk.data(), 32 * b.n);
    dev_alloc((void**)&r, b.r.data(), 32 * b.n); dev_alloc((void**)&pk, b.with_pk ? b.pk.data() : nullptr, 64 * b.n);
    for (int k = 0; k < 7; k++) dev_alloc((void**)&out[k], nullptr, W[k] * b.n, kFill);
    auto fn = sec1 ? plume_sign_batch_sec1_device : plume_sign_batch_device;
    REQUIRE(fn(ctx, b.version, b.n, msgs, off, b.msgs.size(), sk, r, b.with_pk ? pk : nullptr, out[0], out[1], out[2], out[3], out[4], out[5], out[6], st) == 0);
    REQUIRE(hipStreamSynchronize(st) == hipSuccess);
    check_outputs(b, out, sec1, true);                 // (the mock's device memory is host memory)
    check_nothing_withheld_lingers(b);                 // the caller's own device arrays included
    for (void* q : {(void*)msgs, (void*)sk, (void*)r, (void*)pk, (void*)off}) (void)hipFree(q);
    for (auto* q : out) (void)hipFree(q);
}

// derived nonces with the check on: r never leaves the device, so the reference is the same call with the check off -- byte-identical where the status stays 0, zeros and
// status 8 on exactly the planted keys (every planted key breaks the signature whatever r is; the oracle agreed for explicit r above)
static void derived_call(plume_ctx* ctx, const Batch& b) {
    std::vector<uint8_t> a[7], c[7];
    for (int k = 0; k < 7; k++) { a[k].assign(kW[k] * b.n, kFill); c[k].assign(kW[k] * b.n, kFill); }
    auto call = [&](std::vector<uint8_t>* o) {
        return plume_sign_batch_rfc6979(ctx, b.version, b.n, b.msgs.data(), b.off.data(), b.sk.data(), nullptr, b.with_pk ? b.pk.data() : nullptr, o[0].data(), o[1].data(),
                                        o[2].data(), o[3].data(), o[4].data(), o[5].data(), o[6].data());
    };
    REQUIRE(plume_set_sign_selfcheck(ctx, 0) == 0);
    REQUIRE(call(a) == 0);
    REQUIRE(plume_set_sign_selfcheck(ctx, 1) == 0);
    REQUIRE(call(c) == 0);
    std::vector<uint8_t> ok(b.n, 0);
    REQUIRE(oracle_verify_non_zk_batch(b.version, b.n, b.msgs.data(), b.off.data(), a[0].data(), a[1].data(), a[3].data(), a[4].data(), a[5].data(), a[2].data(), ok.data(), 1) == 0);
    for (size_t i = 0; i < b.n; i++) {
        const bool withheld = a[6][i] == 0 && ok[i] != 1;
        REQUIRE(c[6][i] == (withheld ? PLUME_STATUS_SELFCHECK_FAILED : a[6][i]));
        for (int k = 0; k < 6; k++)
            for (size_t j = 0; j < kW[k]; j++) REQUIRE(c[k][kW[k] * i + j] == (withheld ? 0 : a[k][kW[k] * i + j]));
    }
}

static void group_calls(plume_ctx* ctx, const char* what, int calls, bool device_form) {
    hipStream_t st = nullptr;
    if (device_form) REQUIRE(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
    REQUIRE(plume_set_sign_selfcheck(ctx, 1) == 0);
    REQUIRE(plume_get_sign_selfcheck(ctx) == 1);
    for (int k = 0; k < calls; k++) {
        const size_t piece = 5 + rng() % 60, n = 1 + rng() % 200;
        if (!device_form) REQUIRE(plume_set_host_piece(ctx, piece) == 0);
        const bool pinned = rng() & 1, sec1 = rng() & 1, has_pk = rng() % 4 != 0;
        Batch b = make_batch(n, rng() % 4 != 0);
        g_what = std::string(what) + " call " + std::to_string(k) + ": n " + std::to_string(n) + ", piece " + std::to_string(piece) + (pinned ? ", page-locked" : ", pageable") +
                 ", v" + std::to_string(b.version) + (b.with_pk ? ", pk given" : "") + (sec1 ? ", SEC1" : "") + ", withheld " + std::to_string(b.n_withheld);
        if (device_form) device_call(ctx, b, st, sec1);
        else host_call(ctx, b, pinned, sec1, has_pk);
        if (!device_form && k % 3 == 0) derived_call(ctx, b);
    }
    if (st) REQUIRE(hipStreamDestroy(st) == hipSuccess);
}

// an allocation failure at every allocation a self-checking sign call makes on a fresh context: PLUME_ERR_HIP, nothing leaked, every output item either still its
// pre-fill or what the gate releases, no withheld value anywhere, and the context still signs
static void group_alloc_failures() {                    // (the caller keeps a context of device 0 alive: it holds the generator tables every context there shares)
    int failures = 0;
    for (long k = 0;; k++) {
        g_what = "allocation failure " + std::to_string(k);
        const long base = mockhip::outstanding(0);
        plume_ctx* ctx = nullptr;
        REQUIRE(plume_init(&ctx, 0) == 0);
        REQUIRE(plume_set_host_piece(ctx, 16) == 0);
        REQUIRE(plume_set_sign_selfcheck(ctx, 1) == 0);
        Batch b = make_batch(40, true);
        std::vector<uint8_t> o[7];
        for (int j = 0; j < 7; j++) o[j].assign(kW[j] * b.n, kFill);
        auto call = [&] {
            return plume_sign_batch(ctx, b.version, b.n, b.msgs.data(), b.off.data(), b.sk.data(), b.r.data(), b.pk.data(), o[0].data(), o[1].data(), o[2].data(), o[3].data(),
                                    o[4].data(), o[5].data(), o[6].data());
        };
        mockhip::fail_allocation(k);
        int rc = call();
        mockhip::fail_allocation(-1);
        const bool done = rc == 0;
        if (!done) {
            failures++;
            REQUIRE(rc == PLUME_ERR_HIP);
            for (size_t i = 0; i < b.n; i++)
                for (int j = 0; j < 7; j++)
                    REQUIRE(all_fill(&o[j][kW[j] * i], kW[j]) || std::memcmp(&o[j][kW[j] * i], &b.want[j][kW[j] * i], kW[j]) == 0);
            check_nothing_withheld_lingers(b);
            REQUIRE(call() == 0);
        }
        uint8_t* got[7];
        for (int j = 0; j < 7; j++) got[j] = o[j].data();
        check_outputs(b, got, false, true);
        check_nothing_withheld_lingers(b);
        plume_destroy(ctx);
        REQUIRE(mockhip::outstanding(0) == base);                 // nothing leaked
        if (done) break;
    }
    g_what = "allocation failures: " + std::to_string(failures);
    REQUIRE(failures >= 10);
}

static void group_switch(plume_ctx* ctx) {
    g_what = "the switch";
    REQUIRE(plume_get_sign_selfcheck(ctx) == 0);
    REQUIRE(plume_set_sign_selfcheck(ctx, 2) == PLUME_ERR_ARG);
    REQUIRE(plume_set_sign_selfcheck(ctx, -1) == PLUME_ERR_ARG);
    REQUIRE(plume_set_sign_selfcheck(nullptr, 1) == PLUME_ERR_ARG);
    REQUIRE(plume_get_sign_selfcheck(nullptr) == PLUME_ERR_ARG);
    REQUIRE(plume_get_sign_selfcheck(ctx) == 0);
    // off: a planted key is released as the signer writes it, status 0 (what the check exists for)
    Batch b = make_batch(12, true);
    std::vector<uint8_t> o[7];
    for (int j = 0; j < 7; j++) o[j].assign(kW[j] * b.n, kFill);
    REQUIRE(plume_sign_batch(ctx, b.version, b.n, b.msgs.data(), b.off.data(), b.sk.data(), b.r.data(), b.pk.data(), o[0].data(), o[1].data(), o[2].data(), o[3].data(), o[4].data(),
                             o[5].data(), o[6].data()) == 0);
    REQUIRE(b.n_withheld >= 2);
    for (int j = 0; j < 7; j++) REQUIRE(o[j] == b.signed_[j]);
}

int main(int argc, char** argv) {
    const unsigned long long seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
    g_prefill_mode = argc > 2 && std::string(argv[2]) == "prefill";
    rng.seed(seed);
    plume_ctx* ctx = nullptr;
    REQUIRE(plume_init(&ctx, 0) == 0);
    group_switch(ctx);
    if (g_prefill_mode) {                                // the caller's DEVICE arrays: a host-pointer call copies its slots out whatever is in them
        group_calls(ctx, "one device, device form, nothing released", 8, true);
        plume_destroy(ctx);
        std::printf("selfcheck_driver seed %llu: ok\n", seed);
        return 0;
    }
    group_calls(ctx, "one device, host form", 10, false);
    group_calls(ctx, "one device, device form", 6, true);
    plume_ctx* multi = nullptr;
    int ids[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    REQUIRE(plume_init_multi(&multi, ids, 8) == 0);
    group_calls(multi, "eight devices, host form", 6, false);
    plume_destroy(multi);
    group_alloc_failures();
    plume_destroy(ctx);
    std::printf("selfcheck_driver seed %llu: ok\n", seed);
    return 0;
}
