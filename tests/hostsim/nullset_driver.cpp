// TEST INFRASTRUCTURE ONLY.  Drives the persistent nullifier set's C ABI (csrc/plume_nullset_capi.hip, with csrc/plume_capi.hip for the context) compiled as plain C++
// against the mock runtime (mockhip/hip/hip_runtime.h), with the kernels as host loops (nullset_launch.cpp), and compares every answer with a std::set of the records.
// Built and run by tests/test_nullset_hostsim.py under AddressSanitizer + UBSan and under ThreadSanitizer, with the mock's random stream scheduler: whatever the set does
// not order (an operation on a second caller stream that does not wait for the previous one, a download before its kernel, a buffer freed under queued work) shows up as
// a wrong answer or a sanitizer report.
//   nullset_driver [seed]
#include <array>
#include <map>
#include <set>

#define DRIVER_NAME "nullset_driver"
#include "driver_prelude.h"

using Rec = std::array<uint8_t, 64>;

// one call's inputs and what the definition says about them
struct Call {
    size_t n = 0;
    std::vector<uint8_t> nul, live, fresh;
    std::vector<uint64_t> ids;
    uint64_t n_fresh = 0;
    bool with_live = false, with_ids = false;
};
static Rec rec_of(const Call& c, size_t i) { Rec r; std::memcpy(r.data(), &c.nul[64 * i], 64); return r; }

// records drawn from a pool (repeats across and within calls), the identity among them; a live mask and descending 64-bit ids on some calls
static Call make_call(size_t n, const std::vector<Rec>& pool) {
    Call c;
    c.n = n;
    c.nul.resize(64 * n);
    c.live.assign(n, 1);
    c.ids.resize(n);
    c.with_live = rng() % 2;
    c.with_ids = rng() % 2;
    const uint64_t base = (1ull << 40) + rng() % 1000;
    for (size_t i = 0; i < n; i++) {
        const Rec& r = pool[rng() % pool.size()];
        std::memcpy(&c.nul[64 * i], r.data(), 64);
        if (c.with_live) c.live[i] = rng() % 5 != 0;
        c.ids[i] = base + (n - i) * 3;                 // reversed: the LAST of several equal records wins
    }
    return c;
}
// the definition: fresh iff live, not in S, smallest id among the call's live items with that record; then S gets every live record
static void expect(Call& c, std::set<Rec>& S) {
    std::map<Rec, uint64_t> best;
    for (size_t i = 0; i < c.n; i++) {
        if (!c.live[i]) continue;
        const uint64_t id = c.with_ids ? c.ids[i] : i;
        auto it = best.find(rec_of(c, i));
        if (it == best.end() || id < it->second) best[rec_of(c, i)] = id;
    }
    c.fresh.assign(c.n, 0);
    c.n_fresh = 0;
    for (size_t i = 0; i < c.n; i++) {
        if (!c.live[i]) continue;
        const Rec r = rec_of(c, i);
        if (!S.count(r) && best[r] == (c.with_ids ? c.ids[i] : i)) { c.fresh[i] = 1; c.n_fresh++; }
    }
    for (auto& kv : best) S.insert(kv.first);
}
static std::vector<Rec> make_pool(size_t k) {
    std::vector<Rec> pool(k);
    for (size_t j = 0; j < k; j++) for (auto& b : pool[j]) b = (uint8_t)rng();
    pool[0].fill(0);                                   // the identity is an ordinary record
    if (k > 2) { pool[2] = pool[1]; pool[2][63] ^= 1; } // differs in the last byte only
    return pool;
}

static void check_members(void* set, const std::set<Rec>& S, const std::vector<Rec>& pool) {
    std::vector<uint8_t> q(64 * pool.size()), found(pool.size(), 0xEE);
    for (size_t j = 0; j < pool.size(); j++) std::memcpy(&q[64 * j], pool[j].data(), 64);
    REQUIRE(plume_nullset_contains(set, pool.size(), q.data(), found.data()) == 0);
    for (size_t j = 0; j < pool.size(); j++) REQUIRE(found[j] == (S.count(pool[j]) ? 1 : 0));
    uint64_t size = 0, cap = 0;
    REQUIRE(plume_nullset_size(set, &size, &cap) == 0);
    REQUIRE(size == S.size());
    REQUIRE(cap >= 64 && (cap & (cap - 1)) == 0 && 2 * size <= cap);
}

static void host_insert(void* set, Call& c, std::set<Rec>& S) {
    expect(c, S);
    std::vector<uint8_t> fresh(c.n, 0xEE);
    uint64_t nf = 12345;
    REQUIRE(plume_nullset_insert(set, c.n, c.nul.data(), c.with_live ? c.live.data() : nullptr, c.with_ids ? c.ids.data() : nullptr, fresh.data(), &nf) == 0);
    REQUIRE(fresh == c.fresh);
    REQUIRE(nf == c.n_fresh);
}

// device-resident buffers of one call
struct DevCall {
    uint8_t *nul = nullptr, *live = nullptr, *fresh = nullptr;
    uint64_t *ids = nullptr, *nf = nullptr;
    std::vector<uint8_t> fresh_h;
    uint64_t nf_h = 0;
    void upload(const Call& c, hipStream_t st) {
        REQUIRE(hipMalloc((void**)&nul, 64 * c.n + 1) == hipSuccess && hipMalloc((void**)&live, c.n + 1) == hipSuccess && hipMalloc((void**)&fresh, c.n + 1) == hipSuccess);
        REQUIRE(hipMalloc((void**)&ids, 8 * c.n + 8) == hipSuccess && hipMalloc((void**)&nf, 8) == hipSuccess);
        REQUIRE(hipMemcpyAsync(nul, c.nul.data(), 64 * c.n, hipMemcpyHostToDevice, st) == hipSuccess);
        REQUIRE(hipMemcpyAsync(live, c.live.data(), c.n, hipMemcpyHostToDevice, st) == hipSuccess);
        REQUIRE(hipMemcpyAsync(ids, c.ids.data(), 8 * c.n, hipMemcpyHostToDevice, st) == hipSuccess);
    }
    void download(const Call& c, hipStream_t st) {
        fresh_h.assign(c.n, 0xEE);
        REQUIRE(hipMemcpyAsync(fresh_h.data(), fresh, c.n, hipMemcpyDeviceToHost, st) == hipSuccess);
        REQUIRE(hipMemcpyAsync(&nf_h, nf, 8, hipMemcpyDeviceToHost, st) == hipSuccess);
    }
    void release() { for (void* p : {(void*)nul, (void*)live, (void*)fresh, (void*)ids, (void*)nf}) (void)hipFree(p); }
};

// host forms: sequences with growth from an empty table, contains after every step, export round trip, clear
static void group_host(plume_ctx* ctx) {
    g_what = "host forms";
    const std::vector<Rec> pool = make_pool(700);
    void* set = nullptr;
    REQUIRE(plume_nullset_create(ctx, 0, &set) == 0 && set);
    std::set<Rec> S;
    for (size_t n : {1, 65, 300, 0, 900, 2000, 5}) {
        Call c = make_call(n, pool);
        host_insert(set, c, S);
        check_members(set, S, pool);
    }
    // export: exact sizes only, then into a new set
    uint64_t cnt = 0;
    REQUIRE(plume_nullset_export(set, 0, nullptr, &cnt) == 0 && cnt == S.size());
    std::vector<uint8_t> recs(64 * cnt);
    REQUIRE(plume_nullset_export(set, cnt - 1, recs.data(), &cnt) == PLUME_ERR_ARG && cnt == S.size());
    REQUIRE(plume_nullset_export(set, cnt, recs.data(), &cnt) == 0 && cnt == S.size());
    std::set<Rec> got;
    for (uint64_t j = 0; j < cnt; j++) { Rec r; std::memcpy(r.data(), &recs[64 * j], 64); got.insert(r); }
    REQUIRE(got == S);
    void* copy = nullptr;
    REQUIRE(plume_nullset_create(ctx, 10, &copy) == 0);
    std::vector<uint8_t> fresh(cnt);
    uint64_t nf = 0;
    REQUIRE(plume_nullset_insert(copy, cnt, recs.data(), nullptr, nullptr, fresh.data(), &nf) == 0 && nf == cnt);
    check_members(copy, S, pool);
    plume_nullset_destroy(copy);
    // clear, then the set starts over with the same capacity
    uint64_t size = 0, cap0 = 0, cap1 = 0;
    REQUIRE(plume_nullset_size(set, &size, &cap0) == 0);
    REQUIRE(plume_nullset_clear(set) == 0);
    S.clear();
    check_members(set, S, pool);
    REQUIRE(plume_nullset_size(set, &size, &cap1) == 0 && cap1 == cap0 && size == 0);
    REQUIRE(plume_nullset_export(set, 0, nullptr, &cnt) == 0 && cnt == 0);
    Call c = make_call(400, pool);
    host_insert(set, c, S);
    check_members(set, S, pool);
    REQUIRE(plume_nullset_reserve(set, 5000) == 0);
    REQUIRE(plume_nullset_size(set, &size, &cap1) == 0 && cap1 == 16384 && size == S.size());
    check_members(set, S, pool);
    plume_nullset_destroy(set);
}

// device forms on the set's own stream and on two caller streams in turn, nothing synchronised in between; then a destroy with work still queued
static void group_device(plume_ctx* ctx) {
    g_what = "device forms";
    const std::vector<Rec> pool = make_pool(500);
    void* set = nullptr;
    REQUIRE(plume_nullset_create(ctx, 0, &set) == 0);
    hipStream_t a = nullptr, b = nullptr;
    REQUIRE(hipStreamCreateWithFlags(&a, hipStreamNonBlocking) == hipSuccess && hipStreamCreateWithFlags(&b, hipStreamNonBlocking) == hipSuccess);
    std::set<Rec> S;
    std::vector<Call> calls;
    std::vector<DevCall> dev(8);
    for (int k = 0; k < 8; k++) calls.push_back(make_call(k == 3 ? 0 : 50 + 110 * k, pool));
    for (int k = 0; k < 8; k++) {
        hipStream_t st = k % 3 == 0 ? nullptr : k % 3 == 1 ? a : b;
        hipStream_t io = st ? st : a;                  // (the set's own stream is not the caller's: stage through a, which then has to wait for the set)
        dev[k].upload(calls[k], io);
        if (!st) REQUIRE(hipStreamSynchronize(a) == hipSuccess);
        expect(calls[k], S);
        const Call& c = calls[k];
        REQUIRE(plume_nullset_insert_device(set, c.n, dev[k].nul, c.with_live ? dev[k].live : nullptr, c.with_ids ? dev[k].ids : nullptr, dev[k].fresh, dev[k].nf, st) == 0);
        if (st) dev[k].download(c, st);
    }
    REQUIRE(hipStreamSynchronize(a) == hipSuccess && hipStreamSynchronize(b) == hipSuccess);
    uint64_t size = 0;                                 // the calls on the set's own stream: their outputs are there once size() has waited for the set
    REQUIRE(plume_nullset_size(set, &size, nullptr) == 0 && size == S.size());
    for (int k = 0; k < 8; k++) if (k % 3 == 0) dev[k].download(calls[k], a);
    REQUIRE(hipStreamSynchronize(a) == hipSuccess);
    for (int k = 0; k < 8; k++) {
        REQUIRE(dev[k].fresh_h == calls[k].fresh);
        REQUIRE(dev[k].nf_h == calls[k].n_fresh);
    }
    // contains_device on a caller stream after a device insert on the other one
    Call c = make_call(300, pool);
    DevCall d;
    d.upload(c, a);
    expect(c, S);
    REQUIRE(plume_nullset_insert_device(set, c.n, d.nul, c.with_live ? d.live : nullptr, c.with_ids ? d.ids : nullptr, d.fresh, nullptr, a) == 0);
    uint8_t* found = nullptr;
    REQUIRE(hipMalloc((void**)&found, c.n) == hipSuccess);
    REQUIRE(plume_nullset_contains_device(set, c.n, d.nul, found, b) == 0);
    std::vector<uint8_t> fh(c.n, 0xEE);
    REQUIRE(hipMemcpyAsync(fh.data(), found, c.n, hipMemcpyDeviceToHost, b) == hipSuccess);
    REQUIRE(hipStreamSynchronize(b) == hipSuccess);
    for (size_t i = 0; i < c.n; i++) REQUIRE(fh[i] == (S.count(rec_of(c, i)) ? 1 : 0));
    check_members(set, S, pool);
    // destroy with work queued: inserts enqueued on a, nothing synchronised, then the set goes
    Call q = make_call(700, pool);
    DevCall dq;
    dq.upload(q, a);
    REQUIRE(plume_nullset_insert_device(set, q.n, dq.nul, nullptr, nullptr, dq.fresh, dq.nf, a) == 0);
    REQUIRE(plume_nullset_insert_device(set, q.n, dq.nul, nullptr, nullptr, dq.fresh, dq.nf, b) == 0);
    plume_nullset_destroy(set);
    REQUIRE(hipStreamSynchronize(a) == hipSuccess && hipStreamSynchronize(b) == hipSuccess);
    (void)hipFree(found);
    d.release(); dq.release();
    for (auto& x : dev) x.release();
    REQUIRE(hipStreamDestroy(a) == hipSuccess && hipStreamDestroy(b) == hipSuccess);
}

// a multi-device context: the set lands on the first shard's device; the set outlives its context
static void group_multi() {
    g_what = "multi-device context";
    const int ids[2] = {3, 5};
    plume_ctx* m = nullptr;
    REQUIRE(plume_init_multi(&m, ids, 2) == 0);
    const long s3 = mockhip::st().dev[3].streams.size(), s5 = mockhip::st().dev[5].streams.size();
    void* set = nullptr;
    REQUIRE(plume_nullset_create(m, 100, &set) == 0);
    REQUIRE((long)mockhip::st().dev[3].streams.size() == s3 + 1 && (long)mockhip::st().dev[5].streams.size() == s5);
    plume_destroy(m);                                  // the set stays usable
    const std::vector<Rec> pool = make_pool(300);
    std::set<Rec> S;
    for (size_t n : {200, 333}) { Call c = make_call(n, pool); host_insert(set, c, S); }
    check_members(set, S, pool);
    plume_nullset_destroy(set);
}

// every allocation of a growing insert fails in turn (each time on a set in the same state): PLUME_ERR_HIP, the set unchanged and usable, nothing leaked
static void group_faults(plume_ctx* ctx) {
    const std::vector<Rec> pool = make_pool(2000);
    const Call c0 = make_call(40, pool);
    Call c = make_call(1500, pool);                    // grows the table
    for (int form = 0; form < 2; form++) {
        int failures = 0;
        for (long k = 0;; k++) {
            g_what = "allocation failures: form " + std::to_string(form) + ", allocation " + std::to_string(k);
            void* set = nullptr;
            REQUIRE(plume_nullset_create(ctx, 0, &set) == 0);
            std::set<Rec> S;
            Call first = c0;
            host_insert(set, first, S);
            uint64_t size0 = 0, cap0 = 0;
            REQUIRE(plume_nullset_size(set, &size0, &cap0) == 0);
            DevCall d;
            if (form == 1) { d.upload(c, nullptr); REQUIRE(hipStreamSynchronize(nullptr) == hipSuccess); }
            const long dev_before = mockhip::outstanding(0);
            mockhip::fail_allocation(k);
            std::vector<uint8_t> fresh(c.n, 0xEE);
            uint64_t nf = 0;
            int rc;
            if (form == 0) rc = plume_nullset_insert(set, c.n, c.nul.data(), c.with_live ? c.live.data() : nullptr, c.with_ids ? c.ids.data() : nullptr, fresh.data(), &nf);
            else rc = plume_nullset_insert_device(set, c.n, d.nul, c.with_live ? d.live : nullptr, c.with_ids ? d.ids : nullptr, d.fresh, d.nf, nullptr);
            mockhip::fail_allocation(-1);
            const bool done = rc == 0;
            if (!done) {
                failures++;
                REQUIRE(rc == PLUME_ERR_HIP);
                REQUIRE(mockhip::outstanding(0) <= dev_before);
                uint64_t size = 0, cap = 0;
                REQUIRE(plume_nullset_size(set, &size, &cap) == 0 && size == size0 && cap == cap0);
                check_members(set, S, pool);
                if (form == 0) rc = plume_nullset_insert(set, c.n, c.nul.data(), c.with_live ? c.live.data() : nullptr, c.with_ids ? c.ids.data() : nullptr, fresh.data(), &nf);
                else rc = plume_nullset_insert_device(set, c.n, d.nul, c.with_live ? d.live : nullptr, c.with_ids ? d.ids : nullptr, d.fresh, d.nf, nullptr);
                REQUIRE(rc == 0);                      // still usable
            }
            if (form == 1) { REQUIRE(plume_nullset_size(set, nullptr, nullptr) == 0); d.download(c, nullptr); REQUIRE(hipStreamSynchronize(nullptr) == hipSuccess); fresh = d.fresh_h; nf = d.nf_h; }
            Call cc = c;
            expect(cc, S);
            REQUIRE(fresh == cc.fresh && nf == cc.n_fresh);
            check_members(set, S, pool);
            d.release();
            plume_nullset_destroy(set);
            if (done) break;
        }
        g_what = "allocation failures: form " + std::to_string(form) + ", " + std::to_string(failures) + " failures";
        REQUIRE(failures >= 3);                        // scratch, new tags, new records at least
    }
}

static void group_args(plume_ctx* ctx) {
    g_what = "argument errors";
    uint8_t rec[64] = {0}, out[1] = {0};
    uint64_t v = 0;
    void* set = nullptr;
    const long allocs = mockhip::outstanding(0);
    REQUIRE(plume_nullset_create(nullptr, 0, &set) == PLUME_ERR_ARG && set == nullptr);
    REQUIRE(plume_nullset_create(ctx, 0, nullptr) == PLUME_ERR_ARG);
    mockhip::fail_allocation(0);                       // "before anything is allocated": an allocation here would fail and report PLUME_ERR_HIP
    REQUIRE(plume_nullset_create(ctx, (size_t(1) << 31) + 1, &set) == PLUME_ERR_ARG && set == nullptr);
    mockhip::fail_allocation(-1);
    REQUIRE(mockhip::outstanding(0) == allocs);
    REQUIRE(plume_nullset_insert(nullptr, 1, rec, nullptr, nullptr, out, &v) == PLUME_ERR_ARG);
    REQUIRE(plume_nullset_contains(nullptr, 1, rec, out) == PLUME_ERR_ARG);
    REQUIRE(plume_nullset_size(nullptr, &v, &v) == PLUME_ERR_ARG);
    REQUIRE(plume_nullset_reserve(nullptr, 1) == PLUME_ERR_ARG);
    REQUIRE(plume_nullset_clear(nullptr) == PLUME_ERR_ARG);
    REQUIRE(plume_nullset_export(nullptr, 0, nullptr, &v) == PLUME_ERR_ARG);
    REQUIRE(plume_nullset_insert_device(nullptr, 1, rec, nullptr, nullptr, out, nullptr, nullptr) == PLUME_ERR_ARG);
    REQUIRE(plume_nullset_contains_device(nullptr, 1, rec, out, nullptr) == PLUME_ERR_ARG);
    plume_nullset_destroy(nullptr);
    REQUIRE(plume_nullset_create(ctx, 0, &set) == 0);
    const long with_set = mockhip::outstanding(0);
    mockhip::fail_allocation(0);
    REQUIRE(plume_nullset_insert(set, 1, nullptr, nullptr, nullptr, out, &v) == PLUME_ERR_ARG);
    REQUIRE(plume_nullset_insert(set, 1, rec, nullptr, nullptr, nullptr, &v) == PLUME_ERR_ARG);
    REQUIRE(plume_nullset_insert(set, (size_t(1) << 30) + 1, rec, nullptr, nullptr, out, &v) == PLUME_ERR_ARG);
    REQUIRE(plume_nullset_insert_device(set, (size_t(1) << 30) + 1, rec, nullptr, nullptr, out, nullptr, nullptr) == PLUME_ERR_ARG);
    REQUIRE(plume_nullset_contains(set, 1, nullptr, out) == PLUME_ERR_ARG);
    REQUIRE(plume_nullset_contains_device(set, (size_t(1) << 30) + 1, rec, out, nullptr) == PLUME_ERR_ARG);
    REQUIRE(plume_nullset_reserve(set, (size_t(1) << 31) + 1) == PLUME_ERR_ARG);
    REQUIRE(plume_nullset_export(set, 0, nullptr, nullptr) == PLUME_ERR_ARG);
    mockhip::fail_allocation(-1);
    REQUIRE(mockhip::outstanding(0) == with_set);
    uint64_t size = 1, cap = 0;
    REQUIRE(plume_nullset_size(set, &size, &cap) == 0 && size == 0 && cap == 64);
    REQUIRE(plume_nullset_insert(set, 0, nullptr, nullptr, nullptr, nullptr, &v) == 0 && v == 0);
    plume_nullset_destroy(set);
}

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
    rng.seed(seed * 0x9E3779B97F4A7C15ull + 777);
    std::printf("%s\n", plume_version());
    plume_ctx* ctx = nullptr;
    REQUIRE(plume_init(&ctx, 1) == 0);
    group_args(ctx);
    group_host(ctx);
    group_device(ctx);
    group_faults(ctx);
    plume_destroy(ctx);
    group_multi();
    g_what = "leak check";
    REQUIRE(mockhip::outstanding(0) == 0);
    REQUIRE(mockhip::outstanding(1) == 0);
    REQUIRE(mockhip::outstanding(2) == 0);
    REQUIRE(mockhip::outstanding(3) == 0);
    std::printf("nullset_driver seed %llu: ok\n", (unsigned long long)seed);
    return 0;
}
