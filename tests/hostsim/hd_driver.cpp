// TEST INFRASTRUCTURE ONLY.  plume_hd_master_batch*, plume_hd_derive_priv_batch* and plume_hd_derive_pub_batch* on the library's host side (csrc/plume_hd_capi.hip) on the mock HIP runtime, under the sanitizers (tests/test_hd_hostsim.py).
// usage: hd_driver VECTORS SEED.  VECTORS is written by the test from the Python restatement (tests/_hd.py): u32 n, u32 depth, u32 seed_len; n parent sk, n chain codes (32
// bytes each), n x depth u32 indices, n parent pk (64 bytes), n x depth u32 indices of the public form, n seeds; then what the calls give, each as its arrays in ABI
// order: private (sk, chain, pk, address, status), public (pk, chain, address, status), private with PLUME_HD_SHARED_PARENT (record 0), private with PLUME_HD_SHARED_PATH
// (row 0), public with both flags' single records, master (sk, chain, status).  Every call must reproduce those bytes: the host form with chunks that cut the batch into 1,
// 2 and many pieces and on sub-ranges, pageable and page-locked arrays, NULL optional outputs; the device form on a caller stream (which must not have run anything when
// the call returns, under the lazy scheduler); the uniform levels; sub-batches; the stage lists; plume_init_multi contexts over two and eight mock devices; argument
// errors; then every allocation of a call fails in turn -- an error code, a repeated call right, nothing leaked; and after every call no device allocation other than the
// caller's own holds a key or a chain code of the batch, going in or coming out.
#include <array>
#include <mutex>
#include <set>

#define DRIVER_NAME "hd_driver"
#include "driver_prelude.h"

static size_t g_n = 0, g_depth = 0, g_seed_len = 0;
static std::vector<uint8_t> g_sk, g_chain, g_path, g_pk, g_ppath, g_seeds;
struct Want { std::vector<uint8_t> sk, chain, pk, addr, st; };
static Want g_priv, g_pub, g_priv_par, g_priv_path, g_pub_both, g_master;

static void rd(FILE* f, std::vector<uint8_t>& v, size_t bytes) { v.resize(bytes + 1); REQUIRE(bytes == 0 || std::fread(v.data(), 1, bytes, f) == bytes); }
static void read_want(FILE* f, Want& w, bool priv) {
    if (priv) rd(f, w.sk, 32 * g_n);
    if (priv) { rd(f, w.chain, 32 * g_n); rd(f, w.pk, 64 * g_n); } else { rd(f, w.pk, 64 * g_n); rd(f, w.chain, 32 * g_n); }
    rd(f, w.addr, 20 * g_n); rd(f, w.st, g_n);
}
static void read_vectors(const char* path) {
    FILE* f = std::fopen(path, "rb");
    REQUIRE(f);
    uint32_t h[3];
    REQUIRE(std::fread(h, 4, 3, f) == 3 && h[0] >= 30 && h[1] >= 1 && h[1] <= 8);
    g_n = h[0]; g_depth = h[1]; g_seed_len = h[2];
    rd(f, g_sk, 32 * g_n); rd(f, g_chain, 32 * g_n); rd(f, g_path, 4 * g_depth * g_n); rd(f, g_pk, 64 * g_n); rd(f, g_ppath, 4 * g_depth * g_n); rd(f, g_seeds, g_seed_len * g_n);
    read_want(f, g_priv, true); read_want(f, g_pub, false); read_want(f, g_priv_par, true); read_want(f, g_priv_path, true); read_want(f, g_pub_both, false);
    rd(f, g_master.sk, 32 * g_n); rd(f, g_master.chain, 32 * g_n); rd(f, g_master.st, g_n);
    uint8_t extra;
    REQUIRE(std::fread(&extra, 1, 1, f) == 0);
    std::fclose(f);
}

// no device allocation but the caller's own (skip) holds a key or a chain code of the batch: the staging and the workspace are wiped behind every call
using Rec = std::array<uint8_t, 32>;
static std::set<Rec> g_secrets;
static void collect_secrets() {
    for (const std::vector<uint8_t>* v : {&g_sk, &g_chain, &g_priv.sk, &g_priv.chain, &g_pub.chain, &g_priv_par.sk, &g_priv_par.chain, &g_priv_path.sk, &g_priv_path.chain,
                                          &g_pub_both.chain, &g_master.sk, &g_master.chain})
        for (size_t i = 0; i < g_n; i++) {
            Rec r;
            std::memcpy(r.data(), &(*v)[32 * i], 32);
            if (!all_of(r.data(), 32, 0) && !all_of(r.data(), 32, 0xFF)) g_secrets.insert(r);
        }
}
static void check_no_secrets(const std::set<const void*>& skip = {}) {
    mockhip::State& s = mockhip::st();
    std::lock_guard<std::mutex> lk(s.m);
    for (const auto& kv : s.ranges) {
        if (kv.second.type != hipMemoryTypeDevice || skip.count(kv.first)) continue;
        const uint8_t* p = (const uint8_t*)kv.first;
        for (size_t o = 0; o + 32 <= kv.second.bytes; o += 4) {               // (the workspace's records are 4-byte aligned)
            Rec r;
            std::memcpy(r.data(), p + o, 32);
            REQUIRE(!g_secrets.count(r));
        }
    }
}

// items [lo, lo + n) of one of the recorded calls
struct Call {
    bool pub;
    int flags;
    size_t lo, n;
    int kind;
    unsigned present;                                     // bit 0 chain, 1 pk (private form), 2 address
    const Want& want;
    Arr parent, pchain, path, sk, chain, pk, addr, st;
    Call(bool pub_, int flags_, size_t lo_, size_t n_, int k, unsigned present_, const Want& w)
        : pub(pub_), flags(flags_), lo(lo_), n(n_), kind(k), present(present_), want(w),
          parent((pub_ ? 64 : 32) * ((flags_ & PLUME_HD_SHARED_PARENT) ? 1 : n_), k, pub_ ? &g_pk[64 * ((flags_ & PLUME_HD_SHARED_PARENT) ? 0 : lo_)] : &g_sk[32 * ((flags_ & PLUME_HD_SHARED_PARENT) ? 0 : lo_)]),
          pchain(32 * ((flags_ & PLUME_HD_SHARED_PARENT) ? 1 : n_), k, &g_chain[32 * ((flags_ & PLUME_HD_SHARED_PARENT) ? 0 : lo_)]),
          path(4 * g_depth * ((flags_ & PLUME_HD_SHARED_PATH) ? 1 : n_), k, &(pub_ ? g_ppath : g_path)[4 * g_depth * ((flags_ & PLUME_HD_SHARED_PATH) ? 0 : lo_)]),
          sk(32 * n_, k), chain(32 * n_, k), pk(64 * n_, k), addr(20 * n_, k), st(n_, k) {}
    int run(plume_ctx* ctx, hipStream_t stream) {
        uint8_t *c = (present & 1u) ? chain.p : nullptr, *k = (pub || (present & 2u)) ? pk.p : nullptr, *a = (present & 4u) ? addr.p : nullptr;
        const uint32_t* pt = (const uint32_t*)path.p;
        if (pub) {
            if (kind == 2) return plume_hd_derive_pub_batch_device(ctx, flags, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, n, parent.p, pchain.p, pt, g_depth, k, c, a, st.p, stream);
            return plume_hd_derive_pub_batch(ctx, flags, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, n, parent.p, pchain.p, pt, g_depth, k, c, a, st.p);
        }
        if (kind == 2) return plume_hd_derive_priv_batch_device(ctx, flags, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, n, parent.p, pchain.p, pt, g_depth, sk.p, c, k, a, st.p, stream);
        return plume_hd_derive_priv_batch(ctx, flags, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, n, parent.p, pchain.p, pt, g_depth, sk.p, c, k, a, st.p);
    }
    bool untouched() const {
        return all_of(sk.p, sk.bytes, kFill) && all_of(chain.p, chain.bytes, kFill) && all_of(pk.p, pk.bytes, kFill) && all_of(addr.p, addr.bytes, kFill) && all_of(st.p, st.bytes, kFill);
    }
    void check() {                                        // (the mock's device memory is host memory)
        REQUIRE(std::memcmp(st.p, &want.st[lo], n) == 0);
        if (!pub) REQUIRE(std::memcmp(sk.p, &want.sk[32 * lo], 32 * n) == 0); else REQUIRE(all_of(sk.p, sk.bytes, kFill));
        if (present & 1u) REQUIRE(std::memcmp(chain.p, &want.chain[32 * lo], 32 * n) == 0); else REQUIRE(all_of(chain.p, chain.bytes, kFill));
        if (pub || (present & 2u)) REQUIRE(std::memcmp(pk.p, &want.pk[64 * lo], 64 * n) == 0); else REQUIRE(all_of(pk.p, pk.bytes, kFill));
        if (present & 4u) REQUIRE(std::memcmp(addr.p, &want.addr[20 * lo], 20 * n) == 0); else REQUIRE(all_of(addr.p, addr.bytes, kFill));
        for (size_t i = 0; i < n; i++) {                  // a status means zero records
            if (!st.p[i]) continue;
            REQUIRE(pub || all_of(sk.p + 32 * i, 32, 0));
            REQUIRE(!(present & 1u) || all_of(chain.p + 32 * i, 32, 0));
            REQUIRE(!(pub || (present & 2u)) || all_of(pk.p + 64 * i, 64, 0));
            REQUIRE(!(present & 4u) || all_of(addr.p + 20 * i, 20, 0));
        }
    }
    std::set<const void*> own() const { return {parent.p, pchain.p, path.p, sk.p, chain.p, pk.p, addr.p, st.p}; }
};

static void derive_group(plume_ctx* ctx, const char* what, int calls, bool device_form, size_t chunk) {
    const bool lazy = std::getenv("PLUME_MOCK_SCHED") == nullptr;
    hipStream_t st = nullptr;
    if (device_form) REQUIRE(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
    if (chunk) REQUIRE(plume_set_chunk(ctx, chunk) == 0);
    for (int k = 0; k < calls; k++) {
        // the recorded calls in turn: private, public, shared parent, shared path, public with both shared; whole batch first, then sub-ranges
        const int which = k % 5;
        const bool pub = which == 1 || which == 4;
        const int flags = which == 2 ? PLUME_HD_SHARED_PARENT : which == 3 ? PLUME_HD_SHARED_PATH : which == 4 ? (PLUME_HD_SHARED_PARENT | PLUME_HD_SHARED_PATH) : 0;
        const Want& w = which == 0 ? g_priv : which == 1 ? g_pub : which == 2 ? g_priv_par : which == 3 ? g_priv_path : g_pub_both;
        // a sub-range of a call with a shared array still starts from record 0 of that array: only per-item arrays move
        const size_t n = k < 5 ? g_n : 1 + rng() % g_n, lo = flags ? 0 : rng() % (g_n - n + 1);
        const unsigned present = k < 5 ? 7u : (unsigned)(rng() % 8);
        g_what = std::string(what) + " call " + std::to_string(k) + ": n " + std::to_string(n) + " from " + std::to_string(lo) + ", flags " + std::to_string(flags) + (pub ? ", public" : "") +
                 ", present " + std::to_string(present) + ", chunk " + std::to_string(chunk);
        // (with SHARED_PATH alone the parents move with lo while the row stays: lo = 0 keeps the recorded answers valid)
        Call c(pub, flags, lo, n, device_form ? 2 : (int)(rng() & 1), present, w);
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

static void master_group(plume_ctx* ctx, const char* what, bool device_form, size_t chunk) {
    g_what = std::string(what) + ", chunk " + std::to_string(chunk);
    hipStream_t st = nullptr;
    if (device_form) REQUIRE(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
    if (chunk) REQUIRE(plume_set_chunk(ctx, chunk) == 0);
    const int kind = device_form ? 2 : 1;
    Arr seeds(g_seed_len * g_n, kind, g_seeds.data()), sk(32 * g_n, kind), chain(32 * g_n, kind), status(g_n, kind);
    if (device_form) REQUIRE(plume_hd_master_batch_device(ctx, g_n, seeds.p, g_seed_len, sk.p, chain.p, status.p, st) == 0 && hipStreamSynchronize(st) == hipSuccess);
    else REQUIRE(plume_hd_master_batch(ctx, g_n, seeds.p, g_seed_len, sk.p, chain.p, status.p) == 0);
    REQUIRE(std::memcmp(sk.p, g_master.sk.data(), 32 * g_n) == 0 && std::memcmp(chain.p, g_master.chain.data(), 32 * g_n) == 0 && std::memcmp(status.p, g_master.st.data(), g_n) == 0);
    check_no_secrets(device_form ? std::set<const void*>{seeds.p, sk.p, chain.p, status.p} : std::set<const void*>{});
    if (st) REQUIRE(hipStreamDestroy(st) == hipSuccess);
}

static std::vector<std::string> stages_of_a_device_call(plume_ctx* ctx, bool pub) {
    hipStream_t st = nullptr;
    REQUIRE(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
    REQUIRE(plume_set_stage_timing(ctx, 1) == 0);
    Call c(pub, 0, 0, g_n, 2, 7, pub ? g_pub : g_priv);
    REQUIRE(c.run(ctx, st) == 0 && hipStreamSynchronize(st) == hipSuccess);
    c.check();
    const std::vector<std::string> names = last_stage_names(ctx);
    REQUIRE(plume_set_stage_timing(ctx, 0) == 0);
    REQUIRE(hipStreamDestroy(st) == hipSuccess);
    return names;
}

static void group_arguments(plume_ctx* ctx) {
    g_what = "arguments";
    Call c(false, 0, 0, 4, 0, 7, g_priv);
    const uint32_t* pt = (const uint32_t*)c.path.p;
    for (size_t depth : {(size_t)0, (size_t)9, (size_t)1 << 33})
        REQUIRE(plume_hd_derive_priv_batch(ctx, 0, 0, 0, 4, c.parent.p, c.pchain.p, pt, depth, c.sk.p, c.chain.p, c.pk.p, c.addr.p, c.st.p) == PLUME_ERR_ARG);
    for (int flags : {4, 0x100, -1})
        REQUIRE(plume_hd_derive_priv_batch(ctx, flags, 0, 0, 4, c.parent.p, c.pchain.p, pt, g_depth, c.sk.p, c.chain.p, c.pk.p, c.addr.p, c.st.p) == PLUME_ERR_ARG);
    REQUIRE(plume_hd_derive_priv_batch(ctx, 0, 2, 0, 4, c.parent.p, c.pchain.p, pt, g_depth, c.sk.p, c.chain.p, c.pk.p, c.addr.p, c.st.p) == PLUME_ERR_ARG);
    REQUIRE(plume_hd_derive_priv_batch(ctx, 0, 0, 3, 4, c.parent.p, c.pchain.p, pt, g_depth, c.sk.p, c.chain.p, c.pk.p, c.addr.p, c.st.p) == PLUME_ERR_ARG);
    REQUIRE(plume_hd_derive_priv_batch(ctx, 0, 0, 0, 4, nullptr, c.pchain.p, pt, g_depth, c.sk.p, c.chain.p, c.pk.p, c.addr.p, c.st.p) == PLUME_ERR_ARG);
    REQUIRE(plume_hd_derive_priv_batch(ctx, 0, 0, 0, 4, c.parent.p, nullptr, pt, g_depth, c.sk.p, c.chain.p, c.pk.p, c.addr.p, c.st.p) == PLUME_ERR_ARG);
    REQUIRE(plume_hd_derive_priv_batch(ctx, 0, 0, 0, 4, c.parent.p, c.pchain.p, nullptr, g_depth, c.sk.p, c.chain.p, c.pk.p, c.addr.p, c.st.p) == PLUME_ERR_ARG);
    REQUIRE(plume_hd_derive_priv_batch(ctx, 0, 0, 0, 4, c.parent.p, c.pchain.p, pt, g_depth, nullptr, c.chain.p, c.pk.p, c.addr.p, c.st.p) == PLUME_ERR_ARG);
    REQUIRE(plume_hd_derive_priv_batch(ctx, 0, 0, 0, 4, c.parent.p, c.pchain.p, pt, g_depth, c.sk.p, c.chain.p, c.pk.p, c.addr.p, nullptr) == PLUME_ERR_ARG);
    REQUIRE(plume_hd_derive_pub_batch(ctx, 0, 0, 0, 4, c.pk.p, c.pchain.p, pt, g_depth, nullptr, c.chain.p, c.addr.p, c.st.p) == PLUME_ERR_ARG);
    REQUIRE(plume_hd_derive_priv_batch(nullptr, 0, 0, 0, 4, c.parent.p, c.pchain.p, pt, g_depth, c.sk.p, c.chain.p, c.pk.p, c.addr.p, c.st.p) == PLUME_ERR_ARG);
    for (size_t sl : {(size_t)0, (size_t)15, (size_t)65}) REQUIRE(plume_hd_master_batch(ctx, 4, g_seeds.data(), sl, c.sk.p, c.chain.p, c.st.p) == PLUME_ERR_ARG);
    REQUIRE(plume_hd_master_batch(ctx, 4, nullptr, 16, c.sk.p, c.chain.p, c.st.p) == PLUME_ERR_ARG);
    REQUIRE(c.untouched());
    REQUIRE(plume_hd_derive_priv_batch(ctx, 0, 0, 0, 0, nullptr, nullptr, nullptr, 1, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    REQUIRE(plume_hd_derive_pub_batch_device(ctx, 0, 0, 0, 0, nullptr, nullptr, nullptr, 1, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    REQUIRE(plume_hd_master_batch(ctx, 0, nullptr, 16, nullptr, nullptr, nullptr) == 0);
    REQUIRE(plume_set_chunk(ctx, 8) == 0);
    {
        Call d(false, 0, 0, 9, 2, 7, g_priv);                                        // the device form takes at most a chunk
        REQUIRE(d.run(ctx, nullptr) == PLUME_ERR_ARG && d.untouched());
    }
    REQUIRE(plume_set_chunk(ctx, (size_t)1 << 20) == 0);
}

// every allocation of a host-form call fails in turn: an error code, the call right when repeated, nothing leaked, and nothing secret left staged
static void group_failing_allocations() {
    plume_ctx* keeper = nullptr;                                                     // keeps the device's shared tables alive: the counted calls build none
    REQUIRE(plume_init(&keeper, 0) == 0);
    { g_what = "allocations: tables"; Call c(false, 0, 0, 8, 0, 7, g_priv); REQUIRE(c.run(keeper, nullptr) == 0); c.check(); }
    const Outstanding before;
    for (int which = 0; which < 2; which++) {
        const bool pub = which == 1;
        const int flags = pub ? 0 : PLUME_HD_SHARED_PARENT;
        const Want& w = pub ? g_pub : g_priv_par;
        plume_ctx* ctx = nullptr;
        REQUIRE(plume_init(&ctx, 0) == 0 && plume_set_chunk(ctx, 11) == 0);
        (void)mockhip::fail_allocation(-1);
        { g_what = "allocations: counting call"; Call c(pub, flags, 0, g_n, 0, 7, w); REQUIRE(c.run(ctx, nullptr) == 0); c.check(); }
        const long made = mockhip::fail_allocation(-1);
        REQUIRE(made >= 8 && made < 60);
        plume_destroy(ctx);
        for (long k = 0; k < made; k++) {
            g_what = "allocations: number " + std::to_string(k) + " fails, form " + std::to_string(which);
            REQUIRE(plume_init(&ctx, 0) == 0 && plume_set_chunk(ctx, 11) == 0);
            Call c(pub, flags, 0, g_n, (int)(k & 1), 7, w);
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
    plume_destroy(keeper);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    read_vectors(argv[1]);
    collect_secrets();
    const unsigned long long seed = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1;
    rng.seed(seed);
    plume_ctx* ctx = nullptr;
    REQUIRE(plume_init(&ctx, 0) == 0);
    derive_group(ctx, "one device, host form, one piece", 5, false, g_n);
    derive_group(ctx, "one device, host form, two pieces", 5, false, (g_n + 1) / 2);
    derive_group(ctx, "one device, host form, chunks of 7", 12, false, 7);
    derive_group(ctx, "one device, host form, chunks of 1", 5, false, 1);
    master_group(ctx, "master, host form, chunks of 5", false, 5);
    REQUIRE(plume_set_chunk(ctx, (size_t)1 << 20) == 0);
    master_group(ctx, "master, host form", false, 0);
    master_group(ctx, "master, device form", true, 0);
    derive_group(ctx, "one device, device form", 10, true, 0);
    for (int level : {0, 2, 1}) {
        REQUIRE(plume_set_sign_uniform(ctx, level) == 0);
        derive_group(ctx, ("uniform level " + std::to_string(level)).c_str(), 5, true, 0);
    }
    REQUIRE(plume_set_sub_batches(ctx, 3) == 0);
    derive_group(ctx, "one device, device form, three sub-batches", 7, true, 0);
    REQUIRE(plume_set_sub_batches(ctx, 1) == 0);
    {
        std::vector<std::string> want = {"hd_priv_load"};
        for (size_t j = 0; j < g_depth; j++) for (const char* s : {"hd_gmul", "to_affine", "hd_priv_step"}) want.push_back(s);
        for (const char* s : {"hd_gmul", "to_affine", "hd_finish"}) want.push_back(s);
        REQUIRE(stages_of_a_device_call(ctx, false) == want);
        want = {"hd_pub_load"};
        for (size_t j = 0; j < g_depth; j++) for (const char* s : {"hd_pub_step", "to_affine"}) want.push_back(s);
        want.push_back("hd_finish");
        REQUIRE(stages_of_a_device_call(ctx, true) == want);
    }
    for (int devices : {2, 8}) {
        plume_ctx* multi = nullptr;
        int ids[8] = {0, 1, 2, 3, 4, 5, 6, 7};
        REQUIRE(plume_init_multi(&multi, ids, devices) == 0 && plume_num_shards(multi) == devices);
        derive_group(multi, "several devices, host form", 10, false, 0);
        derive_group(multi, "several devices, host form, chunks of 3", 5, false, 3);
        master_group(multi, "several devices, master", false, 0);
        plume_destroy(multi);
    }
    group_arguments(ctx);
    plume_destroy(ctx);
    group_failing_allocations();
    REQUIRE(mockhip::outstanding(0) == 0 && mockhip::outstanding(2) == 0 && mockhip::outstanding(3) == 0);
    std::printf("hd_driver seed %llu: ok\n", seed);
    return 0;
}
