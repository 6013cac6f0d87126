// TEST INFRASTRUCTURE ONLY.  plume_eth_tx_sign_batch* on the library's host side (csrc/plume_eth_tx_sign_capi.hip) on the mock
// HIP runtime, under the sanitizers (tests/test_eth_tx_sign_hostsim.py).
// usage: eth_tx_sign_driver VECTORS SEED.  VECTORS is written by the test from the Python restatement (tests/_eth_tx_sign.py): u32 n, n + 1 u64 offsets, the bytes, n sk, n
// aux (32 bytes each), then what the call gives without aux and with it -- out (bytes + 68 n), out_len (4 n), status (n), hash, r, s (32 n each), v (n), chain_id (8 n),
// tx_type (n), twice.  Every call must reproduce those bytes, the assembled `out` compared whole: the host form with chunks that cut the batch into 1, 2 and many pieces and
// on sub-ranges that start at a non-zero offset, pageable and page-locked arrays, optional records absent; the device form on a caller stream (which must not have run
// anything when the call returns, under the lazy scheduler); the self-check on with the stage list of the header; plume_init_multi contexts over two and eight mock devices;
// argument errors, offsets that decrease in a later piece or shard than the first among them (nothing staged, nothing written); then every allocation of a call fails in turn -- an error code, `out` untouched, a repeated call right, nothing leaked; and after every call, failed ones
// included, no device allocation holds a key or a hedging input of the batch.
#include <array>
#include <set>

#define DRIVER_NAME "eth_tx_sign_driver"
#include "driver_prelude.h"

constexpr size_t kGrow = PLUME_ETH_TX_SIGN_GROWTH;

struct Want { std::vector<uint8_t> out, out_len, st, hash, r, s, v, chain, type; };
static size_t g_n = 0;
static std::vector<uint64_t> g_off;
static std::vector<uint8_t> g_txs, g_sk, g_aux;
static Want g_want[2];

static void rd(FILE* f, std::vector<uint8_t>& v, size_t bytes) { v.resize(bytes); REQUIRE(bytes == 0 || std::fread(v.data(), 1, bytes, f) == bytes); }
static void read_vectors(const char* path) {
    FILE* f = std::fopen(path, "rb");
    REQUIRE(f);
    uint32_t n = 0;
    REQUIRE(std::fread(&n, 4, 1, f) == 1 && n >= 40);
    g_n = n;
    g_off.resize(g_n + 1);
    REQUIRE(std::fread(g_off.data(), 8, g_n + 1, f) == g_n + 1 && g_off[0] == 0);
    rd(f, g_txs, (size_t)g_off[g_n]); rd(f, g_sk, 32 * g_n); rd(f, g_aux, 32 * g_n);
    for (Want& w : g_want) {
        rd(f, w.out, (size_t)g_off[g_n] + kGrow * g_n); rd(f, w.out_len, 4 * g_n); rd(f, w.st, g_n); rd(f, w.hash, 32 * g_n); rd(f, w.r, 32 * g_n); rd(f, w.s, 32 * g_n);
        rd(f, w.v, g_n); rd(f, w.chain, 8 * g_n); rd(f, w.type, g_n);
    }
    std::fclose(f);
}
static size_t slot_at(size_t lo, size_t i) { return (size_t)(g_off[i] - g_off[lo]) + kGrow * (i - lo); }     // of item i in a call that starts at item lo

// no device allocation other than the caller's own holds a key or a hedging input of the batch at a 32-byte boundary: the staged copies were wiped
using Rec = std::array<uint8_t, 32>;
static void check_no_secrets(const std::set<const void*>& skip = {}) {
    std::set<Rec> sec;
    for (size_t i = 0; i < g_n; i++) {
        Rec r;
        std::memcpy(r.data(), &g_sk[32 * i], 32); if (!all_of(r.data(), 32, 0)) sec.insert(r);
        std::memcpy(r.data(), &g_aux[32 * i], 32); sec.insert(r);
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

// items [lo, lo + n) signed with or without aux; the offsets are the caller's absolute ones, so a sub-range starts at a non-zero offset
struct Call {
    size_t lo, n, nbytes, out_bytes;
    bool hedged, records;
    int kind;
    Arr txs, off, sk, aux, out, out_len, st, hash, r, s, v, chain, type;
    Call(size_t lo_, size_t n_, bool hedged_, bool records_, int k)
        : lo(lo_), n(n_), nbytes((size_t)(g_off[lo_ + n_] - g_off[lo_])), out_bytes(nbytes + kGrow * n_), hedged(hedged_), records(records_), kind(k),
          txs(k == 2 ? nbytes : g_txs.size(), k, k == 2 ? g_txs.data() + g_off[lo_] : g_txs.data()), off(8 * (n_ + 1), k, &g_off[lo_]), sk(32 * n_, k, &g_sk[32 * lo_]),
          aux(32 * n_, k, &g_aux[32 * lo_]), out(out_bytes, k), out_len(4 * n_, k), st(n_, k), hash(32 * n_, k), r(32 * n_, k), s(32 * n_, k), v(n_, k), chain(8 * n_, k), type(n_, k) {
        if (k == 2) { uint64_t* o = (uint64_t*)off.p; const uint64_t base = o[0]; for (size_t i = 0; i <= n_; i++) o[i] -= base; }      // (the device buffer holds this range alone)
    }
    int run(plume_ctx* ctx, hipStream_t stream) {
        const uint8_t* a = hedged ? aux.p : nullptr;
        uint8_t *ph = records ? hash.p : nullptr, *pr = records ? r.p : nullptr, *ps = records ? s.p : nullptr, *pv = records ? v.p : nullptr, *pt = records ? type.p : nullptr;
        uint64_t* pc = records ? (uint64_t*)chain.p : nullptr;
        if (kind == 2)
            return plume_eth_tx_sign_batch_device(ctx, 0, n, txs.p, (const uint64_t*)off.p, nbytes, sk.p, a, out.p, out_bytes, (uint32_t*)out_len.p, ph, pr, ps, pv, pc, pt, st.p, stream);
        return plume_eth_tx_sign_batch(ctx, 0, n, txs.p, (const uint64_t*)off.p, sk.p, a, out.p, (uint32_t*)out_len.p, ph, pr, ps, pv, pc, pt, st.p);
    }
    bool untouched() const { return all_of(out.p, out.bytes, kFill) && all_of(out_len.p, out_len.bytes, kFill) && all_of(st.p, st.bytes, kFill) && all_of(r.p, r.bytes, kFill); }
    void check() {                                        // (the mock's device memory is host memory)
        const Want& w = g_want[hedged ? 1 : 0];
        REQUIRE(std::memcmp(st.p, &w.st[lo], n) == 0 && std::memcmp(out_len.p, &w.out_len[4 * lo], 4 * n) == 0);
        std::vector<uint8_t> want(out_bytes);             // the whole of out: every slot of the range, rebased
        for (size_t i = lo; i < lo + n; i++) std::memcpy(&want[slot_at(lo, i)], &w.out[slot_at(0, i)], (size_t)(g_off[i + 1] - g_off[i]) + kGrow);
        REQUIRE(std::memcmp(out.p, want.data(), out_bytes) == 0);
        if (records) {
            REQUIRE(std::memcmp(hash.p, &w.hash[32 * lo], 32 * n) == 0 && std::memcmp(r.p, &w.r[32 * lo], 32 * n) == 0 && std::memcmp(s.p, &w.s[32 * lo], 32 * n) == 0);
            REQUIRE(std::memcmp(v.p, &w.v[lo], n) == 0 && std::memcmp(chain.p, &w.chain[8 * lo], 8 * n) == 0 && std::memcmp(type.p, &w.type[lo], n) == 0);
        } else {
            REQUIRE(all_of(hash.p, hash.bytes, kFill) && all_of(r.p, r.bytes, kFill) && all_of(chain.p, chain.bytes, kFill));
        }
        REQUIRE(std::memcmp(sk.p, &g_sk[32 * lo], 32 * n) == 0 && std::memcmp(aux.p, &g_aux[32 * lo], 32 * n) == 0);
        check_no_secrets(kind == 2 ? std::set<const void*>{sk.p, aux.p} : std::set<const void*>{});
    }
};

static void group(plume_ctx* ctx, const char* what, int calls, bool device_form, size_t chunk) {
    const bool lazy = std::getenv("PLUME_MOCK_SCHED") == nullptr;
    hipStream_t st = nullptr;
    if (device_form) REQUIRE(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
    if (chunk) REQUIRE(plume_set_chunk(ctx, chunk) == 0);
    for (int k = 0; k < calls; k++) {
        const size_t n = k < 2 ? g_n : 1 + rng() % g_n, lo = rng() % (g_n - n + 1);
        const bool hedged = (k & 1) != 0, records = k != 2;
        g_what = std::string(what) + " call " + std::to_string(k) + ": n " + std::to_string(n) + " from " + std::to_string(lo) + (hedged ? ", hedged" : "") + ", chunk " + std::to_string(chunk);
        Call c(lo, n, hedged, records, device_form ? 2 : (int)(rng() & 1));
        REQUIRE(c.run(ctx, st) == 0);
        if (device_form) {
            if (lazy) REQUIRE(c.untouched());                                      // enqueued, not run: the device form does not synchronise
            REQUIRE(hipStreamSynchronize(st) == hipSuccess);
        }
        c.check();
    }
    if (st) REQUIRE(hipStreamDestroy(st) == hipSuccess);
}

static std::vector<std::string> stages_of_a_device_call(plume_ctx* ctx) {
    hipStream_t st = nullptr;
    REQUIRE(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
    REQUIRE(plume_set_stage_timing(ctx, 1) == 0);
    Call c(0, g_n, false, true, 2);
    REQUIRE(c.run(ctx, st) == 0 && hipStreamSynchronize(st) == hipSuccess);
    c.check();
    const std::vector<std::string> names = last_stage_names(ctx);
    REQUIRE(plume_set_stage_timing(ctx, 0) == 0);
    REQUIRE(hipStreamDestroy(st) == hipSuccess);
    return names;
}

// Offsets that decrease in a LATER piece or shard than the first, which is sound on its own.  `out` is sized as the header says, from tx_off[n] - tx_off[0], in a pageable
// allocation that ends with its last byte: a piece or a shard that downloaded its share before the call noticed would write past it (or, where tx_off[lo] < tx_off[0], in
// front of it) -- a heap overflow under ASan.  The call must return PLUME_ERR_ARG before anything is staged or written.
static void group_late_decrease(plume_ctx* ctx, const char* what, size_t chunk) {
    g_what = std::string("late decrease, ") + what;
    REQUIRE(g_n >= 4 && g_off[3] > g_off[2] && g_off[2] > g_off[1] && g_off[1] > 10);
    const uint64_t later_piece[5] = {0, g_off[1], g_off[2], 5, 10};                 // items 0 and 1 are real transactions; the decrease lies behind them
    const uint64_t wraps[5] = {g_off[2], g_off[3], 0, g_off[1], g_off[2]};           // the second half is monotone on its own and starts below tx_off[0]
    if (chunk) REQUIRE(plume_set_chunk(ctx, chunk) == 0);
    for (const uint64_t* off : {later_piece, wraps}) {
        const size_t out_bytes = plume_eth_tx_sign_out_bytes(4, off[4] - off[0]);
        Arr out(out_bytes, 0), out_len(16, 0), st(4, 0), r(128, 0);
        REQUIRE(plume_eth_tx_sign_batch(ctx, 0, 4, g_txs.data(), off, g_sk.data(), g_aux.data(), out.p, (uint32_t*)out_len.p, nullptr, r.p, nullptr, nullptr, nullptr, nullptr, st.p) ==
                PLUME_ERR_ARG);
        REQUIRE(all_of(out.p, out.bytes, kFill) && all_of(out_len.p, 16, kFill) && all_of(st.p, 4, kFill) && all_of(r.p, 128, kFill));
        check_no_secrets();
    }
    REQUIRE(plume_set_chunk(ctx, (size_t)1 << 20) == 0);
}

static void group_arguments(plume_ctx* ctx) {
    g_what = "arguments";
    Call c(0, 4, false, true, 0);
    const uint64_t* off = (const uint64_t*)c.off.p;
    uint32_t* len = (uint32_t*)c.out_len.p;
    for (int flags : {1, 2, 0x100, -1}) REQUIRE(plume_eth_tx_sign_batch(ctx, flags, 4, c.txs.p, off, c.sk.p, nullptr, c.out.p, len, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, c.st.p) == PLUME_ERR_ARG);
    REQUIRE(plume_eth_tx_sign_batch(ctx, 0, 4, c.txs.p, nullptr, c.sk.p, nullptr, c.out.p, len, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, c.st.p) == PLUME_ERR_ARG);
    REQUIRE(plume_eth_tx_sign_batch(ctx, 0, 4, c.txs.p, off, nullptr, nullptr, c.out.p, len, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, c.st.p) == PLUME_ERR_ARG);
    REQUIRE(plume_eth_tx_sign_batch(ctx, 0, 4, c.txs.p, off, c.sk.p, nullptr, nullptr, len, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, c.st.p) == PLUME_ERR_ARG);
    REQUIRE(plume_eth_tx_sign_batch(ctx, 0, 4, c.txs.p, off, c.sk.p, nullptr, c.out.p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, c.st.p) == PLUME_ERR_ARG);
    REQUIRE(plume_eth_tx_sign_batch(ctx, 0, 4, c.txs.p, off, c.sk.p, nullptr, c.out.p, len, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PLUME_ERR_ARG);
    REQUIRE(plume_eth_tx_sign_batch(nullptr, 0, 4, c.txs.p, off, c.sk.p, nullptr, c.out.p, len, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, c.st.p) == PLUME_ERR_ARG);
    const uint64_t down[5] = {0, 40, 30, 60, 70};                                    // the host form refuses decreasing offsets
    REQUIRE(plume_eth_tx_sign_batch(ctx, 0, 4, c.txs.p, down, c.sk.p, nullptr, c.out.p, len, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, c.st.p) == PLUME_ERR_ARG);
    REQUIRE(c.untouched());
    check_no_secrets();
    REQUIRE(plume_eth_tx_sign_batch(ctx, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    REQUIRE(plume_eth_tx_sign_batch_device(ctx, 0, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    REQUIRE(plume_eth_tx_sign_out_bytes(3, 100) == 100 + 3 * kGrow);
    REQUIRE(plume_set_chunk(ctx, 8) == 0);
    {
        Call d(0, 9, false, true, 2);                                                // the device form takes at most a chunk
        REQUIRE(d.run(ctx, nullptr) == PLUME_ERR_ARG && d.untouched());
    }
    REQUIRE(plume_set_chunk(ctx, (size_t)1 << 20) == 0);
}

// every allocation of a host-form call fails in turn: an error code, out untouched, no staged key left behind, the call right when repeated, nothing leaked
static void group_failing_allocations() {
    plume_ctx* keeper = nullptr;                                                     // keeps the device's shared tables alive: the counted calls build none
    REQUIRE(plume_init(&keeper, 0) == 0);
    { g_what = "allocations: tables"; Call c(0, 8, false, true, 0); REQUIRE(c.run(keeper, nullptr) == 0); c.check(); }
    const Outstanding before;
    for (int selfcheck = 0; selfcheck < 2; selfcheck++) {
        plume_ctx* ctx = nullptr;
        REQUIRE(plume_init(&ctx, 0) == 0 && plume_set_sign_selfcheck(ctx, selfcheck) == 0 && plume_set_chunk(ctx, 33) == 0);
        (void)mockhip::fail_allocation(-1);
        { g_what = "allocations: counting call"; Call c(0, g_n, true, true, 0); REQUIRE(c.run(ctx, nullptr) == 0); c.check(); }
        const long made = mockhip::fail_allocation(-1);
        REQUIRE(made >= 10 && made < 90);
        plume_destroy(ctx);
        for (long k = 0; k < made; k++) {
            g_what = "allocations: number " + std::to_string(k) + " fails, self-check " + std::to_string(selfcheck);
            REQUIRE(plume_init(&ctx, 0) == 0 && plume_set_sign_selfcheck(ctx, selfcheck) == 0 && plume_set_chunk(ctx, 33) == 0);
            Call c(0, g_n, true, true, (int)(k & 1));
            (void)mockhip::fail_allocation(k);
            REQUIRE(c.run(ctx, nullptr) == PLUME_ERR_HIP);
            (void)mockhip::fail_allocation(-1);
            check_no_secrets();                                                      // the staged sk and aux are wiped on the failure path too
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
    group(ctx, "one device, host form, one piece", 4, false, g_n);
    group(ctx, "one device, host form, two pieces", 3, false, (g_n + 1) / 2);
    group(ctx, "one device, host form, chunks of 7", 4, false, 7);
    REQUIRE(plume_set_chunk(ctx, (size_t)1 << 20) == 0);
    group(ctx, "one device, device form", 5, true, 0);
    REQUIRE(plume_set_sub_batches(ctx, 3) == 0);
    group(ctx, "one device, device form, three sub-batches", 3, true, 0);
    REQUIRE(plume_set_sub_batches(ctx, 1) == 0);
    {
        const std::vector<std::string> off = stages_of_a_device_call(ctx);
        REQUIRE((off == std::vector<std::string>{"eth_tx_sign_frame", "ecdsa_sign_nonce", "ecdsa_sign_gmul", "to_affine", "ecdsa_sign_finalize", "eth_tx_sign_assemble"}));
        REQUIRE(plume_set_sign_selfcheck(ctx, 1) == 0);
        const std::vector<std::string> on = stages_of_a_device_call(ctx);
        REQUIRE((on == std::vector<std::string>{"eth_tx_sign_frame", "ecdsa_sign_nonce", "ecdsa_sign_gmul", "to_affine", "ecdsa_sign_finalize", "ecdsa_prepare", "tables", "ecdsa_mul",
                                                "to_affine", "ecdsa_finalize", "ecdsa_sign_release", "eth_tx_sign_assemble"}));
        group(ctx, "self-check, host form, chunks of 9", 3, false, 9);
        REQUIRE(plume_set_chunk(ctx, (size_t)1 << 20) == 0 && plume_set_sign_selfcheck(ctx, 0) == 0);
    }
    for (int devices : {2, 8}) {
        plume_ctx* multi = nullptr;
        int ids[8] = {0, 1, 2, 3, 4, 5, 6, 7};
        REQUIRE(plume_init_multi(&multi, ids, devices) == 0 && plume_num_shards(multi) == devices);
        group(multi, "several devices, host form", 3, false, 0);
        group(multi, "several devices, host form, chunks of 5", 2, false, 5);
        group_late_decrease(multi, "several devices", 0);
        group_late_decrease(multi, "several devices, chunks of 1", 1);
        plume_destroy(multi);
    }
    group_arguments(ctx);
    group_late_decrease(ctx, "one device, chunks of 2", 2);
    group_late_decrease(ctx, "one device, chunks of 1", 1);
    plume_destroy(ctx);
    group_failing_allocations();
    REQUIRE(mockhip::outstanding(0) == 0 && mockhip::outstanding(2) == 0 && mockhip::outstanding(3) == 0);
    std::printf("eth_tx_sign_driver seed %llu: ok\n", seed);
    return 0;
}
