// TEST INFRASTRUCTURE ONLY.  plume_eth_tx_parse_batch* and plume_eth_tx_sender_batch* on the library's host side (csrc/plume_eth_tx_capi.hip) on the mock HIP runtime, under the sanitizers (tests/test_eth_tx_hostsim.py).
// usage: eth_tx_driver VECTORS SEED.  VECTORS is written by the test from the Python restatement (tests/_eth_tx.py, tests/_ecdsa.py) over the committed fixture: u32 n,
// n + 1 u64 offsets, the bytes, then what the parse writes (hash, r, s 32 n each; v, tx_type, status n each; chain_id 8 n) and what the sender writes under
// PLUME_ECDSA_LOW_S in the 64-byte / raw formats (pk 64 n, address 20 n, status n).  Every call on a range of the items must reproduce those bytes: the host form with
// chunks of 1, 7 and n, pageable and page-locked arrays, optional outputs absent, the device form on a caller stream (which must not have run anything when the call
// returns, under the lazy scheduler), plume_init_multi contexts over three and eight mock devices, empty items of a null buffer on one device and on several, argument errors, the stage lists, and every allocation of a call
// failing in turn: an error code, untouched outputs, the outputs of a repeated call right, nothing leaked.  A context that only parses builds no table.
#define DRIVER_NAME "eth_tx_driver"
#include "driver_prelude.h"

static size_t g_n;
static std::vector<uint64_t> g_off;
static std::vector<uint8_t> g_txs, g_hash, g_r, g_s, g_v, g_type, g_status, g_chain, g_pk, g_addr, g_sstatus;

static void read_vectors(const char* path) {
    FILE* f = std::fopen(path, "rb");
    REQUIRE(f);
    uint32_t n = 0;
    REQUIRE(std::fread(&n, 4, 1, f) == 1 && n >= 100);
    g_n = n;
    g_off.resize(g_n + 1);
    REQUIRE(std::fread(g_off.data(), 8, g_n + 1, f) == g_n + 1);
    auto rd = [&](std::vector<uint8_t>& v, size_t bytes) { v.resize(bytes); REQUIRE(std::fread(v.data(), 1, bytes, f) == bytes); };
    rd(g_txs, (size_t)g_off[g_n]); rd(g_hash, 32 * g_n); rd(g_r, 32 * g_n); rd(g_s, 32 * g_n); rd(g_v, g_n); rd(g_type, g_n); rd(g_status, g_n); rd(g_chain, 8 * g_n);
    rd(g_pk, 64 * g_n); rd(g_addr, 20 * g_n); rd(g_sstatus, g_n);
    std::fclose(f);
}

// an output given to the call holds items [lo, lo + n) of ref; one not given is untouched
static void want(const Arr& a, bool given, const std::vector<uint8_t>& ref, size_t width, size_t lo, size_t n) {
    if (given) REQUIRE(std::memcmp(a.p, ref.data() + width * lo, width * n) == 0); else REQUIRE(a.untouched());
}

// items [lo, lo + n).  The host forms get the whole offsets array from `lo` on (absolute offsets into the whole buffer); the device forms a buffer and offsets of their own
struct Call {
    bool sender;
    int kind, outs;                                       // outs: parse bit 0 chain_id, 1 tx_type, 2 status; sender bit 0 pk, 1 address, 2 status, 3 chain_id + tx_type, 4 expect
    size_t lo, n, bytes;
    std::vector<uint64_t> rel;
    Arr txs, off, hash, r, s, v, chain, type, status, pk, addr, expect;
    Call(bool sender_, size_t lo_, size_t n_, int outs_, int k)
        : sender(sender_), kind(k), outs(outs_), lo(lo_), n(n_), bytes((size_t)(g_off[lo_ + n_] - g_off[lo_])), txs(bytes, k, g_txs.data() + g_off[lo_]), off(8 * (n_ + 1), k),
          hash(32 * n_, k), r(32 * n_, k), s(32 * n_, k), v(n_, k), chain(8 * n_, k), type(n_, k), status(n_, k), pk(64 * n_, k), addr(20 * n_, k),
          expect(20 * n_, k, g_addr.data() + 20 * lo_) {
        rel.resize(n + 1);
        for (size_t i = 0; i <= n; i++) rel[i] = g_off[lo + i] - g_off[lo];
        std::memcpy(off.p, rel.data(), 8 * (n + 1));
    }
    int run(plume_ctx* ctx, hipStream_t st, int flags = PLUME_ECDSA_LOW_S) {
        uint64_t* c = (uint64_t*)chain.p;
        if (!sender) {
            uint64_t* cc = (outs & 1) ? c : nullptr;
            uint8_t *ty = (outs & 2) ? type.p : nullptr, *stt = (outs & 4) ? status.p : nullptr;
            if (kind == 2) return plume_eth_tx_parse_batch_device(ctx, n, txs.p, (const uint64_t*)off.p, bytes, hash.p, r.p, s.p, v.p, cc, ty, stt, st);
            return plume_eth_tx_parse_batch(ctx, n, g_txs.data(), g_off.data() + lo, hash.p, r.p, s.p, v.p, cc, ty, stt);
        }
        uint8_t *pp = (outs & 1) ? pk.p : nullptr, *aa = (outs & 2) ? addr.p : nullptr, *stt = (outs & 4) ? status.p : nullptr, *ty = (outs & 8) ? type.p : nullptr;
        uint64_t* cc = (outs & 8) ? c : nullptr;
        const uint8_t* ee = (outs & 16) ? expect.p : nullptr;
        if (kind == 2) return plume_eth_tx_sender_batch_device(ctx, flags, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, n, txs.p, (const uint64_t*)off.p, bytes, ee, pp, aa, cc, ty, stt, st);
        return plume_eth_tx_sender_batch(ctx, flags, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, n, g_txs.data(), g_off.data() + lo, ee, pp, aa, cc, ty, stt);
    }
    bool untouched() const {
        return hash.untouched() && r.untouched() && s.untouched() && v.untouched() && chain.untouched() && type.untouched() && status.untouched() && pk.untouched() && addr.untouched();
    }
    void check() const {                                  // (the mock's device memory is host memory)
        if (!sender) {
            want(hash, true, g_hash, 32, lo, n); want(r, true, g_r, 32, lo, n); want(s, true, g_s, 32, lo, n); want(v, true, g_v, 1, lo, n);
            want(chain, outs & 1, g_chain, 8, lo, n); want(type, outs & 2, g_type, 1, lo, n); want(status, outs & 4, g_status, 1, lo, n);
            REQUIRE(pk.untouched() && addr.untouched());
        } else {
            want(pk, outs & 1, g_pk, 64, lo, n); want(addr, outs & 2, g_addr, 20, lo, n); want(status, outs & 4, g_sstatus, 1, lo, n);
            want(chain, outs & 8, g_chain, 8, lo, n); want(type, outs & 8, g_type, 1, lo, n);
            REQUIRE(hash.untouched() && r.untouched() && s.untouched() && v.untouched());
        }
        REQUIRE(std::memcmp(txs.p, g_txs.data() + g_off[lo], bytes) == 0 && std::memcmp(off.p, rel.data(), 8 * (n + 1)) == 0 &&
                std::memcmp(expect.p, g_addr.data() + 20 * lo, 20 * n) == 0);
    }
};

static void group(plume_ctx* ctx, const char* what, int calls, bool device_form, size_t chunk, size_t sender_max) {
    const bool lazy = std::getenv("PLUME_MOCK_SCHED") == nullptr;
    hipStream_t st = nullptr;
    if (device_form) REQUIRE(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
    if (chunk) REQUIRE(plume_set_chunk(ctx, chunk) == 0);
    for (int k = 0; k < calls; k++) {
        const bool sender = (k & 1) != 0;
        const size_t cap = sender ? sender_max : g_n;
        const size_t n = k < 2 ? cap : 1 + rng() % cap, lo = rng() % (g_n - n + 1);
        int outs = k < 2 ? (sender ? 31 : 7) : (int)(rng() % (sender ? 32 : 8));
        if (sender && !(outs & 7)) outs |= 4;                                          // at least one of pk, address, status
        g_what = std::string(what) + " call " + std::to_string(k) + (sender ? ": sender" : ": parse") + ", n " + std::to_string(n) + " from " + std::to_string(lo) + ", outputs " +
                 std::to_string(outs) + ", chunk " + std::to_string(chunk);
        Call c(sender, lo, n, outs, device_form ? 2 : (int)(rng() & 1));
        REQUIRE(c.run(ctx, st) == 0);
        if (device_form) {
            if (lazy) REQUIRE(c.untouched());                                          // enqueued, not run: the device forms do not synchronise
            REQUIRE(hipStreamSynchronize(st) == hipSuccess);
        }
        c.check();
    }
    if (st) REQUIRE(hipStreamDestroy(st) == hipSuccess);
}

// a batch of empty items needs no buffer: txs may be null when the offsets give it no bytes.  Every item comes out as the vectors' own empty item does, whichever piece
// or shard it falls to
static void group_null_buffer(plume_ctx* ctx, const char* what, size_t chunk) {
    g_what = what;
    size_t j = 0;
    while (j < g_n && g_off[j + 1] != g_off[j]) j++;
    REQUIRE(j < g_n);                                                                  // the vectors hold an empty item
    if (chunk) REQUIRE(plume_set_chunk(ctx, chunk) == 0);
    constexpr size_t m = 11;
    const std::vector<uint64_t> off(m + 1, 5);
    Arr hash(32 * m, 0), r(32 * m, 0), s(32 * m, 0), v(m, 0), chain(8 * m, 0), type(m, 0), status(m, 0), pk(64 * m, 0), addr(20 * m, 0), schain(8 * m, 0), stype(m, 0), sstatus(m, 0);
    REQUIRE(plume_eth_tx_parse_batch(ctx, m, nullptr, off.data(), hash.p, r.p, s.p, v.p, (uint64_t*)chain.p, type.p, status.p) == 0);
    REQUIRE(plume_eth_tx_sender_batch(ctx, PLUME_ECDSA_LOW_S, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, m, nullptr, off.data(), nullptr, pk.p, addr.p, (uint64_t*)schain.p, stype.p,
                                      sstatus.p) == 0);
    for (size_t i = 0; i < m; i++) {
        REQUIRE(std::memcmp(hash.p + 32 * i, g_hash.data() + 32 * j, 32) == 0 && std::memcmp(r.p + 32 * i, g_r.data() + 32 * j, 32) == 0 &&
                std::memcmp(s.p + 32 * i, g_s.data() + 32 * j, 32) == 0 && v.p[i] == g_v[j] && std::memcmp(chain.p + 8 * i, g_chain.data() + 8 * j, 8) == 0 && type.p[i] == g_type[j] &&
                status.p[i] == g_status[j]);
        REQUIRE(std::memcmp(pk.p + 64 * i, g_pk.data() + 64 * j, 64) == 0 && std::memcmp(addr.p + 20 * i, g_addr.data() + 20 * j, 20) == 0 && sstatus.p[i] == g_sstatus[j] &&
                std::memcmp(schain.p + 8 * i, g_chain.data() + 8 * j, 8) == 0 && stype.p[i] == g_type[j]);
    }
    REQUIRE(plume_eth_tx_parse_batch(ctx, m, nullptr, g_off.data(), hash.p, r.p, s.p, v.p, nullptr, nullptr, nullptr) == PLUME_ERR_ARG &&
            std::string(plume_last_error()).find("null transaction buffer") != std::string::npos);     // ... and only then
    REQUIRE(plume_set_chunk(ctx, (size_t)1 << 20) == 0);
}

static void group_stages_and_order(plume_ctx* ctx) {
    g_what = "stage lists; a sender and a parse back to back on one caller stream";
    hipStream_t st = nullptr;
    REQUIRE(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
    REQUIRE(plume_set_stage_timing(ctx, 1) == 0);
    Call a(true, 3, 40, 31, 2), b(false, 0, g_n, 7, 2);
    REQUIRE(a.run(ctx, st) == 0);
    REQUIRE(hipStreamSynchronize(st) == hipSuccess);
    REQUIRE((last_stage_names(ctx) == std::vector<std::string>{"eth_tx_parse", "ecdsa_prepare", "tables", "ecdsa_mul", "to_affine", "ecdsa_finalize"}));
    REQUIRE(b.run(ctx, st) == 0);
    REQUIRE(hipStreamSynchronize(st) == hipSuccess);
    REQUIRE((last_stage_names(ctx) == std::vector<std::string>{"eth_tx_parse"}));
    REQUIRE(plume_set_stage_timing(ctx, 0) == 0);
    a.check(); b.check();
    Call c(true, 10, 33, 7, 2), d(true, 50, 20, 23, 2), e(false, 7, 90, 5, 2);
    REQUIRE(plume_set_sub_batches(ctx, 2) == 0);
    REQUIRE(c.run(ctx, st) == 0 && d.run(ctx, st, 0) == 0 && e.run(ctx, st) == 0);
    REQUIRE(hipStreamSynchronize(st) == hipSuccess);
    REQUIRE(plume_set_sub_batches(ctx, 1) == 0);
    c.check(); e.check();
    for (size_t i = 0; i < d.n; i++)                                                   // without the low-s rule at least everything the rule accepts recovers, to the same bytes
        if (g_sstatus[d.lo + i] != PLUME_ECDSA_INVALID) REQUIRE(std::memcmp(d.pk.p + 64 * i, g_pk.data() + 64 * (d.lo + i), 64) == 0 && d.status.p[i] == PLUME_ECDSA_MATCH);
    REQUIRE(hipStreamDestroy(st) == hipSuccess);
}

static void group_arguments(plume_ctx* ctx) {
    g_what = "arguments";
    Call c(true, 0, 4, 31, 0), p(false, 0, 4, 7, 0);
    const uint8_t* T = g_txs.data();
    const uint64_t* O = g_off.data();
    uint64_t* ch = (uint64_t*)c.chain.p;
    REQUIRE(plume_eth_tx_parse_batch(nullptr, 4, T, O, p.hash.p, p.r.p, p.s.p, p.v.p, nullptr, nullptr, nullptr) == PLUME_ERR_ARG);
    REQUIRE(plume_eth_tx_parse_batch(ctx, 4, T, nullptr, p.hash.p, p.r.p, p.s.p, p.v.p, nullptr, nullptr, nullptr) == PLUME_ERR_ARG);
    REQUIRE(plume_eth_tx_parse_batch(ctx, 4, T, O, nullptr, p.r.p, p.s.p, p.v.p, nullptr, nullptr, nullptr) == PLUME_ERR_ARG);
    REQUIRE(plume_eth_tx_parse_batch(ctx, 4, T, O, p.hash.p, nullptr, p.s.p, p.v.p, nullptr, nullptr, nullptr) == PLUME_ERR_ARG);
    REQUIRE(plume_eth_tx_parse_batch(ctx, 4, T, O, p.hash.p, p.r.p, nullptr, p.v.p, nullptr, nullptr, nullptr) == PLUME_ERR_ARG);
    REQUIRE(plume_eth_tx_parse_batch(ctx, 4, T, O, p.hash.p, p.r.p, p.s.p, nullptr, nullptr, nullptr, nullptr) == PLUME_ERR_ARG);
    REQUIRE(plume_eth_tx_parse_batch(ctx, 4, nullptr, O, p.hash.p, p.r.p, p.s.p, p.v.p, nullptr, nullptr, nullptr) == PLUME_ERR_ARG);
    REQUIRE(plume_eth_tx_parse_batch(ctx, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    std::vector<uint64_t> down(O, O + 9);
    down[4] = down[3] - 1;
    REQUIRE(plume_eth_tx_parse_batch(ctx, 8, T, down.data(), p.hash.p, p.r.p, p.s.p, p.v.p, nullptr, nullptr, nullptr) == PLUME_ERR_ARG);
    REQUIRE(plume_eth_tx_sender_batch(ctx, PLUME_ECDSA_LOW_S, 0, 0, 8, T, down.data(), nullptr, c.pk.p, nullptr, nullptr, nullptr, nullptr) == PLUME_ERR_ARG);
    for (int flags : {2, 3, 0x100, -1}) REQUIRE(plume_eth_tx_sender_batch(ctx, flags, 0, 0, 4, T, O, nullptr, c.pk.p, c.addr.p, ch, c.type.p, c.status.p) == PLUME_ERR_ARG);
    for (int pf : {2, -1}) REQUIRE(plume_eth_tx_sender_batch(ctx, 0, pf, 0, 4, T, O, nullptr, c.pk.p, c.addr.p, ch, c.type.p, c.status.p) == PLUME_ERR_ARG);
    for (int af : {3, -1}) REQUIRE(plume_eth_tx_sender_batch(ctx, 0, 0, af, 4, T, O, nullptr, c.pk.p, c.addr.p, ch, c.type.p, c.status.p) == PLUME_ERR_ARG);
    REQUIRE(plume_eth_tx_sender_batch(ctx, 0, 0, 0, 4, T, O, nullptr, nullptr, nullptr, ch, c.type.p, nullptr) == PLUME_ERR_ARG && std::string(plume_last_error()) == "no output array");
    REQUIRE(plume_eth_tx_sender_batch(nullptr, 0, 0, 0, 4, T, O, nullptr, c.pk.p, nullptr, nullptr, nullptr, nullptr) == PLUME_ERR_ARG);
    REQUIRE(plume_eth_tx_sender_batch(ctx, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    REQUIRE(c.untouched() && p.untouched());
    plume_ctx* multi = nullptr;
    int ids[2] = {0, 1};
    REQUIRE(plume_init_multi(&multi, ids, 2) == 0);
    Call d(false, 0, 8, 7, 2), e(true, 0, 8, 31, 2);
    REQUIRE(d.run(multi, nullptr) == PLUME_ERR_ARG && e.run(multi, nullptr) == PLUME_ERR_ARG);       // device pointers belong to one GPU
    plume_destroy(multi);
    REQUIRE(plume_set_chunk(ctx, 3) == 0);
    REQUIRE(d.run(ctx, nullptr) == 0);                                                 // the device form of the parse is one launch whatever the chunk size is
    REQUIRE(e.run(ctx, nullptr) == PLUME_ERR_ARG);                                     // ... the sender's takes at most one chunk, like the recovery's
    REQUIRE(plume_set_chunk(ctx, (size_t)1 << 20) == 0);
    REQUIRE(hipDeviceSynchronize() == hipSuccess);
    d.check();
    REQUIRE(e.untouched());
}

// every allocation of one host-form call fails in turn
static void group_failing_allocations(bool sender) {
    const Outstanding before;
    plume_ctx* ctx = nullptr;
    REQUIRE(plume_init(&ctx, 0) == 0);
    (void)mockhip::fail_allocation(-1);
    { Call c(sender, 0, 30, sender ? 31 : 7, 0); g_what = "allocations: counting call"; REQUIRE(c.run(ctx, nullptr) == 0); c.check(); }
    const long made = mockhip::fail_allocation(-1);
    REQUIRE(made >= (sender ? 12 : 10));                                               // the offsets (page-locked and device), the bytes, the outputs' staging; the sender: the comb and the workspace too
    plume_destroy(ctx);
    for (long k = 0; k < made; k++) {
        g_what = std::string("allocations: ") + (sender ? "sender" : "parse") + ", number " + std::to_string(k) + " fails";
        REQUIRE(plume_init(&ctx, 0) == 0);
        Call c(sender, 2, 30, sender ? 31 : 7, (int)(k & 1));
        (void)mockhip::fail_allocation(k);
        REQUIRE(c.run(ctx, nullptr) == PLUME_ERR_HIP);
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
    { Call c(false, 0, g_n, 7, 0); g_what = "parse only"; REQUIRE(c.run(ctx, nullptr) == 0); c.check(); }
    g_what = "no table";
    REQUIRE(mockhip::outstanding(0) <= dev_after_init + 9);                            // the bytes, the offsets and the seven outputs' staging: no table, no workspace
    group(ctx, "one device, host form, one chunk", 4, false, 0, 48);
    group(ctx, "one device, host form, chunks of 7", 8, false, 7, 40);
    group(ctx, "one device, host form, chunks of 1", 2, false, 1, 5);
    group_null_buffer(ctx, "one device, empty items of a null buffer, chunks of 4", 4);
    REQUIRE(plume_set_chunk(ctx, (size_t)1 << 20) == 0);
    group(ctx, "one device, device form", 8, true, 0, 48);
    group_stages_and_order(ctx);
    for (int devices : {3, 8}) {
        plume_ctx* multi = nullptr;
        int ids[8] = {0, 1, 2, 3, 4, 5, 6, 7};
        REQUIRE(plume_init_multi(&multi, ids, devices) == 0);
        REQUIRE(plume_num_shards(multi) == devices);
        group(multi, devices == 3 ? "three devices, host form" : "eight devices, host form", 6, false, devices == 3 ? 5 : 0, 48);
        group_null_buffer(multi, "several devices, empty items of a null buffer", devices == 3 ? 2 : 0);
        plume_destroy(multi);
    }
    group_arguments(ctx);
    plume_destroy(ctx);
    group_failing_allocations(false);
    group_failing_allocations(true);
    REQUIRE(mockhip::outstanding(0) == 0 && mockhip::outstanding(2) == 0 && mockhip::outstanding(3) == 0);
    std::printf("eth_tx_driver seed %llu: ok\n", seed);
    return 0;
}
