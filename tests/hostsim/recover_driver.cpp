// TEST INFRASTRUCTURE ONLY.  plume_recover_batch* on the library's host side (capi_recover / capi_recover_device in csrc/plume_capi.hip + csrc/plume_recover_capi.hip) on the
// mock HIP runtime, under the sanitizers (tests/test_recover_hostsim.py).  Batches are signed by the C oracle (V1 and V2 items mixed, one item with the nonce r = 0) and then
// mutated field by field.  What must come out is pinned by the C oracle:
//   an item whose c or s is outside [1, n-1] or whose pk / nullifier is no curve point (oracle_point_mul refuses it) and not all zero: status 3, all-zero records;
//   every other item: hashed_to_curve = oracle_hash_to_curve_batch; r_point / hashed_to_curve_r of an unmutated item = r G and r H (oracle_point_mul), and of any item
//   points of the curve; version 2 status = oracle_verify_batch(2); version 1 status = oracle_verify_batch(1) handed the recovered points; the same points for both versions.
// That is checked on one call per version (64-byte records, every output, host form); every other call -- the three formats, every subset of NULL outputs, pieces of 5-64
// items, page-locked arrays, the device form on a caller stream, a plume_init_multi context over eight mock devices, two lanes in flight on two streams, sub_batches = 2 --
// must reproduce those bytes, leave the arrays it was not given untouched, and report "recover_finalize" as its last stage.
#define DRIVER_NAME "recover_driver"
#include "driver_prelude.h"

extern "C" {
int oracle_sign_batch(int version, size_t n, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* sk, const uint8_t* r, const uint8_t* pk_in, uint8_t* pk,
                      uint8_t* nullifier, uint8_t* c, uint8_t* s, uint8_t* r_point, uint8_t* hashed_to_curve_r, uint8_t* h_out, uint8_t* status, int nthreads);
int oracle_verify_batch(int version, size_t n, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* pk, const uint8_t* nullifier, const uint8_t* c, const uint8_t* s,
                        const uint8_t* r_point, const uint8_t* hashed_to_curve_r, uint8_t* ok, int nthreads);
int oracle_hash_to_curve_batch(size_t n, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* pk, uint8_t* h_out, int nthreads);
int oracle_point_mul(const uint8_t k[32], const uint8_t p[64], uint8_t out[64]);
size_t oracle_sec1_compress(const uint8_t p[64], uint8_t out[33]);
}

static const uint8_t kOrder[32] = {0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFE,
                                   0xBA, 0xAE, 0xDC, 0xE6, 0xAF, 0x48, 0xA0, 0x3B, 0xBF, 0xD2, 0x5E, 0x8C, 0xD0, 0x36, 0x41, 0x41};
static const uint8_t kG[64] = {0x79, 0xBE, 0x66, 0x7E, 0xF9, 0xDC, 0xBB, 0xAC, 0x55, 0xA0, 0x62, 0x95, 0xCE, 0x87, 0x0B, 0x07, 0x02, 0x9B, 0xFC, 0xDB, 0x2D, 0xCE,
                               0x28, 0xD9, 0x59, 0xF2, 0x81, 0x5B, 0x16, 0xF8, 0x17, 0x98, 0x48, 0x3A, 0xDA, 0x77, 0x26, 0xA3, 0xC4, 0x65, 0x5D, 0xA4, 0xFB, 0xFC,
                               0x0E, 0x11, 0x08, 0xA8, 0xFD, 0x17, 0xB4, 0x48, 0xA6, 0x85, 0x54, 0x19, 0x9C, 0x47, 0xD0, 0x8F, 0xFB, 0x10, 0xD4, 0xB8};

static bool scalar_ok(const uint8_t* k) { return !all_of(k, 32, 0) && std::memcmp(k, kOrder, 32) < 0; }
static bool point_ok(const uint8_t* p) {
    if (all_of(p, 64, 0)) return true;
    uint8_t one[32] = {0}, out[64];
    one[31] = 1;
    return oracle_point_mul(one, p, out) != 0;
}

struct Batch {
    size_t n = 0;
    std::vector<uint8_t> msgs, pk, nul, c, s;
    std::vector<uint64_t> off;
    std::vector<uint8_t> valid, honest, rG, rH;            // per item; r G and r H of the items left as signed
    std::vector<uint8_t> want[2][4];                      // [version - 1]: r_point, hashed_to_curve_r, hashed_to_curve (64-byte records), status -- from the pinned calls
};

static Batch make_batch(size_t n) {
    Batch b;
    b.n = n;
    b.off.push_back(0);
    for (size_t i = 0; i < n; i++) {
        const size_t len = rng() % 9 == 0 ? 0 : rng() % 121;
        for (size_t k = 0; k < len; k++) b.msgs.push_back((uint8_t)rng());
        b.off.push_back(b.msgs.size());
    }
    b.msgs.resize(b.msgs.size() + 16, 0);
    std::vector<uint8_t> sk(32 * n), r(32 * n);
    for (size_t i = 0; i < 32 * n; i++) { sk[i] = (uint8_t)rng(); r[i] = (uint8_t)rng(); }
    for (size_t i = 0; i < n; i++) { sk[32 * i] &= 0x7F; sk[32 * i + 31] |= 1; r[32 * i] &= 0x7F; r[32 * i + 31] |= 1; }
    const size_t zero = n > 2 ? rng() % n : n;                                      // the accept-at-identity input: r = 0
    if (zero < n) std::memset(&r[32 * zero], 0, 32);
    std::vector<uint8_t> o[2][6], st(n);
    for (int v = 0; v < 2; v++) {
        for (int k = 0; k < 6; k++) o[v][k].assign((k == 2 || k == 3 ? 32 : 64) * n, 0);
        REQUIRE(oracle_sign_batch(v + 1, n, b.msgs.data(), b.off.data(), sk.data(), r.data(), nullptr, o[v][0].data(), o[v][1].data(), o[v][2].data(), o[v][3].data(),
                                  o[v][4].data(), o[v][5].data(), nullptr, st.data(), 1) == 0);
    }
    b.pk = o[0][0]; b.nul = o[0][1]; b.c.resize(32 * n); b.s.resize(32 * n);
    b.rG = o[0][4]; b.rH = o[0][5];
    b.honest.assign(n, 1);
    for (size_t i = 0; i < n; i++) {                                                 // V1 and V2 signatures mixed
        const int v = (int)(rng() & 1);
        std::memcpy(&b.c[32 * i], &o[v][2][32 * i], 32); std::memcpy(&b.s[32 * i], &o[v][3][32 * i], 32);
    }
    for (size_t i = 0; i < n; i++) {
        if (i == zero) continue;
        const unsigned kind = (unsigned)(rng() % 12);
        if (kind >= 6) continue;
        b.honest[i] = 0;
        const size_t j = rng() % n;
        switch (kind) {
            case 0: b.s[32 * i + 31] ^= 1; break;
            case 1: if (rng() & 1) std::memset(&b.c[32 * i], 0, 32); else std::memcpy(&b.c[32 * i], kOrder, 32); break;
            case 2: for (size_t k = 0; k < 64; k++) b.pk[64 * i + k] = (uint8_t)rng(); break;
            case 3: std::memcpy(&b.nul[64 * i], &o[0][1][64 * j], 64); if (j == i) b.nul[64 * i + 63] ^= 1; break;
            case 4: std::memset(&b.pk[64 * i], 0, 64); break;                        // an identity pk is a value
            default: b.nul[64 * i + 40] ^= 0x20; break;                              // off the curve
        }
    }
    b.valid.resize(n);
    for (size_t i = 0; i < n; i++) b.valid[i] = scalar_ok(&b.c[32 * i]) && scalar_ok(&b.s[32 * i]) && point_ok(&b.pk[64 * i]) && point_ok(&b.nul[64 * i]);
    return b;
}

static const size_t kWidth[3] = {64, 33, 64};
// a 64-byte record in the given format
static void convert(uint8_t* dst, const uint8_t* rec, int fmt) {
    if (fmt == PLUME_RECOVER_FMT_AFFINE64) { std::memcpy(dst, rec, 64); return; }
    if (fmt == PLUME_RECOVER_FMT_SEC1) { std::memset(dst, 0, 33); if (!all_of(rec, 64, 0)) REQUIRE(oracle_sec1_compress(rec, dst) == 33); return; }
    for (int k = 0; k < 2; k++) for (int j = 0; j < 32; j++) dst[32 * k + j] = rec[32 * k + 31 - j];          // four little-endian 64-bit registers per coordinate
}

// the pinned calls: 64-byte records, every output, host form, one per version -- against the oracle
static void pin(plume_ctx* ctx, Batch& b) {
    const size_t n = b.n;
    for (int v = 0; v < 2; v++) {
        for (int k = 0; k < 4; k++) b.want[v][k].assign((k == 3 ? 1 : 64) * n, kFill);
        REQUIRE(plume_recover_batch(ctx, v + 1, PLUME_RECOVER_FMT_AFFINE64, n, b.msgs.data(), b.off.data(), b.pk.data(), b.nul.data(), b.c.data(), b.s.data(),
                                    b.want[v][0].data(), b.want[v][1].data(), b.want[v][2].data(), b.want[v][3].data()) == 0);
    }
    std::vector<uint8_t> pkh = b.pk, h(64 * n), ok2(n), ok1(n);
    for (size_t i = 0; i < n; i++) if (!b.valid[i]) std::memset(&pkh[64 * i], 0, 64);
    REQUIRE(oracle_hash_to_curve_batch(n, b.msgs.data(), b.off.data(), pkh.data(), h.data(), 1) == 0);
    REQUIRE(oracle_verify_batch(2, n, b.msgs.data(), b.off.data(), b.pk.data(), b.nul.data(), b.c.data(), b.s.data(), nullptr, nullptr, ok2.data(), 1) == 0);
    REQUIRE(oracle_verify_batch(1, n, b.msgs.data(), b.off.data(), b.pk.data(), b.nul.data(), b.c.data(), b.s.data(), b.want[0][0].data(), b.want[0][1].data(), ok1.data(), 1) == 0);
    size_t seen[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < n; i++) {
        for (int k = 0; k < 3; k++) REQUIRE(std::memcmp(&b.want[0][k][64 * i], &b.want[1][k][64 * i], 64) == 0);       // the points do not depend on the version
        if (!b.valid[i]) {
            for (int v = 0; v < 2; v++) {
                REQUIRE(b.want[v][3][i] == PLUME_RECOVER_INVALID);
                for (int k = 0; k < 3; k++) REQUIRE(all_of(&b.want[v][k][64 * i], 64, 0));
            }
            seen[3]++;
            continue;
        }
        REQUIRE(std::memcmp(&b.want[1][2][64 * i], &h[64 * i], 64) == 0);
        REQUIRE(point_ok(&b.want[1][0][64 * i]) && point_ok(&b.want[1][1][64 * i]));
        if (b.honest[i]) {
            REQUIRE(std::memcmp(&b.want[1][0][64 * i], &b.rG[64 * i], 64) == 0 && std::memcmp(&b.want[1][1][64 * i], &b.rH[64 * i], 64) == 0);
            REQUIRE(b.want[0][3][i] + b.want[1][3][i] == PLUME_RECOVER_MATCH);                                       // signed as V1 or as V2: exactly one hash matches
        }
        REQUIRE(b.want[1][3][i] == (ok2[i] == 1 ? PLUME_RECOVER_MATCH : PLUME_RECOVER_MISMATCH));
        REQUIRE(b.want[0][3][i] == (ok1[i] == 1 ? PLUME_RECOVER_MATCH : PLUME_RECOVER_MISMATCH));
        seen[b.want[1][3][i]]++;
    }
    if (n >= 60) REQUIRE(seen[0] && seen[1] && seen[3]);
}

struct Call {
    const Batch& b;
    int version, fmt, present, kind;
    Arr msgs, off, pk, nul, c, s, o0, o1, o2, o3;
    Call(const Batch& bb, int v, int f, int pres, int k)
        : b(bb), version(v), fmt(f), present(pres), kind(k), msgs(bb.msgs.size(), k, bb.msgs.data()), off(8 * bb.off.size(), k, bb.off.data()), pk(64 * bb.n, k, bb.pk.data()),
          nul(64 * bb.n, k, bb.nul.data()), c(32 * bb.n, k, bb.c.data()), s(32 * bb.n, k, bb.s.data()), o0(kWidth[f] * bb.n, k), o1(kWidth[f] * bb.n, k), o2(kWidth[f] * bb.n, k),
          o3(bb.n, k) {}
    uint8_t* out(int k) { Arr* a[4] = {&o0, &o1, &o2, &o3}; return (present >> k) & 1 ? a[k]->p : nullptr; }
    int run(plume_ctx* ctx, hipStream_t st) {
        if (kind == 2)
            return plume_recover_batch_device(ctx, version, fmt, b.n, msgs.p, (const uint64_t*)off.p, b.msgs.size(), pk.p, nul.p, c.p, s.p, out(0), out(1), out(2), out(3), st);
        return plume_recover_batch(ctx, version, fmt, b.n, msgs.p, (const uint64_t*)off.p, pk.p, nul.p, c.p, s.p, out(0), out(1), out(2), out(3));
    }
    void check() {                                        // (the mock's device memory is host memory)
        Arr* a[4] = {&o0, &o1, &o2, &o3};
        const size_t W = kWidth[fmt];
        std::vector<uint8_t> rec(64);
        for (int k = 0; k < 4; k++) {
            if (!((present >> k) & 1)) { REQUIRE(all_of(a[k]->p, a[k]->bytes, kFill)); continue; }
            if (k == 3) { REQUIRE(std::memcmp(o3.p, b.want[version - 1][3].data(), b.n) == 0); continue; }
            for (size_t i = 0; i < b.n; i++) {
                convert(rec.data(), &b.want[version - 1][k][64 * i], fmt);
                REQUIRE(std::memcmp(a[k]->p + W * i, rec.data(), W) == 0);
            }
        }
    }
};

static void last_stage_is_recover(plume_ctx* ctx) {
    const char* names[64];
    float ms[64];
    const int ns = plume_last_stage_times(ctx, names, ms, 64);
    REQUIRE(ns >= 4 && std::string(names[ns - 1]) == "recover_finalize" && std::string(names[ns - 2]) == "to_affine");
    for (int i = 0; i < ns; i++) REQUIRE(std::string(names[i]) != "verify_finalize");
}

static void group(plume_ctx* ctx, plume_ctx* pinned_on, const char* what, int calls, bool device_form, bool timed) {
    hipStream_t st = nullptr;
    if (device_form) REQUIRE(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
    for (int k = 0; k < calls; k++) {
        const size_t piece = 5 + rng() % 60, n = k == 0 ? 70 + rng() % 60 : 1 + rng() % 130;
        if (!device_form) REQUIRE(plume_set_host_piece(ctx, piece) == 0);
        Batch b = make_batch(n);
        g_what = std::string(what) + " call " + std::to_string(k) + ": n " + std::to_string(n) + ", piece " + std::to_string(piece);
        pin(pinned_on, b);
        const int present = k == 0 ? 15 : 1 + (int)(rng() % 15), fmt = (int)(rng() % 3), version = 1 + (int)(rng() & 1);
        g_what += ", v" + std::to_string(version) + ", format " + std::to_string(fmt) + ", outputs " + std::to_string(present);
        Call c(b, version, fmt, present, device_form ? 2 : (int)(rng() & 1));
        REQUIRE(c.run(ctx, st) == 0);
        if (device_form) REQUIRE(hipStreamSynchronize(st) == hipSuccess);
        c.check();
        if (timed && device_form) last_stage_is_recover(ctx);
    }
    if (st) REQUIRE(hipStreamDestroy(st) == hipSuccess);
}

// two lanes in flight: four calls issued on two caller streams before anything is waited for
static void group_in_flight(plume_ctx* ctx, plume_ctx* pinned_on) {
    REQUIRE(plume_set_in_flight(ctx, 2) == 0);
    hipStream_t st[2];
    for (hipStream_t& q : st) REQUIRE(hipStreamCreateWithFlags(&q, hipStreamNonBlocking) == hipSuccess);
    std::vector<Batch> bs;
    for (int k = 0; k < 4; k++) { g_what = "in flight, batch " + std::to_string(k); bs.push_back(make_batch(20 + rng() % 60)); pin(pinned_on, bs.back()); }
    std::vector<Call*> cs;
    for (int k = 0; k < 4; k++) {
        cs.push_back(new Call(bs[k], 1 + (k & 1), (int)(rng() % 3), 15, 2));
        g_what = "in flight, call " + std::to_string(k);
        REQUIRE(cs[k]->run(ctx, st[k & 1]) == 0);
    }
    for (hipStream_t q : st) REQUIRE(hipStreamSynchronize(q) == hipSuccess);
    for (int k = 0; k < 4; k++) { g_what = "in flight, check " + std::to_string(k); cs[k]->check(); delete cs[k]; }
    REQUIRE(plume_set_in_flight(ctx, 1) == 0);
    for (hipStream_t q : st) REQUIRE(hipStreamDestroy(q) == hipSuccess);
}

static void group_arguments(plume_ctx* ctx) {
    g_what = "arguments";
    Batch b = make_batch(4);
    std::vector<uint8_t> o(64 * 4, kFill);
    auto call = [&](plume_ctx* c, int v, int f, size_t n, const uint8_t* pk, uint8_t* out) {
        return plume_recover_batch(c, v, f, n, b.msgs.data(), b.off.data(), pk, b.nul.data(), b.c.data(), b.s.data(), out, nullptr, nullptr, nullptr);
    };
    REQUIRE(call(nullptr, 2, 0, 4, b.pk.data(), o.data()) == PLUME_ERR_ARG);
    REQUIRE(call(ctx, 0, 0, 4, b.pk.data(), o.data()) == PLUME_ERR_ARG && call(ctx, 3, 0, 4, b.pk.data(), o.data()) == PLUME_ERR_ARG);
    REQUIRE(call(ctx, 2, 3, 4, b.pk.data(), o.data()) == PLUME_ERR_ARG && call(ctx, 2, -1, 4, b.pk.data(), o.data()) == PLUME_ERR_ARG);
    REQUIRE(call(ctx, 2, 0, 4, nullptr, o.data()) == PLUME_ERR_ARG);
    REQUIRE(call(ctx, 2, 0, 4, b.pk.data(), nullptr) == PLUME_ERR_ARG);                // no output at all
    REQUIRE(call(ctx, 2, 0, 0, b.pk.data(), nullptr) == 0);                            // an empty batch is no error, as for verify
    REQUIRE(all_of(o.data(), o.size(), kFill));
    REQUIRE(plume_set_chunk(ctx, 3) == 0);                                             // the device form refuses more than a chunk; the host form cuts
    Call d(b, 2, 0, 15, 2);
    REQUIRE(d.run(ctx, nullptr) == PLUME_ERR_ARG);
    pin(ctx, b);
    REQUIRE(plume_set_chunk(ctx, (size_t)1 << 20) == 0);
    plume_ctx* multi = nullptr;
    int ids[2] = {0, 1};
    REQUIRE(plume_init_multi(&multi, ids, 2) == 0);
    REQUIRE(d.run(multi, nullptr) == PLUME_ERR_ARG);                                   // device pointers belong to one GPU
    plume_destroy(multi);
}

int main(int argc, char** argv) {
    const unsigned long long seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
    rng.seed(seed);
    setenv("PLUME_OVERLAP_MIN", "8", 1);                     // (sub-batches from 8 items on; a slice still needs 8192 items, so the knob's bookkeeping runs with one slice)
    plume_ctx* ctx = nullptr;
    REQUIRE(plume_init(&ctx, 0) == 0);
    unsetenv("PLUME_OVERLAP_MIN");
    group_arguments(ctx);
    group(ctx, ctx, "one device, host form", 8, false, false);
    REQUIRE(plume_set_stage_timing(ctx, 1) == 0);
    group(ctx, ctx, "one device, device form", 6, true, true);
    REQUIRE(plume_set_sub_batches(ctx, 2) == 0);
    group(ctx, ctx, "one device, device form, sub_batches 2", 2, true, false);
    REQUIRE(plume_set_sub_batches(ctx, 1) == 0);
    REQUIRE(plume_set_stage_timing(ctx, 0) == 0);
    group_in_flight(ctx, ctx);
    plume_ctx* multi = nullptr;
    int ids[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    REQUIRE(plume_init_multi(&multi, ids, 8) == 0);
    group(multi, ctx, "eight devices, host form", 5, false, false);
    plume_destroy(multi);
    plume_destroy(ctx);
    REQUIRE(mockhip::outstanding(0) == 0 && mockhip::outstanding(2) == 0 && mockhip::outstanding(3) == 0);
    std::printf("recover_driver seed %llu: ok\n", seed);
    return 0;
}
