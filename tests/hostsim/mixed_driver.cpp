// TEST INFRASTRUCTURE ONLY.  Every call family of the library on ONE mock context, under the sanitizers (tests/test_mixed_hostsim.py): no call's result may depend on what
// its context ran before.  The families share one workspace (csrc/plume_capi_ctx.h) and lay it out differently; the mock runtime hands out dirty (0xA5) device memory, and
// here -- unlike in the families' own drivers -- a context's scratch is also dirty with ANOTHER family's bytes, counters and flags.
// usage: mixed_driver SEED [WALK [GROUPS]].  WALK: calls of the seeded walk (default 300).  GROUPS: letters of the groups to run (default "abc").
// Each family has a "large" (70 items) and a "small" (9 items) deterministic input that carries the family's invalid items, at positions that differ between the two sizes
// (i % 7 == 3 and the last item at 70; i % 7 == 5 and the last item at 9), so a stale flag or status byte is a wrong one.  The reference of an entry is the same call on a
// context that has done nothing else, computed once at start-up in the host form and required of the device form too, over outputs pre-filled with two different bytes
// (so every output byte is one the call wrote); the families' own drivers hold such results to their restatements.  The SEC1 forms of verify and sign are entries too: the
// decompression stage has scratch of its own, one reject flag per item among it.  Groups, each on one long-lived context, every byte of every output and status array compared:
//   a  every ordered pair of entries of different families, and each family's large entry followed by its small one;
//   b  a seeded walk over all entries; before each call the form (host-pointer / device), the stream (two caller streams or the context's own), the signer's self-check,
//      the form of equation 1 (0 / 1 / 3), the signer's schedule (0 / 1 / 2) and stage timing are drawn;
//   c  the same walk on a two-device context (host forms), on a context with two batches in flight, and on one whose host calls take three or more pieces.
// plume_last_redo_tasks is read on the single-lane contexts after every call once the redo list is known: 0 behind a verify call, an error behind an ECDSA-family call.
// A mismatch prints "mixed_driver: seed S, call I: <entry> ... after <entry>" and exits with status 2.
#define DRIVER_NAME "mixed_driver"
#include "driver_prelude.h"

#include <functional>
#include <memory>

typedef std::vector<uint8_t> Bytes;
static const size_t kLarge = 70, kSmall = 9;
static const uint8_t kN[32] = {0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFE,
                               0xBA, 0xAE, 0xDC, 0xE6, 0xAF, 0x48, 0xA0, 0x3B, 0xBF, 0xD2, 0x5E, 0x8C, 0xD0, 0x36, 0x41, 0x41};
static unsigned long long g_seed = 1;

static bool bad_at(size_t n, size_t i) { return i % 7 == (n >= kLarge ? 3u : 5u) || i == n - 1; }
static std::vector<size_t> bad_list(size_t n) { std::vector<size_t> v; for (size_t i = 0; i < n; i++) if (bad_at(n, i)) v.push_back(i); return v; }

enum Redo { kNone = 0, kVerify, kEcdsa, kArmedIfChecked, kEcdsaIfChecked };

// one call (or a chain of calls that feed one another) of a family at one size
struct Entry {
    std::string name;
    int family = 0;
    size_t n = 0;
    std::vector<Bytes> in, in_dev;                         // the input arrays as bytes; in_dev: what the device form is given where that differs (empty: the same)
    std::vector<size_t> out;                               // bytes of every output array
    std::function<int(plume_ctx*, bool, hipStream_t, uint8_t* const*, uint8_t* const*)> call;    // (ctx, device form, stream, inputs, outputs)
    std::vector<Bytes> want, want_dev;                     // the outputs of a context that has done nothing else
    Redo redo = kNone;
    int status = -1;                                       // the output that holds one status (verdict, flag) byte per item
    bool every = true;                                     // ... and every planted item changes its byte there (false: some do; see the family)
    const std::vector<Bytes>& inputs(bool dev) const { return dev && !in_dev.empty() ? in_dev : in; }
    const std::vector<Bytes>& expected(bool dev) const { return dev && !want_dev.empty() ? want_dev : want; }
};
static std::vector<Entry> g_entries;

// a call in flight: the caller's arrays, exactly as large as the call may touch
struct Running {
    const Entry* e;
    bool dev;
    hipStream_t st;
    std::vector<std::unique_ptr<Arr>> in, out;
    Running(plume_ctx* ctx, const Entry& en, bool device, hipStream_t stream, int host_kind, uint8_t fill = kFill) : e(&en), dev(device), st(stream) {
        const int kind = device ? 2 : host_kind;
        for (const Bytes& b : en.inputs(device)) in.emplace_back(new Arr(b.size(), kind, b.data()));
        for (size_t bytes : en.out) { out.emplace_back(new Arr(bytes, kind)); std::memset(out.back()->p, fill, bytes); }     // (the mock's device memory is host memory)
        std::vector<uint8_t*> ip, op;
        for (auto& a : in) ip.push_back(a->p);
        for (auto& a : out) op.push_back(a->p);
        REQUIRE(en.call(ctx, device, stream, ip.data(), op.data()) == 0);
    }
    void wait() { if (dev) REQUIRE((st ? hipStreamSynchronize(st) : hipDeviceSynchronize()) == hipSuccess); }
    // the first output that differs from `want`, as text; empty: every byte is right, and no input was written
    std::string differs(const std::vector<Bytes>& want) const {
        for (size_t k = 0; k < out.size(); k++)
            if (std::memcmp(out[k]->p, want[k].data(), want[k].size()) != 0) {
                size_t at = 0;
                while (out[k]->p[at] == want[k][at]) at++;
                return "output " + std::to_string(k) + " differs at byte " + std::to_string(at) + " of " + std::to_string(want[k].size()) + " (" + std::to_string(out[k]->p[at]) + ", not " +
                       std::to_string(want[k][at]) + ")";
            }
        const std::vector<Bytes>& src = e->inputs(dev);
        for (size_t k = 0; k < in.size(); k++) if (std::memcmp(in[k]->p, src[k].data(), src[k].size()) != 0) return "input " + std::to_string(k) + " was written";
        return "";
    }
    std::vector<Bytes> outputs() const { std::vector<Bytes> v; for (auto& a : out) v.emplace_back(a->p, a->p + a->bytes); return v; }
};

// ------------------------------------------------------------------------------------------------------------ deterministic inputs
static std::mt19937_64 g_gen;                              // the inputs' generator: seeded per entry, never by the walk's seed
static Bytes rnd(size_t bytes) { Bytes b(bytes); for (auto& x : b) x = (uint8_t)g_gen(); return b; }
static Bytes scalars(size_t n) { Bytes b = rnd(32 * n); for (size_t i = 0; i < n; i++) { b[32 * i] &= 0x7F; b[32 * i + 31] |= 1; } return b; }
static Bytes offsets(const std::vector<size_t>& lens) {
    std::vector<uint64_t> off(lens.size() + 1, 0);
    for (size_t i = 0; i < lens.size(); i++) off[i + 1] = off[i] + lens[i];
    return Bytes((const uint8_t*)off.data(), (const uint8_t*)(off.data() + off.size()));
}
static const uint64_t* u64(const uint8_t* p) { return (const uint64_t*)p; }
static void put(Bytes& b, size_t at, const uint8_t* src, size_t len) { std::memcpy(b.data() + at, src, len); }
static void zero(Bytes& b, size_t at, size_t len) { std::memset(b.data() + at, 0, len); }

struct Plume {                                             // a signed batch of ragged messages: what the verify families start from
    size_t n;
    Bytes msgs, off, sk, r, pk, nul, c, s, rpt, hr, status;
};
static Plume plume_signed(plume_ctx* gen, size_t n, int version, unsigned seed) {
    g_gen.seed(seed);
    Plume b;
    b.n = n;
    std::vector<size_t> lens(n);
    for (size_t i = 0; i < n; i++) lens[i] = (size_t)(g_gen() % 70);
    b.off = offsets(lens);
    b.msgs = rnd((size_t)u64(b.off.data())[n] + 16);
    b.sk = scalars(n); b.r = scalars(n);
    b.pk.resize(64 * n); b.nul.resize(64 * n); b.c.resize(32 * n); b.s.resize(32 * n); b.rpt.resize(64 * n); b.hr.resize(64 * n); b.status.resize(n);
    REQUIRE(plume_sign_batch(gen, version, n, b.msgs.data(), u64(b.off.data()), b.sk.data(), b.r.data(), nullptr, b.pk.data(), b.nul.data(), b.c.data(), b.s.data(), b.rpt.data(),
                             b.hr.data(), b.status.data()) == 0);
    REQUIRE(all_of(b.status.data(), n, 0));
    return b;
}
// the planted items of a verify batch: a flipped s, c = n (no scalar), a pk off the curve, a neighbour's nullifier -- in turn
static void corrupt(Plume& b) {
    size_t j = 0;
    for (size_t i : bad_list(b.n)) {
        switch (j++ % 4) {
            case 0: b.s[32 * i + 31] ^= 1; break;
            case 1: put(b.c, 32 * i, kN, 32); break;
            case 2: b.pk[64 * i + 63] ^= 1; break;
            default: { Bytes prev(b.nul.begin() + 64 * (i - 1), b.nul.begin() + 64 * i); put(b.nul, 64 * i, prev.data(), 64); }
        }
    }
}

static void add(Entry e, int family, const char* fam, size_t n) {
    e.family = family; e.n = n;
    e.name = std::string(fam) + "[" + std::to_string(n) + "]";
    g_entries.push_back(std::move(e));
}

// ---- the families (in: the arrays in the order the lambdas index them)
static void fam_verify(plume_ctx* gen, int family, size_t n, int version, int nonzk) {
    Plume b = plume_signed(gen, n, version, 100 * family + (unsigned)n);
    corrupt(b);
    Entry e;
    e.in = {b.msgs, b.off, b.pk, b.nul, b.c, b.s, b.rpt, b.hr};
    e.out = {n};
    e.status = 0;
    e.redo = kVerify;
    e.call = [n, version, nonzk](plume_ctx* c, bool dev, hipStream_t st, uint8_t* const* i, uint8_t* const* o) {
        const uint8_t *rp = version == 1 || nonzk ? i[6] : nullptr, *hr = version == 1 || nonzk ? i[7] : nullptr;
        const size_t mb = (size_t)u64(i[1])[n] + 16;
        if (nonzk) return dev ? plume_verify_non_zk_batch_device(c, version, n, i[0], u64(i[1]), mb, i[2], i[3], i[5], rp, hr, i[4], o[0], st)
                              : plume_verify_non_zk_batch(c, version, n, i[0], u64(i[1]), i[2], i[3], i[5], rp, hr, i[4], o[0]);
        return dev ? plume_verify_batch_device(c, version, n, i[0], u64(i[1]), mb, i[2], i[3], i[4], i[5], rp, hr, o[0], st)
                   : plume_verify_batch(c, version, n, i[0], u64(i[1]), i[2], i[3], i[4], i[5], rp, hr, o[0]);
    };
    add(std::move(e), family, nonzk ? "verify_non_zk" : version == 1 ? "verify_v1" : "verify_v2", n);
}
// 64-byte affine records -> 33-byte SEC1 records: 02|03 || x
static Bytes compress(const Bytes& a64) {
    const size_t n = a64.size() / 64;
    Bytes out(33 * n);
    for (size_t i = 0; i < n; i++) { out[33 * i] = (uint8_t)(2 + (a64[64 * i + 63] & 1)); std::memcpy(&out[33 * i + 1], &a64[64 * i], 32); }
    return out;
}
// the SEC1 ingest (V1): the decompression stage in front of the verifier, with scratch of its own (the four decompressed arrays, one reject flag per item).  Planted: a
// prefix that is none, an x with no point on the curve (x = 5), the other root of a valid x, a flipped s -- over pk, nullifier, r_point and hashed_to_curve_r in turn
static void fam_verify_sec1(plume_ctx* gen, int family, size_t n) {
    Plume b = plume_signed(gen, n, 1, 100 * family + (unsigned)n);
    Bytes rec[4] = {compress(b.pk), compress(b.nul), compress(b.rpt), compress(b.hr)};
    size_t j = 0;
    for (size_t i : bad_list(n)) {
        Bytes& r = rec[(j / 4) % 4];
        switch (j++ % 4) {
            case 0: r[33 * i] = 5; break;
            case 1: std::memset(&r[33 * i + 1], 0, 32); r[33 * i + 32] = 5; break;
            case 2: r[33 * i] ^= 1; break;
            default: b.s[32 * i + 31] ^= 1;
        }
    }
    Entry e;
    e.in = {b.msgs, b.off, rec[0], rec[1], b.c, b.s, rec[2], rec[3]};
    e.out = {n};
    e.status = 0;
    e.redo = kVerify;
    e.call = [n](plume_ctx* c, bool dev, hipStream_t st, uint8_t* const* i, uint8_t* const* o) {
        const size_t mb = (size_t)u64(i[1])[n] + 16;
        return dev ? plume_verify_batch_sec1_device(c, 1, n, i[0], u64(i[1]), mb, i[2], i[3], i[4], i[5], i[6], i[7], o[0], st)
                   : plume_verify_batch_sec1(c, 1, n, i[0], u64(i[1]), i[2], i[3], i[4], i[5], i[6], i[7], o[0]);
    };
    add(std::move(e), family, "verify_sec1", n);
}
static void fam_recover(plume_ctx* gen, int family, size_t n) {
    Plume b = plume_signed(gen, n, 2, 100 * family + (unsigned)n);
    corrupt(b);
    Entry e;
    e.in = {b.msgs, b.off, b.pk, b.nul, b.c, b.s};
    e.out = {64 * n, 64 * n, 64 * n, n};
    e.status = 3;
    e.redo = kVerify;
    e.call = [n](plume_ctx* c, bool dev, hipStream_t st, uint8_t* const* i, uint8_t* const* o) {
        const size_t mb = (size_t)u64(i[1])[n] + 16;
        return dev ? plume_recover_batch_device(c, 2, PLUME_RECOVER_FMT_AFFINE64, n, i[0], u64(i[1]), mb, i[2], i[3], i[4], i[5], o[0], o[1], o[2], o[3], st)
                   : plume_recover_batch(c, 2, PLUME_RECOVER_FMT_AFFINE64, n, i[0], u64(i[1]), i[2], i[3], i[4], i[5], o[0], o[1], o[2], o[3]);
    };
    add(std::move(e), family, "recover", n);
}
static void fam_aggregate(plume_ctx* gen, int family, size_t n) {
    Plume b = plume_signed(gen, n, 1, 100 * family + (unsigned)n);
    corrupt(b);
    Entry e;
    e.in = {b.msgs, b.off, b.pk, b.nul, b.c, b.s, b.rpt, b.hr};
    e.out = {n, 72};
    e.status = 0; e.every = false;                         // (hash_ok: a flipped s leaves the challenge's hash right)
    e.call = [n](plume_ctx* c, bool dev, hipStream_t st, uint8_t* const* i, uint8_t* const* o) {
        static const uint8_t seed[32] = {7, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31};
        const size_t mb = (size_t)u64(i[1])[n] + 16;
        return dev ? plume_aggregate_check_device(c, 1, 0, n, i[0], u64(i[1]), mb, i[2], i[3], i[4], i[5], i[6], i[7], seed, 0, o[0], o[1], st)
                   : plume_aggregate_check(c, 1, 0, n, i[0], u64(i[1]), i[2], i[3], i[4], i[5], i[6], i[7], seed, o[0], o[1]);
    };
    add(std::move(e), family, "aggregate", n);
}
static void fam_sign(plume_ctx* gen, int family, size_t n, bool derived, bool sec1 = false) {
    const size_t P = sec1 ? 33 : 64;
    Plume b = plume_signed(gen, n, derived ? 2 : 1, 100 * family + (unsigned)n);
    Bytes aux = rnd(32 * n);
    size_t j = 0;
    for (size_t i : bad_list(n)) {                         // sk = 0, sk = n, r = 0, r = n: no scalars of the reference's type (the derived-nonce signer has no r: its keys alone)
        Bytes& which = (derived || j % 4 < 2) ? b.sk : b.r;
        if (j % 2 == 0) zero(which, 32 * i, 32); else put(which, 32 * i, kN, 32);
        j++;
    }
    Entry e;
    e.in = {b.msgs, b.off, b.sk, derived ? aux : b.r};
    e.out = {P * n, P * n, 32 * n, 32 * n, P * n, P * n, n};
    e.status = 6;
    e.redo = kArmedIfChecked;
    const int version = derived ? 2 : 1;
    e.call = [n, version, derived, sec1](plume_ctx* c, bool dev, hipStream_t st, uint8_t* const* i, uint8_t* const* o) {
        const size_t mb = (size_t)u64(i[1])[n] + 16;
        if (sec1) return dev ? plume_sign_batch_sec1_device(c, version, n, i[0], u64(i[1]), mb, i[2], i[3], nullptr, o[0], o[1], o[2], o[3], o[4], o[5], o[6], st)
                             : plume_sign_batch_sec1(c, version, n, i[0], u64(i[1]), i[2], i[3], nullptr, o[0], o[1], o[2], o[3], o[4], o[5], o[6]);
        if (derived) return dev ? plume_sign_batch_rfc6979_device(c, version, n, i[0], u64(i[1]), mb, i[2], i[3], nullptr, o[0], o[1], o[2], o[3], o[4], o[5], o[6], st)
                                : plume_sign_batch_rfc6979(c, version, n, i[0], u64(i[1]), i[2], i[3], nullptr, o[0], o[1], o[2], o[3], o[4], o[5], o[6]);
        return dev ? plume_sign_batch_device(c, version, n, i[0], u64(i[1]), mb, i[2], i[3], nullptr, o[0], o[1], o[2], o[3], o[4], o[5], o[6], st)
                   : plume_sign_batch(c, version, n, i[0], u64(i[1]), i[2], i[3], nullptr, o[0], o[1], o[2], o[3], o[4], o[5], o[6]);
    };
    add(std::move(e), family, sec1 ? "sign_sec1" : derived ? "sign_rfc6979" : "sign", n);
}
static void fam_eth_address(plume_ctx* gen, int family, size_t n) {
    Plume b = plume_signed(gen, n, 2, 100 * family + (unsigned)n);
    size_t j = 0;
    for (size_t i : bad_list(n)) { if (j++ % 2) zero(b.pk, 64 * i, 64); else b.pk[64 * i + 63] ^= 1; }     // the zero record, a point off the curve
    Entry e;
    e.in = {b.pk};
    e.out = {42 * n, n};
    e.status = 1;
    e.call = [n](plume_ctx* c, bool dev, hipStream_t st, uint8_t* const* i, uint8_t* const* o) {
        return dev ? plume_eth_address_batch_device(c, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_EIP55, n, i[0], nullptr, o[0], o[1], st)
                   : plume_eth_address_batch(c, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_EIP55, n, i[0], nullptr, o[0], o[1]);
    };
    add(std::move(e), family, "eth_address", n);
}
static void fam_ecdsa_recover(plume_ctx* gen, int family, size_t n) {
    g_gen.seed(100 * family + n);
    Bytes hash = rnd(32 * n), sk = scalars(n), r(32 * n), s(32 * n), v(n), status(n);
    REQUIRE(plume_ecdsa_sign_batch(gen, PLUME_ECDSA_SIGN_V27, n, hash.data(), sk.data(), nullptr, r.data(), s.data(), v.data(), status.data()) == 0 && all_of(status.data(), n, 0));
    size_t j = 0;
    for (size_t i : bad_list(n)) {                         // r = 0, s = n, a v that is none
        switch (j++ % 3) { case 0: zero(r, 32 * i, 32); break; case 1: put(s, 32 * i, kN, 32); break; default: v[i] = 5; }
    }
    Entry e;
    e.in = {hash, r, s, v};
    e.out = {33 * n, 64 * n, n};
    e.status = 2;
    e.redo = kEcdsa;
    e.call = [n](plume_ctx* c, bool dev, hipStream_t st, uint8_t* const* i, uint8_t* const* o) {
        return dev ? plume_ecdsa_recover_batch_device(c, 0, PLUME_ETH_PK_SEC1, PLUME_ETH_ADDR_RECORD64, n, i[0], i[1], i[2], i[3], nullptr, o[0], o[1], o[2], st)
                   : plume_ecdsa_recover_batch(c, 0, PLUME_ETH_PK_SEC1, PLUME_ETH_ADDR_RECORD64, n, i[0], i[1], i[2], i[3], nullptr, o[0], o[1], o[2]);
    };
    add(std::move(e), family, "ecdsa_recover", n);
}
static void fam_ecdsa_sign(int family, size_t n) {         // the digest of every ragged message, then its deterministic signature: the second call is fed by the first
    g_gen.seed(100 * family + n);
    std::vector<size_t> lens(n);
    for (size_t i = 0; i < n; i++) lens[i] = (size_t)(g_gen() % 300);
    Bytes off = offsets(lens), msgs = rnd((size_t)u64(off.data())[n] + 16), sk = scalars(n), aux = rnd(32 * n);
    size_t j = 0;
    for (size_t i : bad_list(n)) { if (j++ % 2) put(sk, 32 * i, kN, 32); else zero(sk, 32 * i, 32); }
    Entry e;
    e.in = {msgs, off, sk, aux};
    e.out = {32 * n, 32 * n, 32 * n, n, n};
    e.status = 4;
    e.redo = kEcdsaIfChecked;
    e.call = [n](plume_ctx* c, bool dev, hipStream_t st, uint8_t* const* i, uint8_t* const* o) {
        const size_t mb = (size_t)u64(i[1])[n] + 16;
        if (int rc = dev ? plume_eth_message_hash_batch_device(c, PLUME_ETH_HASH_EIP191, n, i[0], u64(i[1]), mb, o[0], st) : plume_eth_message_hash_batch(c, PLUME_ETH_HASH_EIP191, n, i[0], u64(i[1]), o[0]))
            return rc;
        return dev ? plume_ecdsa_sign_batch_device(c, PLUME_ECDSA_SIGN_V27, n, o[0], i[2], i[3], o[1], o[2], o[3], o[4], st)
                   : plume_ecdsa_sign_batch(c, PLUME_ECDSA_SIGN_V27, n, o[0], i[2], i[3], o[1], o[2], o[3], o[4]);
    };
    add(std::move(e), family, "ecdsa_sign", n);
}
// unsigned transactions of three kinds in turn: legacy unprotected (6 items), legacy EIP-155 (9 items ending chainId, 80, 80), type 2 (9 items behind the type byte)
static Bytes unsigned_tx(size_t i) {
    Bytes to = rnd(20), body;
    auto small = [&](uint8_t v) { body.push_back(v ? v : 0x80); };                 // an integer below 0x80 is its own encoding; zero is the empty string
    auto word = [&](uint32_t v) { body.push_back(0x84); for (int k = 3; k >= 0; k--) body.push_back((uint8_t)(v >> (8 * k))); };
    const int kind = (int)(i % 3);
    if (kind == 2) small(1);                               // chainId
    small((uint8_t)(1 + i % 100));                         // nonce
    word(0x77359400u + (uint32_t)i);                       // gas price / max priority fee
    if (kind == 2) word(0x7735A000u + (uint32_t)i);        // max fee
    body.push_back(0x82); body.push_back(0x52); body.push_back(0x08);              // gas 21000
    body.push_back(0x94); body.insert(body.end(), to.begin(), to.end());
    small((uint8_t)(i % 0x7F));                            // value
    const size_t dl = i % 9;                               // data: a short string
    if (dl == 1) body.push_back(0x05); else { body.push_back((uint8_t)(0x80 + dl)); for (size_t k = 0; k < dl; k++) body.push_back((uint8_t)(0x90 + k)); }
    if (kind == 2) body.push_back(0xC0);                   // an empty access list
    if (kind == 1) { small(1); small(0); small(0); }
    REQUIRE(body.size() < 56);
    Bytes tx;
    if (kind == 2) tx.push_back(0x02);
    tx.push_back((uint8_t)(0xC0 + body.size()));
    tx.insert(tx.end(), body.begin(), body.end());
    return tx;
}
static void pack(const std::vector<Bytes>& items, Bytes& txs, Bytes& off) {
    std::vector<size_t> lens;
    txs.clear();
    for (const Bytes& t : items) { lens.push_back(t.size()); txs.insert(txs.end(), t.begin(), t.end()); }
    off = offsets(lens);
    txs.resize(txs.size() + 16, 0);
}
static void fam_eth_tx_sign(int family, size_t n) {
    g_gen.seed(100 * family + n);
    std::vector<Bytes> items;
    for (size_t i = 0; i < n; i++) items.push_back(unsigned_tx(i));
    Bytes sk = scalars(n), aux = rnd(32 * n), txs, off;
    size_t j = 0;
    for (size_t i : bad_list(n)) {                         // ill-framed: a byte short, a byte long; and a key that is none
        switch (j++ % 3) { case 0: items[i].pop_back(); break; case 1: items[i].push_back(0); break; default: zero(sk, 32 * i, 32); }
    }
    pack(items, txs, off);
    const size_t nb = (size_t)u64(off.data())[n], ob = nb + PLUME_ETH_TX_SIGN_GROWTH * n;
    Entry e;
    e.in = {txs, off, sk, aux};
    e.out = {ob, 4 * n, 32 * n, 32 * n, 32 * n, n, 8 * n, n, n};
    e.status = 8;
    e.redo = kEcdsaIfChecked;
    e.call = [n, nb, ob](plume_ctx* c, bool dev, hipStream_t st, uint8_t* const* i, uint8_t* const* o) {
        return dev ? plume_eth_tx_sign_batch_device(c, 0, n, i[0], u64(i[1]), nb, i[2], i[3], o[0], ob, (uint32_t*)o[1], o[2], o[3], o[4], o[5], (uint64_t*)o[6], o[7], o[8], st)
                   : plume_eth_tx_sign_batch(c, 0, n, i[0], u64(i[1]), i[2], i[3], o[0], (uint32_t*)o[1], o[2], o[3], o[4], o[5], (uint64_t*)o[6], o[7], o[8]);
    };
    add(std::move(e), family, "eth_tx_sign", n);
}
static void fam_eth_tx_sender(plume_ctx* gen, int family, size_t n) {
    g_gen.seed(100 * family + n);
    std::vector<Bytes> items;
    for (size_t i = 0; i < n; i++) items.push_back(unsigned_tx(i + 1000));
    Bytes sk = scalars(n), txs, off;
    pack(items, txs, off);
    const size_t nb = (size_t)u64(off.data())[n];
    Bytes out(nb + PLUME_ETH_TX_SIGN_GROWTH * n), status(n);
    std::vector<uint32_t> len(n);
    REQUIRE(plume_eth_tx_sign_batch(gen, 0, n, txs.data(), u64(off.data()), sk.data(), nullptr, out.data(), len.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, status.data()) == 0);
    REQUIRE(all_of(status.data(), n, 0));
    std::vector<Bytes> raws;
    for (size_t i = 0; i < n; i++) {
        const size_t at = (size_t)u64(off.data())[i] + PLUME_ETH_TX_SIGN_GROWTH * i;
        raws.emplace_back(out.begin() + at, out.begin() + at + len[i]);
    }
    size_t j = 0;
    for (size_t i : bad_list(n)) { if (j++ % 2) raws[i].push_back(0); else raws[i].pop_back(); }            // ill-framed transactions
    pack(raws, txs, off);
    const size_t rb = (size_t)u64(off.data())[n];
    Entry e;
    e.in = {txs, off};
    e.out = {64 * n, 20 * n, 8 * n, n, n};
    e.status = 4;
    e.redo = kEcdsa;
    e.call = [n, rb](plume_ctx* c, bool dev, hipStream_t st, uint8_t* const* i, uint8_t* const* o) {
        return dev ? plume_eth_tx_sender_batch_device(c, PLUME_ECDSA_LOW_S, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, n, i[0], u64(i[1]), rb, nullptr, o[0], o[1], (uint64_t*)o[2], o[3], o[4], st)
                   : plume_eth_tx_sender_batch(c, PLUME_ECDSA_LOW_S, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, n, i[0], u64(i[1]), nullptr, o[0], o[1], (uint64_t*)o[2], o[3], o[4]);
    };
    add(std::move(e), family, "eth_tx_sender", n);
}
static void fam_hd(plume_ctx* gen, int family, size_t n) { // master nodes, private derivation over two levels, public derivation over two levels: three calls
    Plume b = plume_signed(gen, n, 2, 100 * family + (unsigned)n);     // (its sk and pk = sk G are the parents)
    Bytes seed = rnd(64 * n), chain = rnd(32 * n), psk = b.sk, ppk = b.pk;
    std::vector<uint32_t> path(2 * n), ppath(2 * n);
    for (size_t k = 0; k < 2 * n; k++) { path[k] = (uint32_t)g_gen(); ppath[k] = (uint32_t)g_gen() & 0x7FFFFFFFu; }
    size_t j = 0;
    for (size_t i : bad_list(n)) {                         // keys that are none; a record off the curve, a hardened index in a public derivation
        if (j % 2) { put(psk, 32 * i, kN, 32); ppath[2 * i + 1] |= 0x80000000u; } else { zero(psk, 32 * i, 32); ppk[64 * i + 63] ^= 1; }
        j++;
    }
    Entry e;
    e.in = {seed, psk, chain, Bytes((uint8_t*)path.data(), (uint8_t*)(path.data() + 2 * n)), ppk, Bytes((uint8_t*)ppath.data(), (uint8_t*)(ppath.data() + 2 * n))};
    e.out = {32 * n, 32 * n, n, 32 * n, 32 * n, 64 * n, 20 * n, n, 64 * n, 32 * n, 20 * n, n};
    e.status = 7;
    e.call = [n](plume_ctx* c, bool dev, hipStream_t st, uint8_t* const* i, uint8_t* const* o) {
        const int pf = PLUME_ETH_PK_AFFINE64, af = PLUME_ETH_ADDR_RAW20;
        if (int rc = dev ? plume_hd_master_batch_device(c, n, i[0], 64, o[0], o[1], o[2], st) : plume_hd_master_batch(c, n, i[0], 64, o[0], o[1], o[2])) return rc;
        if (int rc = dev ? plume_hd_derive_priv_batch_device(c, 0, pf, af, n, i[1], i[2], (const uint32_t*)i[3], 2, o[3], o[4], o[5], o[6], o[7], st)
                         : plume_hd_derive_priv_batch(c, 0, pf, af, n, i[1], i[2], (const uint32_t*)i[3], 2, o[3], o[4], o[5], o[6], o[7]))
            return rc;
        return dev ? plume_hd_derive_pub_batch_device(c, 0, pf, af, n, i[4], i[2], (const uint32_t*)i[5], 2, o[8], o[9], o[10], o[11], st)
                   : plume_hd_derive_pub_batch(c, 0, pf, af, n, i[4], i[2], (const uint32_t*)i[5], 2, o[8], o[9], o[10], o[11]);
    };
    add(std::move(e), family, "hd", n);
}
static void fam_kdf(int family, size_t n) {                // 3 iterations; the host form refuses unsound offsets as a whole, so only the device form is given them
    g_gen.seed(100 * family + n);
    static const size_t kLens[9] = {0, 1, 111, 112, 128, 129, 239, 240, 300};
    std::vector<size_t> lens(n);
    for (size_t i = 0; i < n; i++) lens[i] = kLens[i % 9];
    Bytes off = offsets(lens), pw = rnd((size_t)u64(off.data())[n]), salt = rnd(12 * n), doff = off;
    for (size_t i : bad_list(n)) { uint64_t* d = (uint64_t*)doff.data(); d[i + 1] = d[i] - 1; }             // the item's end in front of its start
    Entry e;
    e.in = {pw, off, salt};
    e.in_dev = {pw, doff, salt};
    e.out = {64 * n, n};
    e.status = 1;                                          // (of the device form: the host form is given no unsound item)
    const size_t pb = pw.size();
    e.call = [n, pb](plume_ctx* c, bool dev, hipStream_t st, uint8_t* const* i, uint8_t* const* o) {
        return dev ? plume_pbkdf2_sha512_batch_device(c, 0, n, i[0], u64(i[1]), pb, i[2], 12, 3, 64, o[0], o[1], st) : plume_pbkdf2_sha512_batch(c, 0, n, i[0], u64(i[1]), i[2], 12, 3, 64, o[0], o[1]);
    };
    add(std::move(e), family, "kdf", n);
}
static void fam_merkle(int family, size_t n) {             // leaves of address records, the tree, the proofs of every leaf, their check against the root: four calls
    g_gen.seed(100 * family + n);
    Bytes items(64 * n, 0), flip(1, 0);
    for (size_t i = 0; i < n; i++) { Bytes a = rnd(20); put(items, 64 * i + 44, a.data(), 20); }
    std::vector<uint32_t> extra(n, 0);                     // added to leaf_pos: an index outside the tree for every other planted item
    size_t j = 0;
    for (size_t i : bad_list(n)) { items[64 * i + j % 44] = (uint8_t)(1 + j); if (j % 2 == 0) extra[i] = (uint32_t)(2 * n + 5); j++; }
    const size_t depth = plume_merkle_max_proof_len(n);
    Entry e;
    e.in = {items, Bytes((uint8_t*)extra.data(), (uint8_t*)(extra.data() + n))};
    e.out = {32 * n, n, 32 * (2 * n - 1), 4 * n, 4 * n, 32 * depth * n, n, n};
    e.status = 1;
    // outputs: leaf, leaf status, tree, leaf_pos, pos (leaf_pos + extra: computed by the driver between the calls, on the host side of both forms), proof, proof_len, status
    e.call = [n, depth](plume_ctx* c, bool dev, hipStream_t st, uint8_t* const* i, uint8_t* const* o) {
        const int lf = PLUME_MERKLE_LEAF_ADDRESS, af = PLUME_ETH_ADDR_RECORD64;
        if (int rc = dev ? plume_merkle_leaf_batch_device(c, lf, af, n, i[0], nullptr, o[0], o[1], st) : plume_merkle_leaf_batch(c, lf, af, n, i[0], nullptr, o[0], o[1])) return rc;
        if (int rc = dev ? plume_merkle_tree_build_device(c, PLUME_MERKLE_SORT_LEAVES, n, o[0], o[2], (uint32_t*)o[3], st) : plume_merkle_tree_build(c, PLUME_MERKLE_SORT_LEAVES, n, o[0], o[2], (uint32_t*)o[3]))
            return rc;
        if (dev) REQUIRE((st ? hipStreamSynchronize(st) : hipDeviceSynchronize()) == hipSuccess);             // (the mock's device memory is host memory)
        for (size_t k = 0; k < n; k++) ((uint32_t*)o[4])[k] = ((const uint32_t*)o[3])[k] + ((const uint32_t*)i[1])[k];
        if (int rc = dev ? plume_merkle_proof_batch_device(c, n, o[2], n, (const uint32_t*)o[4], depth, o[5], o[6], st) : plume_merkle_proof_batch(c, n, o[2], n, (const uint32_t*)o[4], depth, o[5], o[6]))
            return rc;
        return dev ? plume_merkle_verify_batch_device(c, lf, af, n, i[0], nullptr, depth, o[5], o[6], o[2], o[7], st) : plume_merkle_verify_batch(c, lf, af, n, i[0], nullptr, depth, o[5], o[6], o[2], o[7]);
    };
    add(std::move(e), family, "merkle", n);
}
static void fam_dedup(int family, size_t n) {              // first occurrences among n records drawn from n / 3; the planted items are not live
    g_gen.seed(100 * family + n);
    const size_t pool = n / 3 > 2 ? n / 3 : 2;
    Bytes recs0 = rnd(64 * pool), recs(64 * n), live(n, 1);
    std::vector<uint64_t> ids(n);
    for (size_t i = 0; i < n; i++) { put(recs, 64 * i, recs0.data() + 64 * (g_gen() % pool), 64); ids[i] = ((uint64_t)1 << 40) + 3 * i; }
    for (size_t i : bad_list(n)) live[i] = 0;
    Entry e;
    e.in = {recs, live, Bytes((uint8_t*)ids.data(), (uint8_t*)(ids.data() + n))};
    e.out = {n, 8};
    e.status = 0; e.every = false;                         // (first: an item that is live in the other size may repeat an earlier record)
    e.call = [n](plume_ctx* c, bool dev, hipStream_t st, uint8_t* const* i, uint8_t* const* o) {
        return dev ? plume_nullifier_first_occurrence_device(c, n, i[0], i[1], u64(i[2]), o[0], (uint64_t*)o[1], st) : plume_nullifier_first_occurrence(c, n, i[0], i[1], u64(i[2]), o[0], (uint64_t*)o[1]);
    };
    add(std::move(e), family, "dedup", n);
}
static int g_families = 0;
static void build_entries() {
    plume_ctx* gen = nullptr;
    REQUIRE(plume_init(&gen, 0) == 0);
    for (size_t n : {kLarge, kSmall}) {
        int f = 0;
        g_what = "inputs of " + std::to_string(n) + " items";
        fam_verify(gen, f++, n, 1, 0); fam_verify(gen, f++, n, 2, 0); fam_verify(gen, f++, n, 1, 1); fam_recover(gen, f++, n); fam_aggregate(gen, f++, n);
        fam_sign(gen, f++, n, false); fam_sign(gen, f++, n, true); fam_eth_address(gen, f++, n); fam_ecdsa_recover(gen, f++, n); fam_ecdsa_sign(f++, n);
        fam_eth_tx_sender(gen, f++, n); fam_eth_tx_sign(f++, n); fam_hd(gen, f++, n); fam_kdf(f++, n); fam_merkle(f++, n); fam_dedup(f++, n);
        fam_verify_sec1(gen, f++, n); fam_sign(gen, f++, n, false, true);
        g_families = f;
    }
    plume_destroy(gen);
    // the references: each entry on a context that has done nothing else, in the host form and in the device form, over outputs pre-filled with two different bytes.  The
    // two give the same bytes (given other inputs, the device form is run with both fills): so every output byte was written, and the forms agree
    for (Entry& e : g_entries) {
        g_what = "reference of " + e.name;
        auto fresh = [&e](bool dev, uint8_t fill) {
            plume_ctx* ctx = nullptr;
            REQUIRE(plume_init(&ctx, 0) == 0);
            std::vector<Bytes> got;
            {
                Running r(ctx, e, dev, nullptr, 0, fill);
                r.wait();
                got = r.outputs();
            }
            plume_destroy(ctx);
            return got;
        };
        e.want = fresh(false, kFill);
        if (e.in_dev.empty()) REQUIRE(fresh(true, 0x55) == e.want);
        else { e.want_dev = fresh(true, kFill); REQUIRE(fresh(true, 0x55) == e.want_dev && fresh(false, 0x55) == e.want); }
    }
    // the planted items do what they are planted for: where one size plants an item and the other does not, the two sizes' status bytes differ -- at every such position,
    // or (Entry::every false) at some -- so a status byte the other size left behind is a wrong one
    const size_t half = g_entries.size() / 2;
    for (size_t k = 0; k < half; k++) {
        const Entry &big = g_entries[k], &small = g_entries[k + half];
        g_what = "planted items of " + big.name + " and " + small.name;
        REQUIRE(big.family == small.family && big.n == kLarge && small.n == kSmall && big.status >= 0 && big.status == small.status);
        const Bytes &sb = big.expected(true)[(size_t)big.status], &ss = small.expected(true)[(size_t)small.status];
        REQUIRE(sb.size() == kLarge && ss.size() == kSmall);
        size_t planted = 0, differ = 0;
        for (size_t i = 0; i < kSmall; i++) if (bad_at(kLarge, i) != bad_at(kSmall, i)) { planted++; if (sb[i] != ss[i]) differ++; }
        REQUIRE(planted >= 3 && (big.every ? differ == planted : differ >= 1));
    }
}

// ------------------------------------------------------------------------------------------------------------ the groups
struct Step {
    const Entry* e;
    bool dev = false;
    int stream = 0;                                        // 0 the context's own, 1 / 2 the caller's
    int selfcheck = -1, eq1 = -1, uniform = -1, timing = -1;   // -1: left as it is
    int host_kind = 0;
    std::string label() const { return e->name + " (" + (dev ? "device" : "host") + " form, stream " + std::to_string(stream) + ")"; }
};
struct Context {
    plume_ctx* ctx = nullptr;
    hipStream_t st[3] = {nullptr, nullptr, nullptr};
    bool device_forms = true, check_redo = true;
    int redo = kNone, selfcheck = 0;
    explicit Context(int devices = 1) {
        int ids[2] = {0, 1};
        REQUIRE((devices == 1 ? plume_init(&ctx, 0) : plume_init_multi(&ctx, ids, devices)) == 0);
        device_forms = devices == 1;
        for (int k = 1; k < 3; k++) REQUIRE(hipStreamCreateWithFlags(&st[k], hipStreamNonBlocking) == hipSuccess);
    }
    ~Context() { plume_destroy(ctx); for (int k = 1; k < 3; k++) (void)hipStreamDestroy(st[k]); }
};
[[noreturn]] static void mismatch(size_t index, const Step& s, const Step* prev, const std::string& what) {
    std::fprintf(stderr, "mixed_driver: seed %llu, call %zu: %s differs from the result of a context that has done nothing else, after %s: %s   [%s]\n", g_seed, index, s.label().c_str(),
                 prev ? prev->label().c_str() : "nothing", what.c_str(), g_what.c_str());
    std::exit(2);
}
static void run_steps(Context& c, const std::vector<Step>& steps) {
    const Step* prev = nullptr;
    for (size_t k = 0; k < steps.size(); k++) {
        const Step& s = steps[k];
        if (s.selfcheck >= 0) { REQUIRE(plume_set_sign_selfcheck(c.ctx, s.selfcheck) == 0); c.selfcheck = s.selfcheck; }
        if (s.eq1 >= 0) REQUIRE(plume_set_eq1_short(c.ctx, s.eq1) == 0);
        if (s.uniform >= 0) REQUIRE(plume_set_sign_uniform(c.ctx, s.uniform) == 0);
        if (s.timing >= 0) REQUIRE(plume_set_stage_timing(c.ctx, s.timing) == 0);
        const bool dev = s.dev && c.device_forms;
        {
            Running r(c.ctx, *s.e, dev, c.st[s.stream], s.host_kind);
            r.wait();
            const std::string d = r.differs(s.e->expected(dev));
            if (!d.empty()) mismatch(k, s, prev, d);
        }
        const int effect = s.e->redo == kArmedIfChecked ? (c.selfcheck ? (int)kArmedIfChecked : (int)kNone) : s.e->redo == kEcdsaIfChecked ? (c.selfcheck ? (int)kEcdsa : (int)kNone) : (int)s.e->redo;
        if (effect) c.redo = effect;
        if (c.check_redo && c.redo) {
            uint64_t count = 99;
            const int rc = plume_last_redo_tasks(c.ctx, &count);
            if (c.redo == kVerify && !(rc == 0 && count == 0)) mismatch(k, s, prev, "plume_last_redo_tasks gave " + std::to_string(rc) + " / " + std::to_string(count) + " behind a verify call (0 tasks expected)");
            if (c.redo == kArmedIfChecked && rc != 0) mismatch(k, s, prev, "plume_last_redo_tasks gave an error behind a self-checked sign call (its check is a verify call)");
            if (c.redo == kEcdsa && !(rc == PLUME_ERR_ARG && std::string(plume_last_error()).find("another family") != std::string::npos))
                mismatch(k, s, prev, "plume_last_redo_tasks gave " + std::to_string(rc) + " / " + std::to_string(count) + " behind an ECDSA-family call (PLUME_ERR_ARG expected: the list is not the verifier's)");
        }
        prev = &steps[k];
    }
}
static std::vector<Step> pair_steps() {
    std::vector<Step> steps;
    int k = 0;
    for (const Entry& a : g_entries)
        for (const Entry& b : g_entries)
            if (a.family != b.family || (a.n == kLarge && b.n == kSmall)) {
                for (const Entry* e : {&a, &b}) { Step s; s.e = e; s.dev = (k & 1) != 0; s.stream = k % 3; s.host_kind = (k / 2) & 1; steps.push_back(s); k++; }
            }
    return steps;
}
static std::vector<Step> walk_steps(size_t calls) {
    std::mt19937_64 w(g_seed * 7919 + 13);
    std::vector<Step> steps;
    static const int kEq1[3] = {0, 1, 3};
    for (size_t k = 0; k < calls; k++) {
        Step s;
        s.e = &g_entries[w() % g_entries.size()];
        s.dev = (w() & 1) != 0; s.stream = (int)(w() % 3); s.selfcheck = (int)(w() & 1); s.eq1 = kEq1[w() % 3]; s.uniform = (int)(w() % 3); s.timing = (int)(w() & 1); s.host_kind = (int)(w() & 1);
        steps.push_back(s);
    }
    return steps;
}

int main(int argc, char** argv) {
    g_seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
    const size_t calls = argc > 2 ? (size_t)std::strtoull(argv[2], nullptr, 10) : 300;
    const std::string groups = argc > 3 ? argv[3] : "abc";
    plume_ctx* keeper = nullptr;                           // holds the device's fixed tables for the whole run: they depend on nothing but G
    REQUIRE(plume_init(&keeper, 0) == 0);
    build_entries();
    REQUIRE(g_entries.size() == 2 * (size_t)g_families && g_families >= 13);
    if (groups.find('a') != std::string::npos) {
        g_what = "group a: every ordered pair of different families, large then small within a family";
        Context c;
        run_steps(c, pair_steps());
    }
    const std::vector<Step> walk = walk_steps(calls);
    if (groups.find('b') != std::string::npos) {
        g_what = "group b: the seeded walk";
        Context c;
        run_steps(c, walk);
    }
    if (groups.find('c') != std::string::npos) {
        {
            g_what = "group c: the walk on two devices";
            Context c(2);
            run_steps(c, walk);
        }
        {
            g_what = "group c: the walk with two batches in flight";
            Context c;
            c.check_redo = false;                          // (the hook reports the lane of the last device-resident call: which call that was is the lanes' business)
            REQUIRE(plume_set_in_flight(c.ctx, 2) == 0);
            run_steps(c, walk);
        }
        {
            g_what = "group c: the walk with host calls of three or more pieces";
            Context c;
            c.check_redo = false;                          // (... and of a host call's last piece)
            REQUIRE(plume_set_host_first_piece(c.ctx, 2) == 0 && plume_set_host_piece(c.ctx, 3) == 0 && plume_set_host_tail_piece(c.ctx, 2) == 0 && plume_set_chunk(c.ctx, 24) == 0);
            c.device_forms = false;                        // (the device form is one call of at most a chunk)
            run_steps(c, walk);
        }
    }
    plume_destroy(keeper);
    REQUIRE(mockhip::outstanding(0) == 0 && mockhip::outstanding(2) == 0 && mockhip::outstanding(3) == 0);
    std::printf("mixed_driver seed %llu: ok\n", g_seed);
    return 0;
}
