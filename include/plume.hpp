// plume.hpp — C++17 host side of the MI355X PLUME engine: the reference's Rust API, name for name, above the C ABI of plume_hip.h.
//
// The reference is Rust and this image has no Rust toolchain, so the host code a caller of `plume_rustcrypto` / `plume_arkworks` would
// switch to is written here in C++ (header-only, nothing but the standard library and libplume_hip.so).  Everything cryptographic --
// hash_to_curve, the scalar multiplications, the c-hash, s = r + sk*c -- runs in the HIP kernels behind plume_hip.h; this file marshals
// records into the ABI's structure-of-arrays form and reproduces the reference's types and error behaviour:
//
//   namespace plume_rustcrypto   rust-k256/src/lib.rs:43-156, rust-k256/src/randomizedsigner.rs:25-112
//       DST, AffinePoint, NonZeroScalar, SecretKey, PlumeSignature{message, pk, nullifier, c, s, v1specific}, PlumeSignatureV1Fields,
//       PlumeSignature::verify / sign_v1 / sign_v2, PlumeSigner{secret_key, v1}::try_sign_with_rng / sign_with_rng, hash_to_curve, encode_pt
//       + batch twins: verify_batch, sign_batch, sign_batch_with_nonces;  the steps either side: verify_batch_sec1 (33-byte SEC1 records), aggregate_check_v1,
//         nullifier_first_occurrence, scalars_to_sec1_der / scalar_from_sec1_der, circuit_h2c_inputs
//   namespace plume_arkworks     rust-arkworks/src/lib.rs:60-291, rust-arkworks/src/tests.rs:28-78,119-124
//       Affine, Fr, PlumeVersion, PlumeSignaturePublic / PlumeSignaturePrivate (zeroized on drop), sec1_affine, hash_to_curve, sign_with_r, sign,
//       keygen, verify_non_zk
//   namespace plume_hip          Engine (RAII over plume_ctx, one or several GPUs), Error, NullifierSet (the persistent nullifier set: insert / contains / export_all)
//
// Error behaviour:  the signer's `expect(..)` panics (randomizedsigner.rs:61,91,95) -> plume_rustcrypto::Panic;  `signature::Error`
// (randomizedsigner.rs:59) -> plume_rustcrypto::SignatureError;  `HashToCurveError` (rust-arkworks/src/lib.rs:99-101) ->
// plume_arkworks::HashToCurveError;  a failing library call -> plume_hip::Error.  There is no CPU fallback: without a gfx950 device
// Engine's constructor throws plume_hip::Error with code PLUME_ERR_NODEV.
//
// What the Rust types guarantee by construction and this header checks on the host: scalars in [1, n-1] (NonZeroScalar, SecretKey), Fr
// reduced mod n.  What it leaves to the engine: a k256::AffinePoint can only hold a point of the curve; AffinePoint here holds 64 bytes and the
// kernels validate them (an off-curve point makes verify() false and the signer report PLUME_STATUS_BAD_SCALAR).
//
// A single sign / verify is a batch of one (a kernel launch per call: use the batch twins for throughput).
#ifndef PLUME_HPP
#define PLUME_HPP
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "plume_hip.h"

namespace plume_hip {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};
// the signer's self-check (Engine::set_sign_selfcheck(1)) withheld a signature: the signer called it good (status 0) but its records do not verify -- a pk that is not
// sk G handed to sign_with_r, or a computation gone wrong.  Its own class: the reference has no such error, it releases the signature.
struct SelfCheckError : std::runtime_error { using std::runtime_error::runtime_error; };
inline void check(int rc, const char* call) {
    if (rc != PLUME_OK) throw Error(rc, std::string(call) + ": " + plume_last_error());
}

// One context: a single GPU (plume_init) or several (plume_init_multi: the host-pointer calls shard every batch evenly over the devices,
// SURVEY.md §8e).  Used by one host thread at a time; distinct engines are independent.
class Engine {
  public:
    explicit Engine(int device = 0) { check(plume_init(&ctx_, device), "plume_init"); }
    explicit Engine(const std::vector<int>& devices) { check(plume_init_multi(&ctx_, devices.data(), (int)devices.size()), "plume_init_multi"); }
    ~Engine() { if (ctx_) plume_destroy(ctx_); }
    Engine(const Engine&) = delete;
    Engine& operator=(const Engine&) = delete;
    Engine(Engine&& o) noexcept : ctx_(o.ctx_) { o.ctx_ = nullptr; }
    plume_ctx* ctx() const { return ctx_; }
    int num_shards() const { return plume_num_shards(ctx_); }
    // The signer's schedule (plume_hip.h, plume_set_sign_uniform): 0 = fastest (its instruction trace and table addresses depend on sk and r), 1 = no branch on a digit of
    // them, 2 = and no table address derived from one -- the property k256's constant-time multiplication has (rust-k256/src/randomizedsigner.rs:51-70 multiplies by secrets).
    void set_sign_uniform(int level) { check(plume_set_sign_uniform(ctx_, level), "plume_set_sign_uniform"); }
    int sign_uniform() const { const int l = plume_get_sign_uniform(ctx_); check(l < 0 ? l : 0, "plume_get_sign_uniform"); return l; }   // 1 by default (library 0.4)
    // The signer's self-check (plume_hip.h, plume_set_sign_selfcheck): 1 = every sign call verifies its own records on the GPU before anything reaches the caller's arrays;
    // a signature that does not verify is withheld and the façades throw SelfCheckError.  0 (the default) = off.
    void set_sign_selfcheck(int mode) { check(plume_set_sign_selfcheck(ctx_, mode), "plume_set_sign_selfcheck"); }
    int sign_selfcheck() const { const int m = plume_get_sign_selfcheck(ctx_); check(m < 0 ? m : 0, "plume_get_sign_selfcheck"); return m; }
    void set_stage_timing(bool on) { check(plume_set_stage_timing(ctx_, on ? 1 : 0), "plume_set_stage_timing"); }   // off by default (library 0.5): needed before last_stage_times
    void set_host_lanes(int lanes) { check(plume_set_host_lanes(ctx_, lanes), "plume_set_host_lanes"); }
    void set_eq1_short(int mode) { check(plume_set_eq1_short(ctx_, mode), "plume_set_eq1_short"); }   // the verifier's first equation where R is given (plume_hip.h): 1 short for large calls (default), 3 short always, 0 long, 2 test
    int eq1_short(size_t* min_items = nullptr) const { const int m = plume_get_eq1_short(ctx_, min_items); check(m < 0 ? m : 0, "plume_get_eq1_short"); return m; }
    const char* last_msm_kernel() const { return plume_last_msm_kernel(ctx_); }                       // measurement hook: the multi-scalar kernel the last verify call launched
    // the engine single-item calls use when none is passed: PLUME_DEVICES="0,1,.." (one multi-device context) or device 0
    static Engine& shared() {
        static std::unique_ptr<Engine> e;
        if (!e) {
            const char* env = std::getenv("PLUME_DEVICES");
            std::vector<int> ids;
            for (const char* p = env; p && *p;) { char* end; long v = std::strtol(p, &end, 10); if (end == p) break; ids.push_back((int)v); p = (*end == ',') ? end + 1 : end; }
            e.reset(ids.size() > 1 ? new Engine(ids) : new Engine(ids.empty() ? 0 : ids[0]));
        }
        return *e;
    }

  private:
    plume_ctx* ctx_ = nullptr;
};

using Bytes = std::vector<uint8_t>;
using Bytes32 = std::array<uint8_t, 32>;
using Bytes64 = std::array<uint8_t, 64>;

// packed messages + (n+1) offsets, the ABI's message form
struct PackedMessages {
    Bytes bytes;
    std::vector<uint64_t> off{0};
    void push(const uint8_t* m, size_t len) { bytes.insert(bytes.end(), m, m + len); off.push_back(bytes.size()); }
    const uint8_t* data() const { static const uint8_t none = 0; return bytes.empty() ? &none : bytes.data(); }
};

// the order of the scalar field (rust-arkworks/src/secp256k1/fields/fr.rs:19), big-endian
inline const Bytes32& order_n() {
    static const Bytes32 n = {0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFE,
                              0xBA, 0xAE, 0xDC, 0xE6, 0xAF, 0x48, 0xA0, 0x3B, 0xBF, 0xD2, 0x5E, 0x8C, 0xD0, 0x36, 0x41, 0x41};
    return n;
}
inline bool is_zero32(const Bytes32& b) { for (uint8_t v : b) if (v) return false; return true; }
inline bool below_n(const Bytes32& b) { return std::memcmp(b.data(), order_n().data(), 32) < 0; }
// big-endian bytes of any length, reduced mod n (Fr::from_be_bytes_mod_order): schoolbook, one byte at a time -- marshalling only, never on a hot path
inline Bytes32 reduce_mod_n(const uint8_t* be, size_t len) {
    // r = (r * 256 + byte) mod n on 5 x 64-bit limbs (r < n < 2^256, so r * 256 + byte < 2^264)
    const Bytes32& nb = order_n();
    uint64_t n[4], r[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++) { n[i] = 0; for (int j = 0; j < 8; j++) n[i] = (n[i] << 8) | nb[(size_t)(24 - 8 * i + j)]; }
    for (size_t k = 0; k < len; k++) {
        for (int i = 4; i > 0; i--) r[i] = (r[i] << 8) | (r[i - 1] >> 56);
        r[0] = (r[0] << 8) | be[k];
        // r < 2^264 = 256 * 2^256 < 257 n: subtract n * 2^j for j = 8..0 while it fits
        for (int j = 8; j >= 0; j--) {
            uint64_t m[5] = {0, 0, 0, 0, 0};
            for (int i = 0; i < 4; i++) { m[i] |= n[i] << j; if (j) m[i + 1] |= n[i] >> (64 - j); }
            bool ge = true;
            for (int i = 4; i >= 0; i--) if (r[i] != m[i]) { ge = r[i] > m[i]; break; }
            if (ge) { unsigned __int128 bw = 0; for (int i = 0; i < 5; i++) { unsigned __int128 d = (unsigned __int128)r[i] - m[i] - (uint64_t)bw; r[i] = (uint64_t)d; bw = (d >> 64) & 1; } }
        }
    }
    Bytes32 out;
    for (int i = 0; i < 4; i++) for (int j = 0; j < 8; j++) out[(size_t)(24 - 8 * i + j)] = (uint8_t)(r[i] >> (56 - 8 * j));
    return out;
}

inline Bytes from_hex(const std::string& h) {
    Bytes b(h.size() / 2);
    auto nib = [](char c) -> int { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; };
    for (size_t i = 0; i < b.size(); i++) {
        const int hi = nib(h[2 * i]), lo = nib(h[2 * i + 1]);
        if (hi < 0 || lo < 0) throw std::invalid_argument("not a hex string");
        b[i] = (uint8_t)(hi * 16 + lo);
    }
    return b;
}
inline std::string to_hex(const uint8_t* b, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s(2 * n, '0');
    for (size_t i = 0; i < n; i++) { s[2 * i] = d[b[i] >> 4]; s[2 * i + 1] = d[b[i] & 15]; }
    return s;
}

}  // namespace plume_hip

// ============================================================================================== plume_rustcrypto shape
namespace plume_rustcrypto {
using plume_hip::Bytes;
using plume_hip::Bytes32;
using plume_hip::Bytes64;
using plume_hip::Engine;

// rust-k256/src/lib.rs:61
inline const std::string DST = "QUUX-V01-CS02-with-secp256k1_XMD:SHA-256_SSWU_RO_";

struct Panic : std::logic_error { using std::logic_error::logic_error; };             // the reference's expect(..) panics
struct SignatureError : std::runtime_error { SignatureError() : std::runtime_error("signature error") {} };   // signature::Error

// k256::AffinePoint as the ABI carries it: x || y big-endian, all-zero = the identity
struct AffinePoint {
    Bytes64 xy{};
    static AffinePoint IDENTITY() { return AffinePoint{}; }
    static AffinePoint GENERATOR() {   // rust-arkworks/src/secp256k1/curves/mod.rs:52-58
        return from_hex("79be667ef9dcbbac55a06295ce870b07029bfcdb2dce28d959f2815b16f81798", "483ada7726a3c4655da4fbfc0e1108a8fd17b448a68554199c47d08ffb10d4b8");
    }
    static AffinePoint from_bytes64(const uint8_t* b) { AffinePoint p; std::memcpy(p.xy.data(), b, 64); return p; }
    static AffinePoint from_hex(const std::string& x, const std::string& y) {
        const Bytes bx = plume_hip::from_hex(x), by = plume_hip::from_hex(y);
        if (bx.size() != 32 || by.size() != 32) throw std::invalid_argument("coordinates are 32 bytes each");
        AffinePoint p; std::memcpy(p.xy.data(), bx.data(), 32); std::memcpy(p.xy.data() + 32, by.data(), 32); return p;
    }
    bool is_identity() const { for (uint8_t v : xy) if (v) return false; return true; }
    Bytes32 x() const { Bytes32 r; std::memcpy(r.data(), xy.data(), 32); return r; }
    Bytes32 y() const { Bytes32 r; std::memcpy(r.data(), xy.data() + 32, 32); return r; }
    // ToEncodedPoint::to_encoded_point (SEC1): identity = the single byte 00 (rust-k256/src/utils.rs:23-25, rust-arkworks/src/tests/test_vectors.rs:3-7)
    Bytes to_encoded_point(bool compress) const {
        if (is_identity()) return Bytes{0};
        Bytes out;
        if (compress) { out.push_back((uint8_t)(2 + (xy[63] & 1))); out.insert(out.end(), xy.begin(), xy.begin() + 32); }
        else { out.push_back(4); out.insert(out.end(), xy.begin(), xy.end()); }
        return out;
    }
    bool operator==(const AffinePoint& o) const { return xy == o.xy; }
    bool operator!=(const AffinePoint& o) const { return !(*this == o); }
};
// encode_pt (rust-k256/src/utils.rs:23-25)
inline Bytes encode_pt(const AffinePoint& p) { return p.to_encoded_point(true); }

// k256::NonZeroScalar: an integer of [1, n-1], 32 bytes big-endian
class NonZeroScalar {
  public:
    // NonZeroScalar::from_repr: None for 0 and for values >= n
    static std::optional<NonZeroScalar> from_repr(const Bytes32& b) {
        if (plume_hip::is_zero32(b) || !plume_hip::below_n(b)) return std::nullopt;
        return NonZeroScalar(b);
    }
    static std::optional<NonZeroScalar> from_repr(const Bytes& b) { Bytes32 a; if (b.size() != 32) return std::nullopt; std::memcpy(a.data(), b.data(), 32); return from_repr(a); }
    static std::optional<NonZeroScalar> from_hex(const std::string& h) { return from_repr(plume_hip::from_hex(h)); }
    const Bytes32& to_bytes() const { return v_; }
    std::string to_string() const { return plume_hip::to_hex(v_.data(), 32); }
    bool operator==(const NonZeroScalar& o) const { return v_ == o.v_; }
    bool operator!=(const NonZeroScalar& o) const { return v_ != o.v_; }

  protected:
    explicit NonZeroScalar(const Bytes32& b) : v_(b) {}
    Bytes32 v_;
};

// k256::SecretKey: zeroized when dropped, like the reference's
class SecretKey : public NonZeroScalar {
  public:
    // SecretKey::from_bytes / from_slice: Err for 0 and values >= n
    static std::optional<SecretKey> from_bytes(const Bytes32& b) { auto s = NonZeroScalar::from_repr(b); if (!s) return std::nullopt; return SecretKey(b); }
    static std::optional<SecretKey> from_bytes(const Bytes& b) { Bytes32 a; if (b.size() != 32) return std::nullopt; std::memcpy(a.data(), b.data(), 32); return from_bytes(a); }
    static std::optional<SecretKey> from_hex(const std::string& h) { return from_bytes(plume_hip::from_hex(h)); }
    // SecretKey::random: 32 bytes from the RNG, big-endian, rejection-sampled (pinned by the mock RNG of rust-k256/tests/signing.rs:23-44)
    template <class Rng>
    static SecretKey random(Rng& rng) {
        for (;;) {
            Bytes32 b;
            rng.fill_bytes(b.data(), b.size());
            if (auto k = from_bytes(b)) { volatile uint8_t* w = b.data(); for (size_t i = 0; i < 32; i++) w[i] = 0; return *k; }
        }
    }
    const NonZeroScalar& to_nonzero_scalar() const { return *this; }
    // SecretKey::public_key: sk * G on the GPU (the signer's comb)
    AffinePoint public_key(Engine& eng = Engine::shared()) const {
        uint8_t der[109], st = 0;
        plume_hip::check(plume_scalars_to_sec1_der_batch(eng.ctx(), 1, v_.data(), der, &st), "plume_scalars_to_sec1_der_batch");
        if (st) throw Panic("secret key outside [1, n-1]");
        return AffinePoint::from_bytes64(der + 45);   // 30 6b 02 01 01 04 20 <32> a1 44 03 42 00 04 <x> <y>
    }
    ~SecretKey() { volatile uint8_t* w = v_.data(); for (size_t i = 0; i < 32; i++) w[i] = 0; }
    SecretKey(const SecretKey&) = default;
    SecretKey& operator=(const SecretKey&) = default;

  private:
    explicit SecretKey(const Bytes32& b) : NonZeroScalar(b) {}
};

// rust-k256/src/lib.rs:84-89
struct PlumeSignatureV1Fields {
    AffinePoint r_point;
    AffinePoint hashed_to_curve_r;
};

class PlumeSigner;

// rust-k256/src/lib.rs:67-80
struct PlumeSignature {
    Bytes message;
    AffinePoint pk;
    AffinePoint nullifier;
    NonZeroScalar c;
    NonZeroScalar s;
    std::optional<PlumeSignatureV1Fields> v1specific;

    // PlumeSignature::verify (rust-k256/src/lib.rs:93-145)
    bool verify(Engine& eng = Engine::shared()) const;
    // The V1-specific fields that pk, nullifier, c, s imply -- r_point = s G - c pk, hashed_to_curve_r = s H - c nullifier, recomputed on the GPU
    // (plume_hip.h plume_recover_batch) -- for a c that is the V1 hash of them: upgrades a compact four-field record to a V1 record.  Throws SignatureError when an
    // input is no value of the reference's types and when c is NOT that hash (a V2 signature, a forgery): never a silent pair of points that do not verify.
    PlumeSignatureV1Fields recover_v1specific(Engine& eng = Engine::shared()) const;
    // The Ethereum address of pk, Keccak-256(x || y)[12..32), computed on the GPU (plume_hip.h plume_eth_address_batch): 20 raw bytes, and "0x" + 40 hex digits with
    // the EIP-55 mixed-case checksum.  Both throw SignatureError when pk is no Ethereum key: off the curve, a coordinate not below p, or the identity, which verify()
    // accepts but which has no address.  verify_for_address = verify() AND "pk is the key of addr20"; false for a pk that has no address.
    std::array<uint8_t, 20> eth_address(Engine& eng = Engine::shared()) const;
    std::string eth_address_eip55(Engine& eng = Engine::shared()) const;
    bool verify_for_address(const std::array<uint8_t, 20>& addr20, Engine& eng = Engine::shared()) const;
    // verify() AND "pk's address is on the allow-list whose Merkle root is root32" (plume_hip.h plume_merkle_verify_batch): pk -> address -> leaf -> proof, for a consumer
    // that holds one 32-byte root of OpenZeppelin's StandardMerkleTree of ["address"] -- or of ["address", "uint256"] when amount (32 big-endian bytes) is given -- and
    // takes a proof from every claimant.  proof: the siblings, leaf side first.  false for a pk that has no address.
    bool verify_for_root(const Bytes32& root32, const std::vector<Bytes32>& proof, const Bytes32* amount = nullptr, Engine& eng = Engine::shared()) const;
    // rust-k256/src/lib.rs:149-156
    template <class Rng> static PlumeSignature sign_v1(const SecretKey& secret_key, const Bytes& msg, Rng& rng, Engine& eng = Engine::shared());
    template <class Rng> static PlumeSignature sign_v2(const SecretKey& secret_key, const Bytes& msg, Rng& rng, Engine& eng = Engine::shared());
};

// batch twin of verify(): ok[i] == sigs[i].verify().  V1 and V2 signatures may be mixed (two calls into the library).
inline std::vector<bool> verify_batch(const std::vector<PlumeSignature>& sigs, Engine& eng = Engine::shared()) {
    std::vector<bool> out(sigs.size(), false);
    for (int ver = 1; ver <= 2; ver++) {
        plume_hip::PackedMessages m;
        Bytes pk, nul, c, s, rp, hr;
        std::vector<size_t> idx;
        for (size_t i = 0; i < sigs.size(); i++) {
            const PlumeSignature& g = sigs[i];
            if ((ver == 1) != g.v1specific.has_value()) continue;
            idx.push_back(i);
            m.push(g.message.data(), g.message.size());
            pk.insert(pk.end(), g.pk.xy.begin(), g.pk.xy.end());
            nul.insert(nul.end(), g.nullifier.xy.begin(), g.nullifier.xy.end());
            c.insert(c.end(), g.c.to_bytes().begin(), g.c.to_bytes().end());
            s.insert(s.end(), g.s.to_bytes().begin(), g.s.to_bytes().end());
            if (ver == 1) {
                rp.insert(rp.end(), g.v1specific->r_point.xy.begin(), g.v1specific->r_point.xy.end());
                hr.insert(hr.end(), g.v1specific->hashed_to_curve_r.xy.begin(), g.v1specific->hashed_to_curve_r.xy.end());
            }
        }
        if (idx.empty()) continue;
        Bytes ok(idx.size());
        plume_hip::check(plume_verify_batch(eng.ctx(), ver, idx.size(), m.data(), m.off.data(), pk.data(), nul.data(), c.data(), s.data(),
                                            ver == 1 ? rp.data() : nullptr, ver == 1 ? hr.data() : nullptr, ok.data()), "plume_verify_batch");
        for (size_t k = 0; k < idx.size(); k++) out[idx[k]] = ok[k] == 1;
    }
    return out;
}
inline bool PlumeSignature::verify(Engine& eng) const { return verify_batch(std::vector<PlumeSignature>{*this}, eng)[0]; }
inline PlumeSignatureV1Fields PlumeSignature::recover_v1specific(Engine& eng) const {
    plume_hip::PackedMessages m;
    m.push(message.data(), message.size());
    uint8_t rp[64], hr[64], st = 0xFF;
    plume_hip::check(plume_recover_batch(eng.ctx(), 1, PLUME_RECOVER_FMT_AFFINE64, 1, m.data(), m.off.data(), pk.xy.data(), nullifier.xy.data(), c.to_bytes().data(),
                                         s.to_bytes().data(), rp, hr, nullptr, &st), "plume_recover_batch");
    if (st != PLUME_RECOVER_MATCH) throw SignatureError();          // PLUME_RECOVER_INVALID, or a c that is not the V1 hash of the recovered points
    return PlumeSignatureV1Fields{AffinePoint::from_bytes64(rp), AffinePoint::from_bytes64(hr)};
}
inline std::array<uint8_t, 20> PlumeSignature::eth_address(Engine& eng) const {
    std::array<uint8_t, 20> out{};
    uint8_t st = 0xFF;
    plume_hip::check(plume_eth_address_batch(eng.ctx(), PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, 1, pk.xy.data(), nullptr, out.data(), &st), "plume_eth_address_batch");
    if (st == PLUME_ETH_INVALID) throw SignatureError();
    return out;
}
inline std::string PlumeSignature::eth_address_eip55(Engine& eng) const {
    char out[42];
    uint8_t st = 0xFF;
    plume_hip::check(plume_eth_address_batch(eng.ctx(), PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_EIP55, 1, pk.xy.data(), nullptr, reinterpret_cast<uint8_t*>(out), &st),
                     "plume_eth_address_batch");
    if (st == PLUME_ETH_INVALID) throw SignatureError();
    return std::string(out, 42);
}
inline bool PlumeSignature::verify_for_address(const std::array<uint8_t, 20>& addr20, Engine& eng) const {
    uint8_t st = 0xFF;
    plume_hip::check(plume_eth_address_batch(eng.ctx(), PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, 1, pk.xy.data(), addr20.data(), nullptr, &st), "plume_eth_address_batch");
    return st == PLUME_ETH_MATCH && verify(eng);
}

// The public key and the 20-byte Ethereum address behind one ECDSA signature over the 32-byte digest hash32, recovered on the GPU (plume_hip.h
// plume_ecdsa_recover_batch: Ethereum's ecrecover).  r, s: 32 big-endian bytes; v: 0, 1, 27 or 28.  Both throw SignatureError when the library rejects the item: v, r or
// s out of range, no curve point with x = r, or a key that comes out as the identity.  ecdsa_recover_address is for callers that want the 20 bytes only.
inline std::pair<AffinePoint, std::array<uint8_t, 20>> ecdsa_recover(const Bytes32& hash32, const Bytes32& r, const Bytes32& s, uint8_t v, Engine& eng = Engine::shared()) {
    uint8_t pk[64], st = 0xFF;
    std::array<uint8_t, 20> addr{};
    plume_hip::check(plume_ecdsa_recover_batch(eng.ctx(), 0, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, 1, hash32.data(), r.data(), s.data(), &v, nullptr, pk, addr.data(), &st),
                     "plume_ecdsa_recover_batch");
    if (st == PLUME_ECDSA_INVALID) throw SignatureError();
    return {AffinePoint::from_bytes64(pk), addr};
}
inline std::array<uint8_t, 20> ecdsa_recover_address(const Bytes32& hash32, const Bytes32& r, const Bytes32& s, uint8_t v, Engine& eng = Engine::shared()) {
    uint8_t st = 0xFF;
    std::array<uint8_t, 20> addr{};
    plume_hip::check(plume_ecdsa_recover_batch(eng.ctx(), 0, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, 1, hash32.data(), r.data(), s.data(), &v, nullptr, nullptr, addr.data(), &st),
                     "plume_ecdsa_recover_batch");
    if (st == PLUME_ECDSA_INVALID) throw SignatureError();
    return addr;
}

// A deterministic ECDSA signature by sk over the 32-byte digest hash32, made on the GPU (plume_hip.h plume_ecdsa_sign_batch): the RFC 6979 nonce over the digest itself --
// byte-identical to geth, ethers and libsecp256k1 -- hedged with the 32 bytes of aux when given; always low s; v 0 / 1, or 27 / 28 with v27.  Throws SignatureError when the
// outcome is degenerate (status 2 / 4: a SecretKey is always in range), plume_hip::SelfCheckError when the self-check withheld the signature.
struct EcdsaSignature {
    Bytes32 r{}, s{};
    uint8_t v = 0;
};
inline EcdsaSignature ecdsa_sign(const SecretKey& sk, const Bytes32& hash32, const Bytes32* aux = nullptr, Engine& eng = Engine::shared(), bool v27 = false) {
    EcdsaSignature sig;
    uint8_t st = 0xFF;
    plume_hip::check(plume_ecdsa_sign_batch(eng.ctx(), v27 ? PLUME_ECDSA_SIGN_V27 : 0, 1, hash32.data(), sk.to_bytes().data(), aux ? aux->data() : nullptr, sig.r.data(), sig.s.data(),
                                            &sig.v, &st),
                     "plume_ecdsa_sign_batch");
    if (st & PLUME_STATUS_SELFCHECK_FAILED) throw plume_hip::SelfCheckError("the signature does not recover the signer's key and was withheld (plume_set_sign_selfcheck)");
    if (st) throw SignatureError();
    return sig;
}
// The EIP-191 digest of msg, Keccak-256("\x19Ethereum Signed Message:\n" || decimal(len) || msg), on the GPU (plume_eth_message_hash_batch)
inline Bytes32 eth_message_hash(const uint8_t* msg, size_t len, Engine& eng = Engine::shared(), int mode = PLUME_ETH_HASH_EIP191) {
    const uint64_t off[2] = {0, (uint64_t)len};
    Bytes32 h{};
    plume_hip::check(plume_eth_message_hash_batch(eng.ctx(), mode, 1, msg, off, h.data()), "plume_eth_message_hash_batch");
    return h;
}
// A wallet's personal_sign: the 65 bytes r || s || v (v = 27 / 28) of ecdsa_sign over the EIP-191 digest of msg
inline std::array<uint8_t, 65> personal_sign(const SecretKey& sk, const uint8_t* msg, size_t len, const Bytes32* aux = nullptr, Engine& eng = Engine::shared()) {
    const EcdsaSignature sig = ecdsa_sign(sk, eth_message_hash(msg, len, eng), aux, eng, true);
    std::array<uint8_t, 65> out{};
    std::copy(sig.r.begin(), sig.r.end(), out.begin());
    std::copy(sig.s.begin(), sig.s.end(), out.begin() + 32);
    out[64] = sig.v;
    return out;
}
// The public key and the address that personal_sign'ed msg: the EIP-191 digest, then ecdsa_recover
inline std::pair<AffinePoint, std::array<uint8_t, 20>> personal_recover(const uint8_t* msg, size_t len, const std::array<uint8_t, 65>& sig65, Engine& eng = Engine::shared()) {
    Bytes32 r{}, s{};
    std::copy(sig65.begin(), sig65.begin() + 32, r.begin());
    std::copy(sig65.begin() + 32, sig65.begin() + 64, s.begin());
    return ecdsa_recover(eth_message_hash(msg, len, eng), r, s, sig65[64], eng);
}

// The senders of raw signed transactions (plume_hip.h plume_eth_tx_parse_batch / plume_eth_tx_sender_batch): legacy (unprotected or EIP-155) and the typed envelopes 01 - 04,
// framed, hashed and recovered on the GPU.  A sender recovery, not a consensus decoder: inner fields are not validated.  tx_signing_hash gives the 32 bytes the sender signed
// and throws SignatureError for an item that is no such transaction; tx_sender gives the public key and the 20-byte address (low_s: the EIP-2 rule, right for everything
// after Homestead) and throws SignatureError when there is no sender -- the framing is broken or the signature recovers no key; tx_sender_address is for callers that want
// the 20 bytes only.
inline Bytes32 tx_signing_hash(const uint8_t* raw, size_t len, Engine& eng = Engine::shared()) {
    const uint64_t off[2] = {0, (uint64_t)len};
    Bytes32 h{}, r{}, s{};
    uint8_t v = 0, st = 0xFF;
    plume_hip::check(plume_eth_tx_parse_batch(eng.ctx(), 1, raw, off, h.data(), r.data(), s.data(), &v, nullptr, nullptr, &st), "plume_eth_tx_parse_batch");
    if (st != PLUME_ETH_TX_OK) throw SignatureError();
    return h;
}
// The signed raw transaction of one UNSIGNED serialization -- exactly the bytes whose Keccak-256 the sender signs --, framed, hashed, signed and assembled on the GPU
// (plume_hip.h plume_eth_tx_sign_batch): legacy with 6 items (unprotected) or 9 (EIP-155: chainId, then two empty strings), or a typed envelope 01 - 04 without its last three
// fields.  The signature is ecdsa_sign's over that hash, hedged with aux when given.  Throws SignatureError for an item that is no such payload (as tx_signing_hash does for a
// bad item) and for a degenerate outcome, plume_hip::SelfCheckError when the self-check withheld the signature.  tx_sender of the result is the key's address.
inline std::vector<uint8_t> sign_tx(const SecretKey& sk, const uint8_t* unsigned_tx, size_t len, const Bytes32* aux = nullptr, Engine& eng = Engine::shared()) {
    const uint64_t off[2] = {0, (uint64_t)len};
    std::vector<uint8_t> out(plume_eth_tx_sign_out_bytes(1, len));
    uint32_t out_len = 0;
    uint8_t st = 0xFF;
    plume_hip::check(plume_eth_tx_sign_batch(eng.ctx(), 0, 1, unsigned_tx, off, sk.to_bytes().data(), aux ? aux->data() : nullptr, out.data(), &out_len, nullptr, nullptr, nullptr,
                                             nullptr, nullptr, nullptr, &st),
                     "plume_eth_tx_sign_batch");
    if (st & PLUME_STATUS_BAD_TX) throw SignatureError();
    if (st & PLUME_STATUS_SELFCHECK_FAILED) throw plume_hip::SelfCheckError("the signature does not recover the signer's key and was withheld (plume_set_sign_selfcheck)");
    if (st) throw SignatureError();
    out.resize(out_len);
    return out;
}
// ---- BIP-32 (plume_hip.h, library 0.17): the single-item forms.  A node is (key, chain code); every derivation runs on the GPU.
struct HdNode { SecretKey sk; Bytes32 chain; };
struct HdPubNode { AffinePoint pk; Bytes32 chain; };
// The indices of "m/44'/60'/0'/0/3" or, relative to a node, "0/3": decimal components below 2^31, a trailing ' or h adds 2^31 (hardened); 1 .. PLUME_HD_MAX_DEPTH of them.
// std::invalid_argument for "m", "m/", an empty component, anything else that is no index, too many components.
inline std::vector<uint32_t> parse_path(const std::string& path) {
    std::vector<uint32_t> out;
    size_t pos = 0;
    if (path == "m" || path.empty()) throw std::invalid_argument("parse_path: no component");
    if (path.compare(0, 2, "m/") == 0) pos = 2;
    for (;;) {
        const size_t end = std::min(path.find('/', pos), path.size());
        std::string c = path.substr(pos, end - pos);
        const bool hard = !c.empty() && (c.back() == '\'' || c.back() == 'h');
        if (hard) c.pop_back();
        if (c.empty() || c.size() > 10 || c.find_first_not_of("0123456789") != std::string::npos) throw std::invalid_argument("parse_path: bad component");
        const unsigned long long v = std::stoull(c);
        if (v >= 0x80000000ull) throw std::invalid_argument("parse_path: index not below 2^31");
        out.push_back((uint32_t)v + (hard ? 0x80000000u : 0u));
        if (out.size() > PLUME_HD_MAX_DEPTH) throw std::invalid_argument("parse_path: too deep");
        if (end == path.size()) break;
        pos = end + 1;
    }
    return out;
}
inline void hd_check_status(uint8_t st) {
    if (st) throw SignatureError();      // 2: an invalid parent; PLUME_STATUS_HD_NO_KEY: the path has no key; PLUME_STATUS_HD_HARDENED: a public key has no hardened children
}
// HMAC-SHA512("Bitcoin seed", seed), 16 <= len <= 64
inline HdNode hd_master(const uint8_t* seed, size_t len, Engine& eng = Engine::shared()) {
    Bytes32 sk{}, chain{};
    uint8_t st = 0xFF;
    plume_hip::check(plume_hd_master_batch(eng.ctx(), 1, seed, len, sk.data(), chain.data(), &st), "plume_hd_master_batch");
    hd_check_status(st);
    return {*SecretKey::from_bytes(sk), chain};
}
inline HdNode hd_derive(const SecretKey& sk, const Bytes32& chain, const std::string& path, Engine& eng = Engine::shared()) {
    const std::vector<uint32_t> idx = parse_path(path);
    Bytes32 csk{}, cchain{};
    uint8_t st = 0xFF;
    plume_hip::check(plume_hd_derive_priv_batch(eng.ctx(), 0, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, 1, sk.to_bytes().data(), chain.data(), idx.data(), idx.size(), csk.data(),
                                                cchain.data(), nullptr, nullptr, &st),
                     "plume_hd_derive_priv_batch");
    hd_check_status(st);
    return {*SecretKey::from_bytes(csk), cchain};
}
// non-hardened indices only ("0/3"): what a watcher holding an xpub derives
inline HdPubNode hd_derive_pub(const AffinePoint& pk, const Bytes32& chain, const std::string& path, Engine& eng = Engine::shared()) {
    const std::vector<uint32_t> idx = parse_path(path);
    uint8_t cpk[64], st = 0xFF;
    Bytes32 cchain{};
    plume_hip::check(plume_hd_derive_pub_batch(eng.ctx(), 0, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, 1, pk.xy.data(), chain.data(), idx.data(), idx.size(), cpk, cchain.data(),
                                               nullptr, &st),
                     "plume_hd_derive_pub_batch");
    hd_check_status(st);
    return {AffinePoint::from_bytes64(cpk), cchain};
}
// the 20-byte Ethereum address of the key at `path` below a private node, or (non-hardened path) below a public one
inline std::array<uint8_t, 20> hd_address(const SecretKey& sk, const Bytes32& chain, const std::string& path, Engine& eng = Engine::shared()) {
    const std::vector<uint32_t> idx = parse_path(path);
    Bytes32 csk{};
    std::array<uint8_t, 20> addr{};
    uint8_t st = 0xFF;
    plume_hip::check(plume_hd_derive_priv_batch(eng.ctx(), 0, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, 1, sk.to_bytes().data(), chain.data(), idx.data(), idx.size(), csk.data(),
                                                nullptr, nullptr, addr.data(), &st),
                     "plume_hd_derive_priv_batch");
    csk.fill(0);
    hd_check_status(st);
    return addr;
}
inline std::array<uint8_t, 20> hd_address(const AffinePoint& pk, const Bytes32& chain, const std::string& path, Engine& eng = Engine::shared()) {
    const std::vector<uint32_t> idx = parse_path(path);
    uint8_t cpk[64], st = 0xFF;
    std::array<uint8_t, 20> addr{};
    plume_hip::check(plume_hd_derive_pub_batch(eng.ctx(), 0, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, 1, pk.xy.data(), chain.data(), idx.data(), idx.size(), cpk, nullptr,
                                               addr.data(), &st),
                     "plume_hd_derive_pub_batch");
    hd_check_status(st);
    return addr;
}
// ---- BIP-39 seeds (plume_hip.h, library 0.18): PBKDF2-HMAC-SHA512 on the GPU, over bytes.  A caller with non-ASCII text normalises it (NFKD) first; the word list is
// out of scope, any bytes have a seed.
// PBKDF2-HMAC-SHA512(password, salt, iterations)[0 .. dklen), 1 <= dklen <= 64, salt of at most PLUME_KDF_MAX_SALT bytes
inline plume_hip::Bytes pbkdf2_sha512(const uint8_t* password, size_t password_len, const uint8_t* salt, size_t salt_len, uint32_t iterations, size_t dklen = 64,
                                      Engine& eng = Engine::shared()) {
    const uint64_t off[2] = {0, password_len};
    plume_hip::Bytes out(dklen ? dklen : 1);
    uint8_t st = 0xFF;
    plume_hip::check(plume_pbkdf2_sha512_batch(eng.ctx(), PLUME_KDF_SHARED_SALT, 1, password, off, salt, salt_len, iterations, dklen, out.data(), &st), "plume_pbkdf2_sha512_batch");
    if (st) throw SignatureError();
    return out;
}
// the 64-byte BIP-39 seed of a mnemonic sentence: PBKDF2-HMAC-SHA512(sentence, "mnemonic" || passphrase, 2048)
inline std::array<uint8_t, 64> mnemonic_to_seed(const std::string& mnemonic, const std::string& passphrase = "", Engine& eng = Engine::shared()) {
    const uint64_t off[2] = {0, mnemonic.size()};
    std::array<uint8_t, 64> seed{};
    uint8_t st = 0xFF;
    plume_hip::check(plume_pbkdf2_sha512_batch(eng.ctx(), PLUME_KDF_BIP39 | PLUME_KDF_SHARED_SALT, 1, (const uint8_t*)mnemonic.data(), off, (const uint8_t*)passphrase.data(),
                                               passphrase.size(), 2048, 64, seed.data(), &st),
                     "plume_pbkdf2_sha512_batch");
    if (st) throw SignatureError();
    return seed;
}
// An extended key "xprv..." / "xpub..." (mainnet), base58check DECODE only: depth, child number, chain code and the key -- 32 bytes of sk in key[1 .. 33) behind a zero
// byte, or the 33 SEC1 bytes of pk.  std::invalid_argument for a bad digit, length, checksum or version.
struct ExtendedKey { uint8_t depth; uint32_t child_number; Bytes32 chain; std::array<uint8_t, 33> key; };
namespace hd_detail {
inline void sha256(const uint8_t* msg, size_t len, uint8_t out[32]) {          // host-side, for the four checksum bytes only
    static const uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74,
        0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d,
        0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e,
        0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5,
        0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    std::vector<uint8_t> m(msg, msg + len);
    m.push_back(0x80);
    while (m.size() % 64 != 56) m.push_back(0);
    for (int b = 7; b >= 0; b--) m.push_back((uint8_t)(((uint64_t)len * 8) >> (8 * b)));
    auto rotr = [](uint32_t x, int n) { return (x >> n) | (x << (32 - n)); };
    for (size_t blk = 0; blk < m.size(); blk += 64) {
        uint32_t w[64];
        for (int i = 0; i < 16; i++) w[i] = ((uint32_t)m[blk + 4 * i] << 24) | ((uint32_t)m[blk + 4 * i + 1] << 16) | ((uint32_t)m[blk + 4 * i + 2] << 8) | m[blk + 4 * i + 3];
        for (int i = 16; i < 64; i++) w[i] = w[i - 16] + (rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7] + (rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10));
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
        for (int i = 0; i < 64; i++) {
            const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
            const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
            hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
    }
    for (int i = 0; i < 8; i++) for (int b = 0; b < 4; b++) out[4 * i + b] = (uint8_t)(h[i] >> (24 - 8 * b));
}
inline ExtendedKey parse_xkey(const std::string& s, uint32_t version) {
    static const char* digits = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz";
    uint8_t raw[82] = {0};
    for (char ch : s) {
        const char* d = ch ? std::strchr(digits, ch) : nullptr;
        if (!d) throw std::invalid_argument("extended key: not a base58 digit");
        uint32_t carry = (uint32_t)(d - digits);
        for (int i = 81; i >= 0; i--) { carry += 58u * raw[i]; raw[i] = (uint8_t)carry; carry >>= 8; }
        if (carry) throw std::invalid_argument("extended key: longer than 82 bytes");
    }
    uint8_t h1[32], h2[32];
    sha256(raw, 78, h1); sha256(h1, 32, h2);
    if (std::memcmp(h2, raw + 78, 4) != 0) throw std::invalid_argument("extended key: checksum");
    if ((((uint32_t)raw[0] << 24) | ((uint32_t)raw[1] << 16) | ((uint32_t)raw[2] << 8) | raw[3]) != version) throw std::invalid_argument("extended key: version bytes");
    ExtendedKey k;
    k.depth = raw[4];
    k.child_number = ((uint32_t)raw[9] << 24) | ((uint32_t)raw[10] << 16) | ((uint32_t)raw[11] << 8) | raw[12];
    std::memcpy(k.chain.data(), raw + 13, 32);
    std::memcpy(k.key.data(), raw + 45, 33);
    return k;
}
}  // namespace hd_detail
inline ExtendedKey parse_xprv(const std::string& s) {
    const ExtendedKey k = hd_detail::parse_xkey(s, 0x0488ADE4u);
    if (k.key[0] != 0) throw std::invalid_argument("parse_xprv: the key is not 00 || 32 bytes");
    return k;
}
inline ExtendedKey parse_xpub(const std::string& s) {
    const ExtendedKey k = hd_detail::parse_xkey(s, 0x0488B21Eu);
    if (k.key[0] != 2 && k.key[0] != 3) throw std::invalid_argument("parse_xpub: the key is not a compressed point");
    return k;
}
inline std::pair<AffinePoint, std::array<uint8_t, 20>> tx_sender(const uint8_t* raw, size_t len, Engine& eng = Engine::shared(), bool low_s = true) {
    const uint64_t off[2] = {0, (uint64_t)len};
    uint8_t pk[64], st = 0xFF;
    std::array<uint8_t, 20> addr{};
    plume_hip::check(plume_eth_tx_sender_batch(eng.ctx(), low_s ? PLUME_ECDSA_LOW_S : 0, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, 1, raw, off, nullptr, pk, addr.data(), nullptr,
                                               nullptr, &st),
                     "plume_eth_tx_sender_batch");
    if (st == PLUME_ECDSA_INVALID) throw SignatureError();
    return {AffinePoint::from_bytes64(pk), addr};
}
inline std::array<uint8_t, 20> tx_sender_address(const uint8_t* raw, size_t len, Engine& eng = Engine::shared(), bool low_s = true) {
    const uint64_t off[2] = {0, (uint64_t)len};
    uint8_t st = 0xFF;
    std::array<uint8_t, 20> addr{};
    plume_hip::check(plume_eth_tx_sender_batch(eng.ctx(), low_s ? PLUME_ECDSA_LOW_S : 0, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, 1, raw, off, nullptr, nullptr, addr.data(),
                                               nullptr, nullptr, &st),
                     "plume_eth_tx_sender_batch");
    if (st == PLUME_ECDSA_INVALID) throw SignatureError();
    return addr;
}

// Keccak Merkle allow-lists (plume_hip.h plume_merkle_*): the tree OpenZeppelin's StandardMerkleTree builds and MerkleProof.verify checks, made on the GPU.  merkle_leaf:
// the leaf of an account, Keccak(Keccak(abi.encode(address))) or, with an amount (32 big-endian bytes), Keccak(Keccak(abi.encode(address, amount))).  merkle_root /
// merkle_proof: the root of the tree over 32-byte leaves and the siblings of leaf `index`, leaf side first (sort: order the leaves by hash first, as StandardMerkleTree
// does).  merkle_verify: MerkleProof.verify of a 32-byte leaf; merkle_verify_address computes the leaf of an address first, in the same kernel.
inline Bytes32 merkle_leaf(const std::array<uint8_t, 20>& addr20, const Bytes32* amount = nullptr, Engine& eng = Engine::shared()) {
    Bytes32 leaf{};
    plume_hip::check(plume_merkle_leaf_batch(eng.ctx(), amount ? PLUME_MERKLE_LEAF_ADDRESS_UINT256 : PLUME_MERKLE_LEAF_ADDRESS, PLUME_ETH_ADDR_RAW20, 1, addr20.data(),
                                             amount ? amount->data() : nullptr, leaf.data(), nullptr),
                     "plume_merkle_leaf_batch");
    return leaf;
}
namespace merkle_detail {
inline std::vector<uint8_t> merkle_tree(const std::vector<Bytes32>& leaves, bool sort, std::vector<uint32_t>& leaf_pos, Engine& eng) {
    std::vector<uint8_t> flat(32 * leaves.size()), tree(leaves.empty() ? 0 : 32 * (2 * leaves.size() - 1));
    for (size_t i = 0; i < leaves.size(); i++) std::copy(leaves[i].begin(), leaves[i].end(), flat.begin() + 32 * i);
    leaf_pos.assign(leaves.size(), 0);
    plume_hip::check(plume_merkle_tree_build(eng.ctx(), sort ? PLUME_MERKLE_SORT_LEAVES : 0, leaves.size(), flat.data(), tree.data(), leaf_pos.data()), "plume_merkle_tree_build");
    return tree;
}
}  // namespace merkle_detail
inline Bytes32 merkle_root(const std::vector<Bytes32>& leaves, bool sort = true, Engine& eng = Engine::shared()) {
    std::vector<uint32_t> pos;
    const std::vector<uint8_t> tree = merkle_detail::merkle_tree(leaves, sort, pos, eng);
    Bytes32 root{};
    std::copy(tree.begin(), tree.begin() + 32, root.begin());
    return root;
}
inline std::vector<Bytes32> merkle_proof(const std::vector<Bytes32>& leaves, size_t index, bool sort = true, Engine& eng = Engine::shared()) {
    std::vector<uint32_t> pos;
    const std::vector<uint8_t> tree = merkle_detail::merkle_tree(leaves, sort, pos, eng);
    if (index >= leaves.size()) throw std::out_of_range("merkle_proof: index");
    const size_t depth = plume_merkle_max_proof_len(leaves.size());
    std::vector<uint8_t> slots(32 * depth + 1);
    uint8_t len = 0;
    plume_hip::check(plume_merkle_proof_batch(eng.ctx(), leaves.size(), tree.data(), 1, &pos[index], depth, slots.data(), &len), "plume_merkle_proof_batch");
    std::vector<Bytes32> proof(len == PLUME_MERKLE_BAD_PROOF ? 0 : len);
    for (size_t k = 0; k < proof.size(); k++) std::copy(slots.begin() + 32 * k, slots.begin() + 32 * k + 32, proof[k].begin());
    return proof;
}
namespace merkle_detail {
inline bool merkle_verify_item(int leaf_format, const uint8_t* item, const Bytes32* amount, const std::vector<Bytes32>& proof, const Bytes32& root32, Engine& eng) {
    if (proof.size() > 64) return false;
    std::vector<uint8_t> slots(32 * proof.size() + 1);
    for (size_t k = 0; k < proof.size(); k++) std::copy(proof[k].begin(), proof[k].end(), slots.begin() + 32 * k);
    const uint8_t len = (uint8_t)proof.size();
    uint8_t st = 0xFF;
    plume_hip::check(plume_merkle_verify_batch(eng.ctx(), leaf_format, PLUME_ETH_ADDR_RAW20, 1, item, amount ? amount->data() : nullptr, proof.size(), slots.data(), &len, root32.data(), &st),
          "plume_merkle_verify_batch");
    return st == PLUME_MERKLE_MATCH;
}
}  // namespace merkle_detail
inline bool merkle_verify(const Bytes32& leaf, const std::vector<Bytes32>& proof, const Bytes32& root32, Engine& eng = Engine::shared()) {
    return merkle_detail::merkle_verify_item(PLUME_MERKLE_LEAF_HASH32, leaf.data(), nullptr, proof, root32, eng);
}
inline bool merkle_verify_address(const std::array<uint8_t, 20>& addr20, const std::vector<Bytes32>& proof, const Bytes32& root32, const Bytes32* amount = nullptr,
                                  Engine& eng = Engine::shared()) {
    return merkle_detail::merkle_verify_item(amount ? PLUME_MERKLE_LEAF_ADDRESS_UINT256 : PLUME_MERKLE_LEAF_ADDRESS, addr20.data(), amount, proof, root32, eng);
}
inline bool PlumeSignature::verify_for_root(const Bytes32& root32, const std::vector<Bytes32>& proof, const Bytes32* amount, Engine& eng) const {
    uint8_t st = 0xFF;
    std::array<uint8_t, 20> addr{};
    plume_hip::check(plume_eth_address_batch(eng.ctx(), PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, 1, pk.xy.data(), nullptr, addr.data(), &st), "plume_eth_address_batch");
    return st != PLUME_ETH_INVALID && merkle_verify_address(addr, proof, root32, amount, eng) && verify(eng);
}

// rust-k256/src/randomizedsigner.rs:25-41: a borrowed secret key and the variant
class PlumeSigner {
  public:
    PlumeSigner(const SecretKey& secret_key, bool v1_) : v1(v1_), secret_key_(secret_key) {}
    bool v1;
    // RandomizedSigner::try_sign_with_rng (randomizedsigner.rs:43-112)
    template <class Rng>
    PlumeSignature try_sign_with_rng(Rng& rng, const Bytes& msg, Engine& eng = Engine::shared()) const;
    template <class Rng>
    PlumeSignature sign_with_rng(Rng& rng, const Bytes& msg, Engine& eng = Engine::shared()) const { return try_sign_with_rng(rng, msg, eng); }
    // the nonce derived on the GPU by RFC 6979 from (secret key, variant, message), hedged with aux when given (plume_hip.h, plume_sign_batch_rfc6979)
    PlumeSignature sign_deterministic(const Bytes& msg, const std::optional<Bytes32>& aux = std::nullopt, Engine& eng = Engine::shared()) const;

  private:
    const SecretKey& secret_key_;
};

// status byte of the signer -> the reference's panics, in the order the reference would hit them (randomizedsigner.rs:61,91,95)
inline void raise_for_status(uint8_t st, const AffinePoint& nullifier) {
    if (st & PLUME_STATUS_SELFCHECK_FAILED) throw plume_hip::SelfCheckError("the signature does not verify and was withheld (plume_set_sign_selfcheck)");
    if (st & PLUME_STATUS_BAD_SCALAR) throw Panic("secret key or nonce outside [1, n-1] (no SecretKey / NonZeroScalar holds it)");
    if ((st & PLUME_STATUS_IDENTITY) && nullifier.is_identity()) throw Panic("something is drammatically wrong if the input hashed to the identity");
    if (st & PLUME_STATUS_C_NOT_CANONICAL) throw Panic("it should be impossible to get the hash equal to zero");
    if (st & PLUME_STATUS_IDENTITY) throw Panic("something is terribly wrong if the nonce is equal to negated product of the secret and the hash");
}

// the signatures of one sign call's outputs; throws Panic at the first item the reference's signer would panic on
inline std::vector<PlumeSignature> detail_signatures(const std::vector<Bytes>& msgs, bool v1, const Bytes& pk, const Bytes& nul, const Bytes& c, const Bytes& s, const Bytes& rp,
                                                     const Bytes& hr, const Bytes& st) {
    const size_t n = msgs.size();
    std::vector<PlumeSignature> out;
    out.reserve(n);
    for (size_t i = 0; i < n; i++) {
        const AffinePoint nl = AffinePoint::from_bytes64(&nul[64 * i]);
        raise_for_status(st[i], nl);
        Bytes32 cb, sb;
        std::memcpy(cb.data(), &c[32 * i], 32);
        std::memcpy(sb.data(), &s[32 * i], 32);
        auto cs = NonZeroScalar::from_repr(cb), ss = NonZeroScalar::from_repr(sb);
        if (!cs) throw Panic("it should be impossible to get the hash equal to zero");
        if (!ss) throw Panic("something is terribly wrong if the nonce is equal to negated product of the secret and the hash");
        PlumeSignature g{msgs[i], AffinePoint::from_bytes64(&pk[64 * i]), nl, *cs, *ss, std::nullopt};
        if (v1) g.v1specific = PlumeSignatureV1Fields{AffinePoint::from_bytes64(&rp[64 * i]), AffinePoint::from_bytes64(&hr[64 * i])};
        out.push_back(std::move(g));
    }
    return out;
}
// batch twin of the signer with the nonces supplied (the RNG stays on the host): one signature per (key, message, nonce).  Throws Panic at the first
// item the reference's signer would panic on.
inline std::vector<PlumeSignature> sign_batch_with_nonces(const std::vector<SecretKey>& keys, const std::vector<Bytes>& msgs, bool v1, const std::vector<SecretKey>& nonces,
                                                          Engine& eng = Engine::shared()) {
    const size_t n = keys.size();
    if (msgs.size() != n || nonces.size() != n) throw std::invalid_argument("keys, msgs and nonces must have one entry per signature");
    plume_hip::PackedMessages m;
    Bytes sk(32 * n), r(32 * n), pk(64 * n), nul(64 * n), c(32 * n), s(32 * n), rp(64 * n), hr(64 * n), st(n);
    for (size_t i = 0; i < n; i++) {
        m.push(msgs[i].data(), msgs[i].size());
        std::memcpy(&sk[32 * i], keys[i].to_bytes().data(), 32);
        std::memcpy(&r[32 * i], nonces[i].to_bytes().data(), 32);
    }
    std::vector<PlumeSignature> out;
    if (n == 0) return out;
    const int rc = plume_sign_batch(eng.ctx(), v1 ? 1 : 2, n, m.data(), m.off.data(), sk.data(), r.data(), nullptr, pk.data(), nul.data(), c.data(), s.data(), rp.data(), hr.data(), st.data());
    { volatile uint8_t* w = sk.data(); for (size_t i = 0; i < sk.size(); i++) w[i] = 0; }
    { volatile uint8_t* w = r.data(); for (size_t i = 0; i < r.size(); i++) w[i] = 0; }
    plume_hip::check(rc, "plume_sign_batch");
    return detail_signatures(msgs, v1, pk, nul, c, s, rp, hr, st);
}
// ... and with each nonce derived on the GPU by RFC 6979 (plume_hip.h, plume_sign_batch_rfc6979): no nonce exists in host memory.  aux: empty, or one 32-byte
// hedging input per signature (RFC 6979 section 3.6).
inline std::vector<PlumeSignature> sign_batch_deterministic(const std::vector<SecretKey>& keys, const std::vector<Bytes>& msgs, bool v1, const std::vector<Bytes32>& aux = {},
                                                            Engine& eng = Engine::shared()) {
    const size_t n = keys.size();
    if (msgs.size() != n || (!aux.empty() && aux.size() != n)) throw std::invalid_argument("keys, msgs and aux (when given) must have one entry per signature");
    plume_hip::PackedMessages m;
    Bytes sk(32 * n), ax(32 * aux.size()), pk(64 * n), nul(64 * n), c(32 * n), s(32 * n), rp(64 * n), hr(64 * n), st(n);
    for (size_t i = 0; i < n; i++) {
        m.push(msgs[i].data(), msgs[i].size());
        std::memcpy(&sk[32 * i], keys[i].to_bytes().data(), 32);
        if (!aux.empty()) std::memcpy(&ax[32 * i], aux[i].data(), 32);
    }
    if (n == 0) return {};
    const int rc = plume_sign_batch_rfc6979(eng.ctx(), v1 ? 1 : 2, n, m.data(), m.off.data(), sk.data(), aux.empty() ? nullptr : ax.data(), nullptr, pk.data(), nul.data(),
                                            c.data(), s.data(), rp.data(), hr.data(), st.data());
    { volatile uint8_t* w = sk.data(); for (size_t i = 0; i < sk.size(); i++) w[i] = 0; }
    { volatile uint8_t* w = ax.data(); for (size_t i = 0; i < ax.size(); i++) w[i] = 0; }
    plume_hip::check(rc, "plume_sign_batch_rfc6979");
    return detail_signatures(msgs, v1, pk, nul, c, s, rp, hr, st);
}
inline PlumeSignature PlumeSigner::sign_deterministic(const Bytes& msg, const std::optional<Bytes32>& aux, Engine& eng) const {
    return std::move(sign_batch_deterministic({secret_key_}, {msg}, v1, aux ? std::vector<Bytes32>{*aux} : std::vector<Bytes32>{}, eng)[0]);
}
// ... and with the nonces drawn as the reference draws them: SecretKey::random(rng) per signature, in order (randomizedsigner.rs:49)
template <class Rng>
std::vector<PlumeSignature> sign_batch(const std::vector<SecretKey>& keys, const std::vector<Bytes>& msgs, bool v1, Rng& rng, Engine& eng = Engine::shared()) {
    std::vector<SecretKey> nonces;
    nonces.reserve(keys.size());
    for (size_t i = 0; i < keys.size(); i++) nonces.push_back(SecretKey::random(rng));
    return sign_batch_with_nonces(keys, msgs, v1, nonces, eng);
}

template <class Rng>
PlumeSignature PlumeSigner::try_sign_with_rng(Rng& rng, const Bytes& msg, Engine& eng) const {
    const SecretKey r_scalar = SecretKey::random(rng);                                         // randomizedsigner.rs:49
    return std::move(sign_batch_with_nonces({secret_key_}, {msg}, v1, {r_scalar}, eng)[0]);
}
template <class Rng>
PlumeSignature PlumeSignature::sign_v1(const SecretKey& secret_key, const Bytes& msg, Rng& rng, Engine& eng) { return PlumeSigner(secret_key, true).sign_with_rng(rng, msg, eng); }
template <class Rng>
PlumeSignature PlumeSignature::sign_v2(const SecretKey& secret_key, const Bytes& msg, Rng& rng, Engine& eng) { return PlumeSigner(secret_key, false).sign_with_rng(rng, msg, eng); }

// ---- the steps either side of sign / verify, as the Rust binding has them (bindings/rust/plume-hip) ----
// The serde / wasm wire format (javascript/src/lib.rs:95-118,147-184): points as 33-byte SEC1-compressed records (02|03 || x; a record starting with 00 is the
// identity), decompressed and validated on the GPU; a record that would fail AffinePoint::from_encoded_point gives false.  Arrays hold n records each; r_point33 /
// hashed_to_curve_r33 are used for v1 only.
inline std::vector<bool> verify_batch_sec1(bool v1, const std::vector<Bytes>& msgs, const Bytes& pk33, const Bytes& nullifier33, const Bytes& c, const Bytes& s, const Bytes& r_point33,
                                           const Bytes& hashed_to_curve_r33, Engine& eng = Engine::shared()) {
    const size_t n = msgs.size();
    if (pk33.size() != 33 * n || nullifier33.size() != 33 * n || c.size() != 32 * n || s.size() != 32 * n || (v1 && (r_point33.size() != 33 * n || hashed_to_curve_r33.size() != 33 * n)))
        throw std::invalid_argument("verify_batch_sec1: arrays must hold one record per message");
    plume_hip::PackedMessages m;
    for (const Bytes& x : msgs) m.push(x.data(), x.size());
    Bytes ok(n);
    if (n) plume_hip::check(plume_verify_batch_sec1(eng.ctx(), v1 ? 1 : 2, n, m.data(), m.off.data(), pk33.data(), nullifier33.data(), c.data(), s.data(), v1 ? r_point33.data() : nullptr,
                                                    v1 ? hashed_to_curve_r33.data() : nullptr, ok.data()), "plume_verify_batch_sec1");
    return std::vector<bool>(ok.begin(), ok.end());
}
// AffinePoint::to_encoded_point(true) as the fixed 33-byte record of that wire format (identity: 00 followed by zeros)
inline std::array<uint8_t, 33> sec1_record(const AffinePoint& p) {
    std::array<uint8_t, 33> r{};
    if (!p.is_identity()) { r[0] = (uint8_t)(2 + (p.xy[63] & 1)); std::memcpy(r.data() + 1, p.xy.data(), 32); }
    return r;
}
// Aggregate pre-filter (no reference counterpart; plume_hip.h plume_aggregate_check): true iff every V1 signature of the batch would verify() -- up to a false-accept
// probability of 2^-126 over `seed`, 32 fresh random bytes the signers could not predict.  All-or-nothing: on false, verify_batch finds the culprits.
// `seed == nullptr`: the library draws the 32 bytes from the OS generator for this call -- what a caller without fresh randomness of its own should do.
inline bool aggregate_check_v1(const std::vector<PlumeSignature>& sigs, const Bytes32* seed, Engine& eng = Engine::shared()) {
    plume_hip::PackedMessages m;
    Bytes pk, nul, c, s, rp, hr;
    for (const PlumeSignature& g : sigs) {
        if (!g.v1specific) throw std::invalid_argument("the aggregate check needs the V1 fields r_point / hashed_to_curve_r");
        m.push(g.message.data(), g.message.size());
        pk.insert(pk.end(), g.pk.xy.begin(), g.pk.xy.end());
        nul.insert(nul.end(), g.nullifier.xy.begin(), g.nullifier.xy.end());
        c.insert(c.end(), g.c.to_bytes().begin(), g.c.to_bytes().end());
        s.insert(s.end(), g.s.to_bytes().begin(), g.s.to_bytes().end());
        rp.insert(rp.end(), g.v1specific->r_point.xy.begin(), g.v1specific->r_point.xy.end());
        hr.insert(hr.end(), g.v1specific->hashed_to_curve_r.xy.begin(), g.v1specific->hashed_to_curve_r.xy.end());
    }
    uint8_t rec[PLUME_AGG_RESULT_BYTES];
    static const uint8_t none[64] = {0};
    const bool e = sigs.empty();
    plume_hip::check(plume_aggregate_check(eng.ctx(), 1, 0, sigs.size(), m.data(), m.off.data(), e ? none : pk.data(), e ? none : nul.data(), e ? none : c.data(), e ? none : s.data(),
                                           e ? none : rp.data(), e ? none : hr.data(), seed ? seed->data() : nullptr, nullptr, rec), "plume_aggregate_check");
    return rec[0] == 1;
}
inline bool aggregate_check_v1(const std::vector<PlumeSignature>& sigs, const Bytes32& seed, Engine& eng = Engine::shared()) { return aggregate_check_v1(sigs, &seed, eng); }
inline bool aggregate_check_v1(const std::vector<PlumeSignature>& sigs, Engine& eng = Engine::shared()) { return aggregate_check_v1(sigs, static_cast<const Bytes32*>(nullptr), eng); }
// The application step after verification (reference README.md:5: one nullifier per (pk, message)): first[i] is true iff item i is live and no live item with the
// same nullifier comes before it.  `live` may be empty (all items take part), e.g. pass verify_batch's result.
inline std::vector<bool> nullifier_first_occurrence(const std::vector<AffinePoint>& nullifiers, const std::vector<bool>& live = {}, Engine& eng = Engine::shared()) {
    const size_t n = nullifiers.size();
    if (!live.empty() && live.size() != n) throw std::invalid_argument("live must be empty or hold one flag per nullifier");
    Bytes nul(64 * n), lv(live.begin(), live.end()), first(n);
    for (size_t i = 0; i < n; i++) std::memcpy(&nul[64 * i], nullifiers[i].xy.data(), 64);
    if (n) plume_hip::check(plume_nullifier_first_occurrence(eng.ctx(), n, nul.data(), live.empty() ? nullptr : lv.data(), nullptr, first.data(), nullptr), "plume_nullifier_first_occurrence");
    return std::vector<bool>(first.begin(), first.end());
}
// SecretKey::from(scalar).to_sec1_der() for a batch -- the encoding the wasm wrapper uses for `s` and `digest_private` (javascript/src/lib.rs:98-110): the 109-byte
// SEC1 ECPrivateKey with publicKey = scalar * G, the generator multiplications on the GPU
inline std::vector<std::array<uint8_t, 109>> scalars_to_sec1_der(const std::vector<NonZeroScalar>& scalars, Engine& eng = Engine::shared()) {
    const size_t n = scalars.size();
    Bytes flat(32 * n), der(109 * n), st(n);
    for (size_t i = 0; i < n; i++) std::memcpy(&flat[32 * i], scalars[i].to_bytes().data(), 32);
    if (n) plume_hip::check(plume_scalars_to_sec1_der_batch(eng.ctx(), n, flat.data(), der.data(), st.data()), "plume_scalars_to_sec1_der_batch");
    std::vector<std::array<uint8_t, 109>> out(n);
    for (size_t i = 0; i < n; i++) std::memcpy(out[i].data(), &der[109 * i], 109);
    return out;
}
// SecretKey::from_sec1_der for that fixed form: nullopt where the reference returns Err -- a record of another shape, a scalar outside [1, n-1], or an embedded
// public key that is not scalar * G (elliptic-curve's TryFrom<EcPrivateKey> validates it; here the GPU recomputes it)
inline std::optional<NonZeroScalar> scalar_from_sec1_der(const std::array<uint8_t, 109>& der, Engine& eng = Engine::shared()) {
    Bytes32 k; uint8_t ok = 0;
    plume_hip::check(plume_sec1_der_to_scalars_checked(eng.ctx(), 1, der.data(), k.data(), &ok), "plume_sec1_der_to_scalars_checked");
    if (!ok) return std::nullopt;
    return NonZeroScalar::from_repr(k);
}

// hash_to_curve(m, pk) (rust-k256/src/utils.rs:11-20): RFC 9380 hash_to_curve over m || SEC1c(pk)
inline AffinePoint hash_to_curve(const Bytes& m, const AffinePoint& pk, Engine& eng = Engine::shared()) {
    plume_hip::PackedMessages pm;
    pm.push(m.data(), m.size());
    AffinePoint h;
    plume_hip::check(plume_hash_to_curve_batch(eng.ctx(), 1, pm.data(), pm.off.data(), pk.xy.data(), h.xy.data()), "plume_hash_to_curve_batch");
    return h;
}
// Secp256k1::hash_from_bytes::<ExpandMsgXmd<Sha256>>(&[s], &[DST]) over the raw bytes (rust-k256/tests/verification.rs:148-156 `hash_to_secp`)
inline AffinePoint hash_to_secp(const Bytes& s, Engine& eng = Engine::shared()) {
    plume_hip::PackedMessages pm;
    pm.push(s.data(), s.size());
    AffinePoint h;
    plume_hip::check(plume_hash_to_curve_batch(eng.ctx(), 1, pm.data(), pm.off.data(), nullptr, h.xy.data()), "plume_hash_to_curve_batch");
    return h;
}

// The circom verifier's hash_to_curve inputs for one signature (circuits/circom/verify_nullifier.circom:14-31), every value as the circuit's four 64-bit little-endian
// registers (circuits/circom/utils.ts:11-17): q{0,1}_x_mapped / q{0,1}_y_mapped from plume_h2c_intermediates_batch (pinned to the reference's vectors) and
// q{0,1}_gx1_sqrt / gx2_sqrt / y_pos from plume_h2c_hints_batch (UNPINNED definitions: include/plume_hip.h).
struct CircuitH2cInputs {
    using Reg = std::array<uint64_t, 4>;
    Reg q0_gx1_sqrt, q0_gx2_sqrt, q0_y_pos, q0_x_mapped, q0_y_mapped, q1_gx1_sqrt, q1_gx2_sqrt, q1_y_pos, q1_x_mapped, q1_y_mapped;
};
inline CircuitH2cInputs circuit_h2c_inputs(const Bytes& m, const AffinePoint& pk, Engine& eng = Engine::shared()) {
    plume_hip::PackedMessages pm;
    pm.push(m.data(), m.size());
    uint64_t hints[24], mapped[16];
    plume_hip::check(plume_h2c_hints_batch(eng.ctx(), 1, pm.data(), pm.off.data(), pk.xy.data(), 1, reinterpret_cast<uint8_t*>(hints)), "plume_h2c_hints_batch");
    plume_hip::check(plume_h2c_intermediates_batch(eng.ctx(), 1, pm.data(), pm.off.data(), pk.xy.data(), 1, nullptr, reinterpret_cast<uint8_t*>(mapped), nullptr, nullptr),
                     "plume_h2c_intermediates_batch");
    auto reg = [](const uint64_t* p) { return CircuitH2cInputs::Reg{p[0], p[1], p[2], p[3]}; };
    CircuitH2cInputs o;
    o.q0_gx1_sqrt = reg(hints); o.q0_gx2_sqrt = reg(hints + 4); o.q0_y_pos = reg(hints + 8);
    o.q1_gx1_sqrt = reg(hints + 12); o.q1_gx2_sqrt = reg(hints + 16); o.q1_y_pos = reg(hints + 20);
    o.q0_x_mapped = reg(mapped); o.q0_y_mapped = reg(mapped + 4); o.q1_x_mapped = reg(mapped + 8); o.q1_y_mapped = reg(mapped + 12);
    return o;
}

}  // namespace plume_rustcrypto

namespace plume_hip {

// A persistent nullifier set (plume_hip.h, plume_nullset_*): GPU-resident, it remembers every nullifier inserted into it across calls, so that an application
// accepts ONE signature per nullifier over a stream of batches.  Lives on the engine's (first) GPU; may outlive the engine.  One host thread at a time.
class NullifierSet {
  public:
    explicit NullifierSet(Engine& eng, size_t reserve = 0) { check(plume_nullset_create(eng.ctx(), reserve, &set_), "plume_nullset_create"); }
    ~NullifierSet() { plume_nullset_destroy(set_); }
    NullifierSet(const NullifierSet&) = delete;
    NullifierSet& operator=(const NullifierSet&) = delete;
    NullifierSet(NullifierSet&& o) noexcept : set_(o.set_) { o.set_ = nullptr; }
    void* handle() const { return set_; }
    // fresh[i]: live[i] (empty = all), the nullifier was not in the set, and no earlier live item of this call has it; every live nullifier is in the set afterwards
    std::vector<bool> insert(const std::vector<plume_rustcrypto::AffinePoint>& nullifiers, const std::vector<bool>& live = {}, uint64_t* n_fresh = nullptr) {
        const size_t n = nullifiers.size();
        if (!live.empty() && live.size() != n) throw std::invalid_argument("live must be empty or hold one flag per nullifier");
        Bytes nul = pack(nullifiers), lv(live.begin(), live.end()), fresh(n);
        uint64_t cnt = 0;
        check(plume_nullset_insert(set_, n, nul.data(), live.empty() ? nullptr : lv.data(), nullptr, fresh.data(), &cnt), "plume_nullset_insert");
        if (n_fresh) *n_fresh = cnt;
        return std::vector<bool>(fresh.begin(), fresh.end());
    }
    std::vector<bool> contains(const std::vector<plume_rustcrypto::AffinePoint>& nullifiers) const {
        Bytes nul = pack(nullifiers), found(nullifiers.size());
        check(plume_nullset_contains(set_, nullifiers.size(), nul.data(), found.data()), "plume_nullset_contains");
        return std::vector<bool>(found.begin(), found.end());
    }
    uint64_t size() const { uint64_t s = 0, c = 0; check(plume_nullset_size(set_, &s, &c), "plume_nullset_size"); return s; }
    uint64_t capacity() const { uint64_t s = 0, c = 0; check(plume_nullset_size(set_, &s, &c), "plume_nullset_size"); return c; }
    void reserve(size_t items) { check(plume_nullset_reserve(set_, items), "plume_nullset_reserve"); }
    void clear() { check(plume_nullset_clear(set_), "plume_nullset_clear"); }
    // every nullifier of the set, in no particular order
    std::vector<plume_rustcrypto::AffinePoint> export_all() const {
        uint64_t cnt = 0;
        check(plume_nullset_export(set_, 0, nullptr, &cnt), "plume_nullset_export");
        Bytes rec(64 * cnt);
        if (cnt) check(plume_nullset_export(set_, cnt, rec.data(), &cnt), "plume_nullset_export");
        std::vector<plume_rustcrypto::AffinePoint> out(cnt);
        for (uint64_t i = 0; i < cnt; i++) out[i] = plume_rustcrypto::AffinePoint::from_bytes64(&rec[64 * i]);
        return out;
    }

  private:
    static Bytes pack(const std::vector<plume_rustcrypto::AffinePoint>& pts) {
        Bytes b(64 * pts.size());
        for (size_t i = 0; i < pts.size(); i++) std::memcpy(&b[64 * i], pts[i].xy.data(), 64);
        return b;
    }
    void* set_ = nullptr;
};

}  // namespace plume_hip

// ================================================================================================ plume_arkworks shape
namespace plume_arkworks {
using plume_hip::Bytes;
using plume_hip::Bytes32;
using plume_hip::Engine;
using Affine = plume_rustcrypto::AffinePoint;          // secp256k1::Affine

struct HashToCurveError : std::runtime_error { using std::runtime_error::runtime_error; };

// secp256k1::Fr: an element of the scalar field, reduced, zero included
class Fr {
  public:
    Fr() : v_{} {}
    static Fr from_be_bytes_mod_order(const uint8_t* b, size_t len) { Fr f; f.v_ = plume_hip::reduce_mod_n(b, len); return f; }
    static Fr from_be_bytes_mod_order(const Bytes& b) { return from_be_bytes_mod_order(b.data(), b.size()); }
    static Fr from_hex(const std::string& h) { return from_be_bytes_mod_order(plume_hip::from_hex(h)); }   // tests.rs:94-106 hex_to_fr
    // Fr::rand: 48 random bytes reduced (bias < 2^-128), the width hash_to_field uses
    template <class Rng> static Fr rand(Rng& rng) { uint8_t b[48]; rng.fill_bytes(b, sizeof b); Fr f = from_be_bytes_mod_order(b, sizeof b); volatile uint8_t* w = b; for (size_t i = 0; i < sizeof b; i++) w[i] = 0; return f; }
    const Bytes32& to_bytes_be() const { return v_; }
    bool is_zero() const { return plume_hip::is_zero32(v_); }
    void zeroize() { volatile uint8_t* w = v_.data(); for (size_t i = 0; i < 32; i++) w[i] = 0; }
    bool operator==(const Fr& o) const { return v_ == o.v_; }
    bool operator!=(const Fr& o) const { return v_ != o.v_; }

  private:
    Bytes32 v_;
};

enum class PlumeVersion { V1 = 1, V2 = 2 };             // rust-arkworks/src/lib.rs:66-69
using PublicKey = Affine;                                // lib.rs:216
using SecretKeyMaterial = Fr;                            // lib.rs:218

// sec1_affine (rust-arkworks/src/lib.rs:76-88): None for the identity
inline std::optional<std::array<uint8_t, 33>> sec1_affine(const Affine& a) {
    if (a.is_identity()) return std::nullopt;
    std::array<uint8_t, 33> w;
    w[0] = (uint8_t)(2 + (a.xy[63] & 1));
    std::memcpy(w.data() + 1, a.xy.data(), 32);
    return w;
}

// rust-arkworks/src/lib.rs:185-191
struct PlumeSignaturePublic {
    Bytes message;
    Fr s;
    Affine nullifier;
    std::optional<PlumeVersion> variant;
};
// rust-arkworks/src/lib.rs:194-214: the witness; zeroized on drop like the reference's
struct PlumeSignaturePrivate {
    Affine hashed_to_curve_r;
    Affine r_point;
    Fr digest_private;
    PlumeVersion variant;
    void zeroize() { digest_private.zeroize(); hashed_to_curve_r = Affine{}; r_point = Affine{}; }
    ~PlumeSignaturePrivate() { zeroize(); }
    PlumeSignaturePrivate(const Affine& hr, const Affine& rp, const Fr& d, PlumeVersion v) : hashed_to_curve_r(hr), r_point(rp), digest_private(d), variant(v) {}
    PlumeSignaturePrivate(const PlumeSignaturePrivate&) = default;
    PlumeSignaturePrivate& operator=(const PlumeSignaturePrivate&) = default;
};
using Signature = std::pair<PlumeSignaturePublic, PlumeSignaturePrivate>;

// hash_to_curve(message, pk) (rust-arkworks/src/lib.rs:90-106): Err for pk = identity
inline Affine hash_to_curve(const Bytes& message, const Affine& pk, Engine& eng = Engine::shared()) {
    if (pk.is_identity()) throw HashToCurveError("`pk` shouldn't be the identity element");
    return plume_rustcrypto::hash_to_curve(message, pk, eng);
}

// keygen (rust-arkworks/src/tests.rs:119-124): sk = Fr::rand, pk = sk * G (on the GPU)
template <class Rng>
std::pair<PublicKey, SecretKeyMaterial> keygen(Rng& rng, Engine& eng = Engine::shared()) {
    for (;;) {
        const Fr sk = Fr::rand(rng);
        if (sk.is_zero()) continue;
        uint8_t der[109], st = 0;
        plume_hip::check(plume_scalars_to_sec1_der_batch(eng.ctx(), 1, sk.to_bytes_be().data(), der, &st), "plume_scalars_to_sec1_der_batch");
        return {Affine::from_bytes64(der + 45), sk};
    }
}

// batch twin of sign_with_r: signature i from (pk_i, sk_i), message i, r_i.  pk is supplied, not recomputed; c is reduced mod n and never rejected.
inline std::vector<Signature> sign_with_r_batch(const std::vector<std::pair<PublicKey, SecretKeyMaterial>>& keypairs, const std::vector<Bytes>& messages, const std::vector<Fr>& r_scalars,
                                                PlumeVersion version, Engine& eng = Engine::shared()) {
    const size_t n = keypairs.size();
    if (messages.size() != n || r_scalars.size() != n) throw std::invalid_argument("keypairs, messages and r_scalars must have one entry per signature");
    plume_hip::PackedMessages m;
    Bytes sk(32 * n), r(32 * n), pkin(64 * n), nul(64 * n), c(32 * n), s(32 * n), rp(64 * n), hr(64 * n), st(n);
    for (size_t i = 0; i < n; i++) {
        if (keypairs[i].first.is_identity()) throw HashToCurveError("`pk` shouldn't be the identity element");   // lib.rs:99-101
        m.push(messages[i].data(), messages[i].size());
        std::memcpy(&pkin[64 * i], keypairs[i].first.xy.data(), 64);
        std::memcpy(&sk[32 * i], keypairs[i].second.to_bytes_be().data(), 32);
        std::memcpy(&r[32 * i], r_scalars[i].to_bytes_be().data(), 32);
    }
    std::vector<Signature> out;
    if (n == 0) return out;
    const int rc = plume_sign_batch(eng.ctx(), (int)version, n, m.data(), m.off.data(), sk.data(), r.data(), pkin.data(), nullptr, nul.data(), c.data(), s.data(), rp.data(), hr.data(), st.data());
    { volatile uint8_t* w = sk.data(); for (size_t i = 0; i < sk.size(); i++) w[i] = 0; }
    { volatile uint8_t* w = r.data(); for (size_t i = 0; i < r.size(); i++) w[i] = 0; }
    plume_hip::check(rc, "plume_sign_batch");
    out.reserve(n);
    for (size_t i = 0; i < n; i++) {
        if (st[i] & PLUME_STATUS_SELFCHECK_FAILED) throw plume_hip::SelfCheckError("the signature does not verify under the supplied pk and was withheld (plume_set_sign_selfcheck)");
        // Fr holds zero, so a zero sk / r is a value here; the engine's k256-shaped status bits are not errors of this API, except an off-curve pk
        if ((st[i] & PLUME_STATUS_BAD_SCALAR) && !keypairs[i].second.is_zero() && !r_scalars[i].is_zero()) throw HashToCurveError("`pk` is not a point of the curve");
        out.emplace_back(PlumeSignaturePublic{messages[i], Fr::from_be_bytes_mod_order(&s[32 * i], 32), Affine::from_bytes64(&nul[64 * i]), version},
                         PlumeSignaturePrivate(Affine::from_bytes64(&hr[64 * i]), Affine::from_bytes64(&rp[64 * i]), Fr::from_be_bytes_mod_order(&c[32 * i], 32), version));
    }
    return out;
}
// sign_with_r (rust-arkworks/src/lib.rs:229-278)
inline Signature sign_with_r(const std::pair<const PublicKey&, const SecretKeyMaterial&>& keypair, const Bytes& message, const Fr& r_scalar, PlumeVersion version,
                             Engine& eng = Engine::shared()) {
    return std::move(sign_with_r_batch({{keypair.first, keypair.second}}, {message}, {r_scalar}, version, eng)[0]);
}
// sign (rust-arkworks/src/lib.rs:281-291): r = Fr::rand(rng)
template <class Rng>
Signature sign(Rng& rng, const std::pair<const PublicKey&, const SecretKeyMaterial&>& keypair, const Bytes& message, PlumeVersion version, Engine& eng = Engine::shared()) {
    return sign_with_r(keypair, message, Fr::rand(rng), version, eng);
}

// verify_non_zk (rust-arkworks/src/tests.rs:28-78), batched: c' from the GIVEN r_point / hashed_to_curve_r, both equations for V1 and V2, c' == digest_private.
// Result i: 1 = Ok(true), 0 = Ok(false), 2 = Err(HashToCurveError).
inline Bytes verify_non_zk_batch(const std::vector<Signature>& sigs, const std::vector<PublicKey>& pks, const std::vector<Bytes>& messages, PlumeVersion version,
                                 Engine& eng = Engine::shared()) {
    const size_t n = sigs.size();
    if (pks.size() != n || messages.size() != n) throw std::invalid_argument("sigs, pks and messages must have one entry per signature");
    plume_hip::PackedMessages m;
    Bytes pk(64 * n), nul(64 * n), s(32 * n), rp(64 * n), hr(64 * n), d(32 * n), ok(n);
    for (size_t i = 0; i < n; i++) {
        m.push(messages[i].data(), messages[i].size());
        std::memcpy(&pk[64 * i], pks[i].xy.data(), 64);
        std::memcpy(&nul[64 * i], sigs[i].first.nullifier.xy.data(), 64);
        std::memcpy(&s[32 * i], sigs[i].first.s.to_bytes_be().data(), 32);
        std::memcpy(&rp[64 * i], sigs[i].second.r_point.xy.data(), 64);
        std::memcpy(&hr[64 * i], sigs[i].second.hashed_to_curve_r.xy.data(), 64);
        std::memcpy(&d[32 * i], sigs[i].second.digest_private.to_bytes_be().data(), 32);
    }
    if (n) plume_hip::check(plume_verify_non_zk_batch(eng.ctx(), (int)version, n, m.data(), m.off.data(), pk.data(), nul.data(), s.data(), rp.data(), hr.data(), d.data(), ok.data()),
                            "plume_verify_non_zk_batch");
    return ok;
}
// the reference's signature takes `pp` (Parameters{g_point}); the generator is fixed in the engine
inline bool verify_non_zk(const Signature& sig, const PublicKey& pk, const Bytes& message, PlumeVersion version, Engine& eng = Engine::shared()) {
    const uint8_t r = verify_non_zk_batch({sig}, {pk}, {message}, version, eng)[0];
    if (r == 2) throw HashToCurveError("`pk` shouldn't be the identity element");
    return r == 1;
}

}  // namespace plume_arkworks
#endif  // PLUME_HPP
