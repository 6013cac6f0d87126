// The C++ façade of the point recovery (include/plume.hpp: PlumeSignature::recover_v1specific) on a GPU: a V1 signature stripped to its four fields gets its own
// r_point and hashed_to_curve_r back and verifies again as a V1 record; a V2 signature, a tampered s and an off-curve nullifier throw SignatureError.
// Built with g++ -std=c++17 -lplume_hip by tests/test_gpu_recover_facades.py.  Prints "recover_test ok".
#include <cstdio>
#include <vector>

#include "plume.hpp"

#define REQUIRE(c)                                                                                   \
    do {                                                                                             \
        if (!(c)) { std::printf("recover_test: %s:%d: %s\n", __FILE__, __LINE__, #c); return 2; } \
    } while (0)

template <class F>
static bool throws_signature_error(F f) {
    try { (void)f(); } catch (const plume_rustcrypto::SignatureError&) { return true; }
    return false;
}

int main() {
    try {
        using namespace plume_rustcrypto;
        plume_hip::Engine eng(0);
        plume_hip::Bytes32 kb{};
        kb[0] = 0x51; kb[31] = 0x07;
        const auto key = *SecretKey::from_bytes(kb);
        const plume_hip::Bytes msg = {'a', 'n', ' ', 'e', 'x', 'a', 'm', 'p', 'l', 'e'};
        const PlumeSignature v1 = PlumeSigner(key, true).sign_deterministic(msg, std::nullopt, eng), v2 = PlumeSigner(key, false).sign_deterministic(msg, std::nullopt, eng);
        REQUIRE(v1.v1specific.has_value() && !v2.v1specific.has_value() && v1.verify(eng) && v2.verify(eng));
        PlumeSignature compact = v1;
        compact.v1specific.reset();
        REQUIRE(!compact.verify(eng));                                   // as a V2 record it does not verify: c is the V1 hash
        const PlumeSignatureV1Fields f = compact.recover_v1specific(eng);
        REQUIRE(f.r_point.xy == v1.v1specific->r_point.xy && f.hashed_to_curve_r.xy == v1.v1specific->hashed_to_curve_r.xy);
        compact.v1specific = f;
        REQUIRE(compact.verify(eng));
        REQUIRE(throws_signature_error([&] { return v2.recover_v1specific(eng); }));       // status 0: c is the V2 hash
        PlumeSignature bad = v1;
        bad.s = v2.s;
        REQUIRE(throws_signature_error([&] { return bad.recover_v1specific(eng); }));      // status 0: other points, the hash does not match
        bad = v1;
        bad.nullifier.xy[63] ^= 1;
        REQUIRE(throws_signature_error([&] { return bad.recover_v1specific(eng); }));      // status 3: off the curve
    } catch (const std::exception& e) {
        std::printf("recover_test: exception %s\n", e.what());
        return 3;
    }
    std::printf("recover_test ok\n");
    return 0;
}
