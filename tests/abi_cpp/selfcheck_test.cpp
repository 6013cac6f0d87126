// The C++ façade of the signer's self-check (include/plume.hpp: Engine::set_sign_selfcheck, plume_hip::SelfCheckError) on a GPU: sign_with_r with a pk that is on the curve
// but is not sk G returns a signature verify_non_zk rejects in mode 0 and throws SelfCheckError in mode 1; the right pk signs and verifies in both modes, with the same bytes.
// Built with g++ -std=c++17 -lplume_hip by tests/test_gpu_sign_selfcheck.py.  Prints "selfcheck_test ok".
#include <cstdio>
#include <vector>

#include "plume.hpp"

#define REQUIRE(c)                                                                                     \
    do {                                                                                               \
        if (!(c)) { std::printf("selfcheck_test: %s:%d: %s\n", __FILE__, __LINE__, #c); return 2; } \
    } while (0)

int main() {
    try {
        using namespace plume_arkworks;
        plume_hip::Engine eng(0);
        REQUIRE(eng.sign_selfcheck() == 0);
        plume_hip::Bytes32 kb{};
        kb[0] = 0x51; kb[31] = 0x07;
        const Fr sk = Fr::from_be_bytes_mod_order(kb.data(), 32), r = Fr::from_hex("93b9323b629f251b8f3fc2dd11f4672c5544e8230d493eceea98a90bda789808");
        const plume_hip::Bytes msg = {'a', 'n', ' ', 'e', 'x', 'a', 'm', 'p', 'l', 'e'};
        const auto key = *plume_rustcrypto::SecretKey::from_bytes(kb);
        const PublicKey right = plume_rustcrypto::PlumeSigner(key, true).sign_deterministic(msg, std::nullopt, eng).pk, wrong = Affine::GENERATOR();
        REQUIRE(right.xy != wrong.xy);
        for (PlumeVersion v : {PlumeVersion::V1, PlumeVersion::V2}) {
            const Signature bad = sign_with_r({wrong, sk}, msg, r, v, eng);
            REQUIRE(!verify_non_zk(bad, wrong, msg, v, eng));
            const Signature good0 = sign_with_r({right, sk}, msg, r, v, eng);
            eng.set_sign_selfcheck(1);
            REQUIRE(eng.sign_selfcheck() == 1);
            bool thrown = false;
            try { (void)sign_with_r({wrong, sk}, msg, r, v, eng); } catch (const plume_hip::SelfCheckError&) { thrown = true; }
            REQUIRE(thrown);
            const Signature good1 = sign_with_r({right, sk}, msg, r, v, eng);
            eng.set_sign_selfcheck(0);
            REQUIRE(verify_non_zk(good1, right, msg, v, eng));
            REQUIRE(good0.first.nullifier.xy == good1.first.nullifier.xy && good0.first.s.to_bytes_be() == good1.first.s.to_bytes_be());
        }
        bool refused = false;
        try { eng.set_sign_selfcheck(2); } catch (const plume_hip::Error& e) { refused = e.code == PLUME_ERR_ARG; }
        REQUIRE(refused && eng.sign_selfcheck() == 0);
    } catch (const std::exception& e) {
        std::printf("selfcheck_test: exception %s\n", e.what());
        return 3;
    }
    std::printf("selfcheck_test ok\n");
    return 0;
}
