// The C++ façade of the derived-nonce signer (include/plume.hpp: PlumeSigner::sign_deterministic, sign_batch_deterministic) on a GPU: signatures verify, the same
// inputs give the same signature, the hedging input and the variant change it.  Built with g++ -std=c++17 -lplume_hip by tests/test_gpu_sign_rfc6979.py.
// Prints "rfc6979_test ok".
#include <cstdio>
#include <vector>

#include "plume.hpp"

#define REQUIRE(c)                                                                                   \
    do {                                                                                             \
        if (!(c)) { std::printf("rfc6979_test: %s:%d: %s\n", __FILE__, __LINE__, #c); return 2; } \
    } while (0)

int main() {
    try {
        plume_hip::Engine eng(0);
        plume_hip::Bytes32 kb{};
        kb[0] = 0x51; kb[31] = 0x07;
        const auto sk = *plume_rustcrypto::SecretKey::from_bytes(kb);
        const plume_hip::Bytes msg = {'a', 'n', ' ', 'e', 'x', 'a', 'm', 'p', 'l', 'e'};
        plume_hip::Bytes32 aux{};
        aux[5] = 0xAA;
        for (bool v1 : {true, false}) {
            const plume_rustcrypto::PlumeSigner signer(sk, v1);
            const auto a = signer.sign_deterministic(msg, std::nullopt, eng), b = signer.sign_deterministic(msg, std::nullopt, eng);
            REQUIRE(a.verify(eng) && b.verify(eng));
            REQUIRE(a.c.to_bytes() == b.c.to_bytes() && a.s.to_bytes() == b.s.to_bytes() && a.nullifier.xy == b.nullifier.xy);
            const auto h = signer.sign_deterministic(msg, aux, eng);
            REQUIRE(h.verify(eng) && h.s.to_bytes() != a.s.to_bytes());
        }
        const auto v1 = plume_rustcrypto::PlumeSigner(sk, true).sign_deterministic(msg, std::nullopt, eng);
        const auto v2 = plume_rustcrypto::PlumeSigner(sk, false).sign_deterministic(msg, std::nullopt, eng);
        REQUIRE(v1.s.to_bytes() != v2.s.to_bytes());
        std::vector<plume_rustcrypto::SecretKey> keys;
        std::vector<plume_hip::Bytes> msgs;
        for (int i = 0; i < 40; i++) { plume_hip::Bytes32 b{}; b[0] = 0x22; b[31] = (uint8_t)(i + 1); keys.push_back(*plume_rustcrypto::SecretKey::from_bytes(b)); msgs.push_back(plume_hip::Bytes(i, (uint8_t)i)); }
        const auto batch = plume_rustcrypto::sign_batch_deterministic(keys, msgs, true, {}, eng);
        const auto ok = plume_rustcrypto::verify_batch(batch, eng);
        for (bool o : ok) REQUIRE(o);
    } catch (const std::exception& e) {
        std::printf("rfc6979_test: exception %s\n", e.what());
        return 3;
    }
    std::printf("rfc6979_test ok\n");
    return 0;
}
