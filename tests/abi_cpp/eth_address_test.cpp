// The C++ façade of the Ethereum-address call (include/plume.hpp: PlumeSignature::eth_address, eth_address_eip55, verify_for_address) on a GPU: the key of sk = 1 has the
// well-known address; a signature verifies for its key's address, not for an address with one flipped bit, not with a tampered s; a pk that is no Ethereum key throws.
// Built with g++ -std=c++17 -lplume_hip by tests/test_gpu_eth_address_facades.py.  Prints "eth_address_test ok".
#include <cstdio>
#include <string>
#include <vector>

#include "plume.hpp"

#define REQUIRE(c)                                                                                       \
    do {                                                                                                 \
        if (!(c)) { std::printf("eth_address_test: %s:%d: %s\n", __FILE__, __LINE__, #c); return 2; } \
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
        kb[31] = 0x01;
        const auto one = *SecretKey::from_bytes(kb);
        const plume_hip::Bytes msg = {'a', 'n', ' ', 'e', 'x', 'a', 'm', 'p', 'l', 'e'};
        for (bool v1 : {true, false}) {
            const PlumeSignature sig = PlumeSigner(one, v1).sign_deterministic(msg, std::nullopt, eng);
            REQUIRE(sig.verify(eng));
            REQUIRE(sig.eth_address_eip55(eng) == "0x7E5F4552091A69125d5DfCb7b8C2659029395Bdf");
            const std::array<uint8_t, 20> addr = sig.eth_address(eng);
            const uint8_t want[20] = {0x7E, 0x5F, 0x45, 0x52, 0x09, 0x1A, 0x69, 0x12, 0x5d, 0x5D, 0xfC, 0xb7, 0xb8, 0xC2, 0x65, 0x90, 0x29, 0x39, 0x5B, 0xdf};
            REQUIRE(std::equal(addr.begin(), addr.end(), want));
            REQUIRE(sig.verify_for_address(addr, eng));
            for (int byte : {0, 7, 19}) {
                std::array<uint8_t, 20> other = addr;
                other[byte] ^= 0x10;
                REQUIRE(!sig.verify_for_address(other, eng));
            }
            PlumeSignature bad = sig;
            bad.s = PlumeSigner(one, !v1).sign_deterministic(msg, std::nullopt, eng).s;
            REQUIRE(!bad.verify(eng) && !bad.verify_for_address(addr, eng));             // the right address, a signature that does not verify
            bad = sig;
            bad.pk.xy[63] ^= 1;                                                       // off the curve
            REQUIRE(throws_signature_error([&] { return bad.eth_address(eng); }) && throws_signature_error([&] { return bad.eth_address_eip55(eng); }));
            REQUIRE(!bad.verify_for_address(addr, eng));
            bad.pk.xy.fill(0);                                                        // the identity: a public key for verify, no Ethereum key
            REQUIRE(throws_signature_error([&] { return bad.eth_address(eng); }) && !bad.verify_for_address(addr, eng));
        }
    } catch (const std::exception& e) {
        std::printf("eth_address_test: exception %s\n", e.what());
        return 3;
    }
    std::printf("eth_address_test ok\n");
    return 0;
}
