// The C++ façade of the ECDSA signer (include/plume.hpp: ecdsa_sign, personal_sign, personal_recover, eth_message_hash) on a GPU, and the C ABI below it once.
// usage: ecdsa_sign_test VECTORS.  VECTORS is written by tests/test_gpu_ecdsa_sign.py from the "public" items of tests/golden/ecdsa_sign_kats.json -- the three widely
// published RFC 6979 / secp256k1 / SHA-256 vectors: one per line, "sk hash r s v" in hex (v in decimal).
// Built with g++ -std=c++17 -lplume_hip by that test.  Prints "ecdsa_sign_test ok".
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "plume.hpp"

#define REQUIRE(c)                                                                                      \
    do {                                                                                                \
        if (!(c)) { std::printf("ecdsa_sign_test: %s:%d: %s\n", __FILE__, __LINE__, #c); return 2; } \
    } while (0)

static plume_hip::Bytes32 b32(const std::string& hex) {
    const plume_hip::Bytes b = plume_hip::from_hex(hex);
    plume_hip::Bytes32 out{};
    if (b.size() == 32) std::copy(b.begin(), b.end(), out.begin());
    return out;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    try {
        using namespace plume_rustcrypto;
        plume_hip::Engine eng(0);
        std::ifstream in(argv[1]);
        std::string line;
        int seen = 0;
        while (std::getline(in, line)) {
            std::istringstream ls(line);
            std::string sk, h, r, s;
            int v = 0;
            if (!(ls >> sk >> h >> r >> s >> v)) continue;
            const auto key = SecretKey::from_bytes(b32(sk));
            REQUIRE(key.has_value());
            const plume_hip::Bytes32 hb = b32(h);
            const EcdsaSignature sig = ecdsa_sign(*key, hb, nullptr, eng);
            REQUIRE(sig.r == b32(r) && sig.s == b32(s) && sig.v == v);
            const EcdsaSignature sig27 = ecdsa_sign(*key, hb, nullptr, eng, true);
            REQUIRE(sig27.r == sig.r && sig27.s == sig.s && sig27.v == v + 27);
            const plume_hip::Bytes32 aux = b32(h);                                      // hedged: another nonce, so another r; still the signer's key
            const EcdsaSignature hedged = ecdsa_sign(*key, hb, &aux, eng);
            REQUIRE(hedged.r != sig.r);
            const AffinePoint pk = key->public_key(eng);
            REQUIRE(ecdsa_recover(hb, sig.r, sig.s, sig.v, eng).first == pk && ecdsa_recover(hb, hedged.r, hedged.s, hedged.v, eng).first == pk);
            const char* msg = "hello world";
            const auto sig65 = personal_sign(*key, reinterpret_cast<const uint8_t*>(msg), std::strlen(msg), nullptr, eng);
            REQUIRE(sig65[64] == 27 || sig65[64] == 28);
            const auto who = personal_recover(reinterpret_cast<const uint8_t*>(msg), std::strlen(msg), sig65, eng);
            REQUIRE(who.first == pk);
            if (seen == 0) {                                    // the C ABI once: the EIP-191 pin, an unknown flag, an unknown mode, n = 0
                const plume_hip::Bytes32 want = b32("d9eba16ed0ecae432b71fe008c98cc872bb4cc214d3220a36f365326cf807d68");
                REQUIRE(eth_message_hash(reinterpret_cast<const uint8_t*>(msg), std::strlen(msg), eng) == want);
                uint8_t rr[32], ss[32], vv = 0xFF, st = 0xFF;
                const uint64_t off[2] = {0, 11};
                REQUIRE(plume_ecdsa_sign_batch(eng.ctx(), 2, 1, hb.data(), key->to_bytes().data(), nullptr, rr, ss, &vv, &st) == PLUME_ERR_ARG);
                REQUIRE(plume_eth_message_hash_batch(eng.ctx(), 2, 1, reinterpret_cast<const uint8_t*>(msg), off, rr) == PLUME_ERR_ARG);
                REQUIRE(plume_ecdsa_sign_batch(eng.ctx(), 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
                REQUIRE(plume_eth_message_hash_batch(eng.ctx(), 0, 0, nullptr, nullptr, nullptr) == 0);
                const uint8_t zero[32] = {0};
                REQUIRE(plume_ecdsa_sign_batch(eng.ctx(), PLUME_ECDSA_SIGN_V27, 1, hb.data(), zero, nullptr, rr, ss, &vv, &st) == 0);
                REQUIRE(st == PLUME_STATUS_BAD_SCALAR && vv == 0 && std::all_of(rr, rr + 32, [](uint8_t b) { return b == 0; }) && std::all_of(ss, ss + 32, [](uint8_t b) { return b == 0; }));
            }
            seen++;
        }
        REQUIRE(seen == 3);
    } catch (const std::exception& e) {
        std::printf("ecdsa_sign_test: exception %s\n", e.what());
        return 3;
    }
    std::printf("ecdsa_sign_test ok\n");
    return 0;
}
