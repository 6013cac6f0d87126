// The C++ façade of the ECDSA recovery (include/plume.hpp: ecdsa_recover, ecdsa_recover_address) on a GPU, and the C ABI below it once.
// usage: ecdsa_recover_test VECTORS.  VECTORS is written by tests/test_gpu_ecdsa_recover_facades.py from tests/golden/ecdsa_recover_kats.json and the restatement of
// tests/_ecdsa.py: one item per line, "hash r s v pk address" in hex (v in decimal), pk and address "-" for an item that recovers nothing.  A genuine item must give its
// key and address; an invalid one must throw SignatureError from both functions.
// Built with g++ -std=c++17 -lplume_hip by that test.  Prints "ecdsa_recover_test ok".
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "plume.hpp"

#define REQUIRE(c)                                                                                         \
    do {                                                                                                   \
        if (!(c)) { std::printf("ecdsa_recover_test: %s:%d: %s\n", __FILE__, __LINE__, #c); return 2; } \
    } while (0)

template <class F>
static bool throws_signature_error(F f) {
    try { (void)f(); } catch (const plume_rustcrypto::SignatureError&) { return true; }
    return false;
}
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
        int valid = 0, invalid = 0;
        while (std::getline(in, line)) {
            std::istringstream ls(line);
            std::string h, r, s, pk, addr;
            int v = 0;
            if (!(ls >> h >> r >> s >> v >> pk >> addr)) continue;
            const plume_hip::Bytes32 hb = b32(h), rb = b32(r), sb = b32(s);
            if (pk == "-") {
                REQUIRE(throws_signature_error([&] { return ecdsa_recover(hb, rb, sb, (uint8_t)v, eng); }));
                REQUIRE(throws_signature_error([&] { return ecdsa_recover_address(hb, rb, sb, (uint8_t)v, eng); }));
                invalid++;
                continue;
            }
            const plume_hip::Bytes wpk = plume_hip::from_hex(pk), wad = plume_hip::from_hex(addr);
            REQUIRE(wpk.size() == 64 && wad.size() == 20);
            const auto got = ecdsa_recover(hb, rb, sb, (uint8_t)v, eng);
            REQUIRE(std::equal(wpk.begin(), wpk.end(), got.first.xy.begin()) && std::equal(wad.begin(), wad.end(), got.second.begin()));
            const std::array<uint8_t, 20> only = ecdsa_recover_address(hb, rb, sb, (uint8_t)v, eng);
            REQUIRE(only == got.second);
            if (valid == 0) {                                   // the C ABI once: SEC1 key, EIP-55 address, a wrong expect, the low-s flag, a bad format
                uint8_t pk33[33], eip[42], st = 0xFF, vb = (uint8_t)v;
                std::array<uint8_t, 20> expect = only;
                expect[19] ^= 1;
                REQUIRE(plume_ecdsa_recover_batch(eng.ctx(), 0, PLUME_ETH_PK_SEC1, PLUME_ETH_ADDR_EIP55, 1, hb.data(), rb.data(), sb.data(), &vb, expect.data(), pk33, eip, &st) == 0);
                REQUIRE(st == PLUME_ECDSA_MISMATCH && pk33[0] == 2 + (wpk[63] & 1) && std::equal(wpk.begin(), wpk.begin() + 32, pk33 + 1) && eip[0] == '0' && eip[1] == 'x');
                REQUIRE(plume_ecdsa_recover_batch(eng.ctx(), 2, PLUME_ETH_PK_SEC1, PLUME_ETH_ADDR_EIP55, 1, hb.data(), rb.data(), sb.data(), &vb, nullptr, pk33, eip, &st) == PLUME_ERR_ARG);
                REQUIRE(plume_ecdsa_recover_batch(eng.ctx(), PLUME_ECDSA_LOW_S, 2, PLUME_ETH_ADDR_EIP55, 1, hb.data(), rb.data(), sb.data(), &vb, nullptr, pk33, eip, &st) == PLUME_ERR_ARG);
                REQUIRE(plume_ecdsa_recover_batch(eng.ctx(), 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
            }
            valid++;
        }
        REQUIRE(valid >= 4 && invalid >= 3);
    } catch (const std::exception& e) {
        std::printf("ecdsa_recover_test: exception %s\n", e.what());
        return 3;
    }
    std::printf("ecdsa_recover_test ok\n");
    return 0;
}
