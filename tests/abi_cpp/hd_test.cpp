// The C++ façade of the key derivation (include/plume.hpp: parse_path, hd_master, hd_derive, hd_derive_pub, hd_address, parse_xprv, parse_xpub) on a GPU.
// usage: hd_test VECTORS.  VECTORS is written by tests/test_gpu_hd_facades.py from the restatement (tests/_hd.py), one item per line, in hex:
//   "master seed sk chain"            hd_master
//   "priv sk chain path sk' chain' address"   hd_derive / hd_address below a private node
//   "pub pk64 chain path pk64' chain' address"  hd_derive_pub / hd_address below a public node
//   "xprv string depth child chain sk"   parse_xprv        "badx string"   parse_xprv throws
//   "badpath path"                    parse_path throws
// Built with g++ -std=c++17 -lplume_hip by that test.  Prints "hd_test ok".
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "plume.hpp"

#define REQUIRE(c)                                                                            \
    do {                                                                                      \
        if (!(c)) { std::printf("hd_test: %s:%d: %s\n", __FILE__, __LINE__, #c); return 2; } \
    } while (0)

template <class E, class F>
static bool throws(F f) {
    try { f(); } catch (const E&) { return true; }
    return false;
}
static plume_hip::Bytes32 b32(const std::string& hex) {
    const plume_hip::Bytes b = plume_hip::from_hex(hex);
    plume_hip::Bytes32 a{};
    if (b.size() == 32) std::copy(b.begin(), b.end(), a.begin());
    return a;
}
template <class A>
static bool same(const A& a, const std::string& hex) {
    const plume_hip::Bytes b = plume_hip::from_hex(hex);
    return b.size() == a.size() && std::equal(a.begin(), a.end(), b.begin());
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
            std::vector<std::string> f;
            for (std::string w; ls >> w;) f.push_back(w);
            if (f.empty()) continue;
            if (f[0] == "master") {
                REQUIRE(f.size() == 4);
                const plume_hip::Bytes seed = plume_hip::from_hex(f[1]);
                const HdNode m = hd_master(seed.data(), seed.size(), eng);
                REQUIRE(same(m.sk.to_bytes(), f[2]) && same(m.chain, f[3]));
            } else if (f[0] == "priv") {
                REQUIRE(f.size() == 7);
                const auto sk = SecretKey::from_hex(f[1]);
                REQUIRE(sk.has_value());
                const HdNode c = hd_derive(*sk, b32(f[2]), f[3], eng);
                REQUIRE(same(c.sk.to_bytes(), f[4]) && same(c.chain, f[5]) && same(hd_address(*sk, b32(f[2]), f[3], eng), f[6]));
            } else if (f[0] == "pub") {
                REQUIRE(f.size() == 7);
                const plume_hip::Bytes pk = plume_hip::from_hex(f[1]);
                REQUIRE(pk.size() == 64);
                const AffinePoint P = AffinePoint::from_bytes64(pk.data());
                const HdPubNode c = hd_derive_pub(P, b32(f[2]), f[3], eng);
                REQUIRE(same(c.pk.xy, f[4]) && same(c.chain, f[5]) && same(hd_address(P, b32(f[2]), f[3], eng), f[6]));
                REQUIRE(throws<SignatureError>([&] { (void)hd_derive_pub(P, b32(f[2]), "0'", eng); }));       // a public key has no hardened children
            } else if (f[0] == "xprv") {
                REQUIRE(f.size() == 6);
                const ExtendedKey k = parse_xprv(f[1]);
                REQUIRE(k.depth == std::stoul(f[2]) && k.child_number == std::stoul(f[3]) && same(k.chain, f[4]));
                REQUIRE(k.key[0] == 0 && std::equal(k.key.begin() + 1, k.key.end(), plume_hip::from_hex(f[5]).begin()));
                REQUIRE(throws<std::invalid_argument>([&] { (void)parse_xpub(f[1]); }));                      // the other version bytes
            } else if (f[0] == "badx") {
                REQUIRE(throws<std::invalid_argument>([&] { (void)parse_xprv(f[1]); }));
            } else if (f[0] == "badpath") {
                REQUIRE(throws<std::invalid_argument>([&] { (void)parse_path(f.size() > 1 ? f[1] : std::string()); }));
            } else {
                REQUIRE(false);
            }
            seen++;
        }
        REQUIRE(seen >= 12);
        REQUIRE((parse_path("m/44'/60h/0'/0/3") == std::vector<uint32_t>{0x8000002Cu, 0x8000003Cu, 0x80000000u, 0u, 3u}));
        REQUIRE((parse_path("0/3") == std::vector<uint32_t>{0u, 3u}));
        const plume_hip::Bytes32 zero{};
        REQUIRE(throws<SignatureError>([&] { const uint8_t seed[8] = {0}; (void)hd_master(seed, 16, eng); }) == false);   // (any 16 bytes are a seed)
        REQUIRE(throws<plume_hip::Error>([&] { const uint8_t seed[8] = {0}; (void)hd_master(seed, 8, eng); }));        // seed_len below 16: the ABI's argument error
        (void)zero;
        std::printf("hd_test ok\n");
        return 0;
    } catch (const std::exception& e) {
        std::printf("hd_test: exception: %s\n", e.what());
        return 3;
    }
}
