// The C++ façade of the seed derivation (include/plume.hpp: mnemonic_to_seed, pbkdf2_sha512) on a GPU.
// usage: kdf_test VECTORS.  VECTORS is written by tests/test_gpu_kdf_facades.py from hashlib, one item per line, the byte strings in hex ("-" for an empty one):
//   "seed mnemonic passphrase seed64"                    mnemonic_to_seed
//   "pbkdf2 password salt iterations dklen out"          pbkdf2_sha512
// Built with g++ -std=c++17 -lplume_hip by that test.  Prints "kdf_test ok".
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "plume.hpp"

#define REQUIRE(c)                                                                             \
    do {                                                                                       \
        if (!(c)) { std::printf("kdf_test: %s:%d: %s\n", __FILE__, __LINE__, #c); return 2; } \
    } while (0)

template <class E, class F>
static bool throws(F f) {
    try { f(); } catch (const E&) { return true; }
    return false;
}
static plume_hip::Bytes bytes_of(const std::string& hex) { return hex == "-" ? plume_hip::Bytes() : plume_hip::from_hex(hex); }
template <class A>
static bool same(const A& a, const std::string& hex) {
    const plume_hip::Bytes b = bytes_of(hex);
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
            if (f[0] == "seed") {
                REQUIRE(f.size() == 4);
                const plume_hip::Bytes m = bytes_of(f[1]), p = bytes_of(f[2]);
                REQUIRE(same(mnemonic_to_seed(std::string(m.begin(), m.end()), std::string(p.begin(), p.end()), eng), f[3]));
            } else if (f[0] == "pbkdf2") {
                REQUIRE(f.size() == 6);
                const plume_hip::Bytes pw = bytes_of(f[1]), salt = bytes_of(f[2]);
                REQUIRE(same(pbkdf2_sha512(pw.data(), pw.size(), salt.data(), salt.size(), (uint32_t)std::stoul(f[3]), std::stoul(f[4]), eng), f[5]));
            } else {
                REQUIRE(false);
            }
            seen++;
        }
        REQUIRE(seen >= 6);
        const uint8_t pw[2] = {'p', 'w'};
        REQUIRE(throws<plume_hip::Error>([&] { (void)pbkdf2_sha512(pw, 2, pw, 2, 0, 64, eng); }));        // the ABI's argument errors
        REQUIRE(throws<plume_hip::Error>([&] { (void)pbkdf2_sha512(pw, 2, pw, 2, 1, 65, eng); }));
        REQUIRE(throws<plume_hip::Error>([&] { (void)pbkdf2_sha512(pw, 2, pw, 2, 1, 0, eng); }));
        std::printf("kdf_test ok\n");
        return 0;
    } catch (const std::exception& e) {
        std::printf("kdf_test: exception: %s\n", e.what());
        return 3;
    }
}
