// The C++ façade of the persistent nullifier set (include/plume.hpp, plume_hip::NullifierSet) against a std::set, on a GPU: nullifiers signed by the engine, with
// repeated (sk, message) pairs within and across batches; insert, contains, size, export_all into a second set, clear, and the error mapping.
// Built with g++ -std=c++17 -lplume_hip by tests/test_gpu_nullset.py.  Prints "nullset_test ok".
#include <cstdio>
#include <set>
#include <vector>

#include "plume.hpp"

using plume_rustcrypto::AffinePoint;

#define REQUIRE(c)                                                                      \
    do {                                                                                \
        if (!(c)) { std::printf("nullset_test: %s:%d: %s\n", __FILE__, __LINE__, #c); return 2; } \
    } while (0)

int main() {
    try {
        plume_hip::Engine eng(0);
        // 12 keys x 3 messages; batch b signs (key k, message m) for the pairs with (k + m + b) % 2 == 0, so pairs repeat across batches, and each batch repeats its first pair
        std::vector<plume_rustcrypto::SecretKey> keys;
        for (int k = 0; k < 12; k++) { plume_hip::Bytes32 b{}; b[31] = (uint8_t)(k + 1); b[0] = 0x11; keys.push_back(*plume_rustcrypto::SecretKey::from_bytes(b)); }
        struct Rng { uint8_t c = 1; void fill_bytes(uint8_t* p, size_t n) { for (size_t i = 0; i < n; i++) p[i] = c++ | 1; } } rng;
        plume_hip::NullifierSet set(eng);
        std::set<std::array<uint8_t, 64>> model;
        for (int b = 0; b < 3; b++) {
            std::vector<AffinePoint> nul;
            for (int k = 0; k < 12; k++)
                for (int m = 0; m < 3; m++)
                    if ((k + m + b) % 2 == 0) {
                        const plume_hip::Bytes msg{(uint8_t)'m', (uint8_t)m};
                        nul.push_back(plume_rustcrypto::PlumeSignature::sign_v1(keys[k], msg, rng, eng).nullifier);
                    }
            nul.push_back(nul.front());
            std::vector<bool> live(nul.size(), true);
            live[1] = false;
            uint64_t nf = 0;
            const std::vector<bool> fresh = set.insert(nul, live, &nf);
            uint64_t want_n = 0;
            std::set<std::array<uint8_t, 64>> seen;
            for (size_t i = 0; i < nul.size(); i++) {
                const bool want = live[i] && !model.count(nul[i].xy) && !seen.count(nul[i].xy);
                if (live[i]) seen.insert(nul[i].xy);
                REQUIRE(fresh[i] == want);
                want_n += want;
            }
            REQUIRE(nf == want_n);
            model.insert(seen.begin(), seen.end());
            REQUIRE(set.size() == model.size());
            const std::vector<bool> found = set.contains(nul);
            for (size_t i = 0; i < nul.size(); i++) REQUIRE(found[i] == (model.count(nul[i].xy) == 1));
        }
        const std::vector<AffinePoint> all = set.export_all();
        REQUIRE(all.size() == model.size());
        plume_hip::NullifierSet copy(eng, all.size());
        uint64_t nf = 0;
        copy.insert(all, {}, &nf);
        REQUIRE(nf == model.size() && copy.size() == model.size());
        for (const auto& p : all) REQUIRE(model.count(p.xy) == 1);
        set.clear();
        REQUIRE(set.size() == 0 && set.capacity() >= 64);
        REQUIRE(!set.contains(all).front());
        try { set.reserve((size_t(1) << 31) + 1); REQUIRE(false); } catch (const plume_hip::Error& e) { REQUIRE(e.code == PLUME_ERR_ARG); }
        std::printf("nullset_test ok\n");
        return 0;
    } catch (const plume_hip::Error& e) {
        std::printf("plume_hip::Error %d: %s\n", e.code, e.what());
        return e.code == PLUME_ERR_NODEV ? 3 : 1;
    }
}
