// The C++ façade of the transaction calls (include/plume.hpp: tx_signing_hash, tx_sender, tx_sender_address) on a GPU, and the C ABI below it once.
// usage: eth_tx_test VECTORS.  VECTORS is written by tests/test_gpu_eth_tx_facades.py from tests/golden/eth_tx_kats.json: one item per line, "kind raw hash address" in
// hex -- kind ok (EIP-155's worked example first, then one item of each kind), bad (framing-invalid: every form throws SignatureError), nosender (framing-valid, r = 0: the
// hash comes out, tx_sender throws), highs (a sender without the EIP-2 rule, none with it).
// Built with g++ -std=c++17 -lplume_hip by that test.  Prints "eth_tx_test ok".
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "plume.hpp"

#define REQUIRE(c)                                                                                  \
    do {                                                                                            \
        if (!(c)) { std::printf("eth_tx_test: %s:%d: %s\n", __FILE__, __LINE__, #c); return 2; } \
    } while (0)

template <class F>
static bool throws_signature_error(F f) {
    try { f(); } catch (const plume_rustcrypto::SignatureError&) { return true; }
    return false;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    try {
        using namespace plume_rustcrypto;
        plume_hip::Engine eng(0);
        std::ifstream in(argv[1]);
        std::string line;
        int ok = 0, bad = 0, other = 0;
        while (std::getline(in, line)) {
            std::istringstream ls(line);
            std::string kind, raw_hex, hash_hex, addr_hex;
            if (!(ls >> kind >> raw_hex >> hash_hex >> addr_hex)) continue;
            const plume_hip::Bytes raw = plume_hip::from_hex(raw_hex);
            const uint8_t* p = raw.data();
            const size_t len = raw.size();
            if (kind == "bad") {
                REQUIRE(throws_signature_error([&] { (void)tx_signing_hash(p, len, eng); }));
                REQUIRE(throws_signature_error([&] { (void)tx_sender(p, len, eng); }));
                REQUIRE(throws_signature_error([&] { (void)tx_sender_address(p, len, eng); }));
                bad++;
                continue;
            }
            const plume_hip::Bytes want_hash = plume_hip::from_hex(hash_hex);
            const plume_hip::Bytes32 h = tx_signing_hash(p, len, eng);
            REQUIRE(want_hash.size() == 32 && std::equal(h.begin(), h.end(), want_hash.begin()));
            if (kind == "nosender") {
                REQUIRE(throws_signature_error([&] { (void)tx_sender(p, len, eng); }));
                REQUIRE(throws_signature_error([&] { (void)tx_sender_address(p, len, eng, false); }));
                other++;
                continue;
            }
            const plume_hip::Bytes want_addr = plume_hip::from_hex(addr_hex);
            REQUIRE(want_addr.size() == 20);
            if (kind == "highs") {
                REQUIRE(throws_signature_error([&] { (void)tx_sender(p, len, eng); }));
                const auto a = tx_sender_address(p, len, eng, false);
                REQUIRE(std::equal(a.begin(), a.end(), want_addr.begin()));
                other++;
                continue;
            }
            const auto who = tx_sender(p, len, eng);
            REQUIRE(std::equal(who.second.begin(), who.second.end(), want_addr.begin()));
            REQUIRE(tx_sender_address(p, len, eng) == who.second);
            plume_hip::Bytes32 r{}, s{};
            uint8_t v = 0xFF, type = 0xFF, st = 0xFF;
            uint64_t chain = ~0ull;
            const uint64_t off[2] = {0, (uint64_t)len};
            plume_hip::Bytes32 h2{};
            REQUIRE(plume_eth_tx_parse_batch(eng.ctx(), 1, p, off, h2.data(), r.data(), s.data(), &v, &chain, &type, &st) == 0);
            REQUIRE(st == PLUME_ETH_TX_OK && h2 == h && v <= 1 && type <= 4);
            REQUIRE(ecdsa_recover(h, r, s, v, eng).first == who.first);                    // the same key by the two calls
            if (ok == 0) {                                                                  // the C ABI once, on EIP-155's example: chain 1, legacy; flags, formats, n = 0, a missing output
                REQUIRE(chain == 1 && type == 0 && v == 0 && len == 110);
                uint8_t pk[64], addr[20];
                REQUIRE(plume_eth_tx_sender_batch(eng.ctx(), 2, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, 1, p, off, nullptr, pk, addr, nullptr, nullptr, &st) == PLUME_ERR_ARG);
                REQUIRE(plume_eth_tx_sender_batch(eng.ctx(), 0, 2, PLUME_ETH_ADDR_RAW20, 1, p, off, nullptr, pk, addr, nullptr, nullptr, &st) == PLUME_ERR_ARG);
                REQUIRE(plume_eth_tx_sender_batch(eng.ctx(), 0, PLUME_ETH_PK_AFFINE64, 3, 1, p, off, nullptr, pk, addr, nullptr, nullptr, &st) == PLUME_ERR_ARG);
                REQUIRE(plume_eth_tx_sender_batch(eng.ctx(), 0, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, 1, p, off, nullptr, nullptr, nullptr, &chain, &type, nullptr) == PLUME_ERR_ARG);
                REQUIRE(plume_eth_tx_parse_batch(eng.ctx(), 1, p, off, h2.data(), r.data(), s.data(), nullptr, nullptr, nullptr, nullptr) == PLUME_ERR_ARG);
                REQUIRE(plume_eth_tx_sender_batch(eng.ctx(), 0, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
                REQUIRE(plume_eth_tx_parse_batch(eng.ctx(), 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
                REQUIRE(plume_eth_tx_sender_batch(eng.ctx(), PLUME_ECDSA_LOW_S, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, 1, p, off, addr, pk, nullptr, nullptr, nullptr, &st) == 0);
                REQUIRE(st == PLUME_ECDSA_MISMATCH);                                        // (addr was never written: it is not the sender's)
                REQUIRE(plume_eth_tx_sender_batch(eng.ctx(), PLUME_ECDSA_LOW_S, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, 1, p, off, who.second.data(), nullptr, nullptr, &chain, &type, &st) == 0);
                REQUIRE(st == PLUME_ECDSA_MATCH && chain == 1 && type == 0);
            }
            ok++;
        }
        REQUIRE(ok == 7 && bad >= 5 && other == 2);
    } catch (const std::exception& e) {
        std::printf("eth_tx_test: exception %s\n", e.what());
        return 3;
    }
    std::printf("eth_tx_test ok\n");
    return 0;
}
