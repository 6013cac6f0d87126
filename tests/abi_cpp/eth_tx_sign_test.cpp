// The C++ façade of the transaction signer (include/plume.hpp: sign_tx) on a GPU, and the C ABI below it once.
// usage: eth_tx_sign_test VECTORS.  VECTORS is written by tests/test_gpu_eth_tx_sign_facades.py from tests/golden/eth_tx_kats.json and the restatement: one item per line,
// "kind sk unsigned raw address" in hex -- kind ok (EIP-155's worked example first, then one item of each kind: sign_tx gives raw, tx_sender of it the address), bad (an
// ill-framed item: sign_tx throws SignatureError).
// Built with g++ -std=c++17 -lplume_hip by that test.  Prints "eth_tx_sign_test ok".
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "plume.hpp"

#define REQUIRE(c)                                                                                       \
    do {                                                                                                 \
        if (!(c)) { std::printf("eth_tx_sign_test: %s:%d: %s\n", __FILE__, __LINE__, #c); return 2; } \
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
        int ok = 0, bad = 0;
        while (std::getline(in, line)) {
            std::istringstream ls(line);
            std::string kind, sk_hex, unsigned_hex, raw_hex, addr_hex;
            if (!(ls >> kind >> sk_hex >> unsigned_hex >> raw_hex >> addr_hex)) continue;
            const auto key = SecretKey::from_hex(sk_hex);
            REQUIRE(key.has_value());
            const plume_hip::Bytes u = unsigned_hex == "-" ? plume_hip::Bytes() : plume_hip::from_hex(unsigned_hex);
            if (kind == "bad") {
                REQUIRE(throws_signature_error([&] { (void)sign_tx(*key, u.data(), u.size(), nullptr, eng); }));
                bad++;
                continue;
            }
            const plume_hip::Bytes want = plume_hip::from_hex(raw_hex), want_addr = plume_hip::from_hex(addr_hex);
            const std::vector<uint8_t> raw = sign_tx(*key, u.data(), u.size(), nullptr, eng);
            REQUIRE(raw.size() == want.size() && std::equal(raw.begin(), raw.end(), want.begin()));
            const auto who = tx_sender(raw.data(), raw.size(), eng);
            REQUIRE(want_addr.size() == 20 && std::equal(who.second.begin(), who.second.end(), want_addr.begin()));
            REQUIRE(who.first == key->public_key(eng));
            plume_hip::Bytes32 aux{};
            aux[0] = 1;
            const std::vector<uint8_t> hedged = sign_tx(*key, u.data(), u.size(), &aux, eng);      // another nonce: other bytes, the same sender
            REQUIRE(hedged != raw && tx_sender_address(hedged.data(), hedged.size(), eng) == who.second);
            if (ok == 0) {                                                                          // the C ABI once, on EIP-155's example: the records, flags, n = 0, a missing output
                const uint64_t off[2] = {0, (uint64_t)u.size()};
                std::vector<uint8_t> out(plume_eth_tx_sign_out_bytes(1, u.size()), 0xAA);
                REQUIRE(out.size() == u.size() + PLUME_ETH_TX_SIGN_GROWTH);
                const plume_hip::Bytes32 skb = key->to_bytes();
                plume_hip::Bytes32 h{}, r{}, s{};
                uint32_t out_len = ~0u;
                uint8_t v = 0xFF, type = 0xFF, st = 0xFF;
                uint64_t chain = ~0ull;
                REQUIRE(plume_eth_tx_sign_batch(eng.ctx(), 0, 1, u.data(), off, skb.data(), nullptr, out.data(), &out_len, h.data(), r.data(), s.data(), &v, &chain, &type, &st) == 0);
                REQUIRE(st == 0 && out_len == raw.size() && chain == 1 && type == 0 && v == 0 && std::equal(raw.begin(), raw.end(), out.begin()));
                REQUIRE(std::all_of(out.begin() + out_len, out.end(), [](uint8_t b) { return b == 0; }));
                REQUIRE(h == tx_signing_hash(raw.data(), raw.size(), eng));
                REQUIRE(plume_eth_tx_sign_batch(eng.ctx(), 1, 1, u.data(), off, skb.data(), nullptr, out.data(), &out_len, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &st) == PLUME_ERR_ARG);
                REQUIRE(plume_eth_tx_sign_batch(eng.ctx(), 0, 1, u.data(), off, skb.data(), nullptr, out.data(), &out_len, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PLUME_ERR_ARG);
                REQUIRE(plume_eth_tx_sign_batch(eng.ctx(), 0, 1, u.data(), off, skb.data(), nullptr, nullptr, &out_len, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &st) == PLUME_ERR_ARG);
                REQUIRE(plume_eth_tx_sign_batch(eng.ctx(), 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
                const plume_hip::Bytes32 zero{};                                                    // BAD_TX is reported alone, whatever the key is; a bad key on a good item is the signer's status
                const uint8_t junk[2] = {0x05, 0xc0};
                const uint64_t joff[2] = {0, 2};
                REQUIRE(plume_eth_tx_sign_batch(eng.ctx(), 0, 1, junk, joff, zero.data(), nullptr, out.data(), &out_len, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &st) == 0);
                REQUIRE(st == PLUME_STATUS_BAD_TX && out_len == 0);
                REQUIRE(plume_eth_tx_sign_batch(eng.ctx(), 0, 1, u.data(), off, zero.data(), nullptr, out.data(), &out_len, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &st) == 0);
                REQUIRE(st == PLUME_STATUS_BAD_SCALAR && out_len == 0 && std::all_of(out.begin(), out.end(), [](uint8_t b) { return b == 0; }));
                eng.set_sign_selfcheck(1);                                                          // the self-check on: the same bytes
                const std::vector<uint8_t> checked = sign_tx(*key, u.data(), u.size(), nullptr, eng);
                eng.set_sign_selfcheck(0);
                REQUIRE(checked == raw);
            }
            ok++;
        }
        REQUIRE(ok == 7 && bad >= 5);
    } catch (const std::exception& e) {
        std::printf("eth_tx_sign_test: exception %s\n", e.what());
        return 3;
    }
    std::printf("eth_tx_sign_test ok\n");
    return 0;
}
