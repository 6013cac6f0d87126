// TEST INFRASTRUCTURE ONLY.  The derived-nonce lane body of csrc/plume_nonce.h compiled for the host (tests/test_nonce_lanes.py builds this with ASan + UBSan and
// compares every answer with the Python oracle, tests/_rfc6979.py).  Reads cases from a file, one answer line per case:
//   K <cap> <q> <x> <h1> <aux|->     ->  <k> <used>                 rfc6979_k for any 256-bit q with its top bit set; cap 16 (the product's) or 4
//   B <version> <n> <aux 0|1> <pk 0|1> <msgs_bytes>                 a batch through sign_nonce, its lanes in a random order, every buffer exactly sized
//     <msgs hex|->  <n + 1 offsets>  then n lines <sk> <aux|-> <pk|->   ->  n lines <h1 of the accepted span> <r> <used>
//   nonce_lanes <case file> <seed>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "plume_nonce.h"

using namespace plume;

#define REQUIRE(c)                                                                                               \
    do {                                                                                                         \
        if (!(c)) { std::fprintf(stderr, "nonce_lanes: %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(2); } \
    } while (0)

static std::vector<uint8_t> unhex(const std::string& s) {
    if (s == "-") return {};
    REQUIRE(s.size() % 2 == 0);
    std::vector<uint8_t> v(s.size() / 2);
    for (size_t i = 0; i < v.size(); i++) v[i] = (uint8_t)std::stoul(s.substr(2 * i, 2), nullptr, 16);
    return v;
}
static std::string hex(const uint8_t* p, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; i++) { s += d[p[i] >> 4]; s += d[p[i] & 15]; }
    return s;
}
static void words(uint32_t w[8], const std::string& s) {
    const std::vector<uint8_t> b = unhex(s);
    REQUIRE(b.size() == 32);
    for (int j = 0; j < 8; j++) w[j] = (uint32_t)b[4 * j] << 24 | (uint32_t)b[4 * j + 1] << 16 | (uint32_t)b[4 * j + 2] << 8 | b[4 * j + 3];
}
static std::string hexw(const uint32_t w[8]) {
    uint8_t b[32];
    for (int j = 0; j < 8; j++) for (int k = 0; k < 4; k++) b[4 * j + k] = (uint8_t)(w[j] >> (24 - 8 * k));
    return hex(b, 32);
}
// exactly-sized heap copies (ASan sees a read past the end); 4-byte aligned as the kernel's loads need
static std::unique_ptr<uint8_t[]> exact(const std::vector<uint8_t>& v) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[v.size() ? v.size() : 1]);
    if (!v.empty()) std::memcpy(p.get(), v.data(), v.size());
    return p;
}

int main(int argc, char** argv) {
    REQUIRE(argc == 3);
    std::ifstream in(argv[1]);
    REQUIRE(in.good());
    std::mt19937_64 rng(std::strtoull(argv[2], nullptr, 10));
    std::string kind;
    size_t cases = 0;
    while (in >> kind) {
        if (kind == "K") {
            int cap;
            std::string qs, xs, hs, as;
            in >> cap >> qs >> xs >> hs >> as;
            uint32_t q[8], x[8], h1[8], aux[8], k[8];
            words(q, qs); words(x, xs); words(h1, hs);
            if (as != "-") words(aux, as);
            REQUIRE(cap == 16 || cap == 4);
            const uint32_t used = cap == 16 ? rfc6979_k<16>(k, q, x, h1, as != "-" ? aux : nullptr) : rfc6979_k<4>(k, q, x, h1, as != "-" ? aux : nullptr);
            std::cout << hexw(k) << " " << used << "\n";
        } else {
            REQUIRE(kind == "B");
            int version, has_aux, has_pk;
            uint32_t n;
            uint64_t msgs_bytes;
            std::string ms;
            in >> version >> n >> has_aux >> has_pk >> msgs_bytes >> ms;
            std::vector<uint8_t> msgs = unhex(ms);
            REQUIRE(msgs.size() == msgs_bytes);
            std::vector<uint64_t> off(n + 1);
            for (auto& o : off) in >> o;
            std::vector<uint8_t> sk, aux, pk;
            for (uint32_t i = 0; i < n; i++) {
                std::string a, b, c;
                in >> a >> b >> c;
                std::vector<uint8_t> va = unhex(a), vb = unhex(b), vc = unhex(c);
                REQUIRE(va.size() == 32 && vb.size() == (has_aux ? 32u : 0u) && vc.size() == (has_pk ? 64u : 0u));
                sk.insert(sk.end(), va.begin(), va.end()); aux.insert(aux.end(), vb.begin(), vb.end()); pk.insert(pk.end(), vc.begin(), vc.end());
            }
            auto m = exact(msgs), s = exact(sk), x = exact(aux), p = exact(pk);
            std::unique_ptr<uint64_t[]> o(new uint64_t[n + 1]);
            std::copy(off.begin(), off.end(), o.get());
            std::unique_ptr<uint8_t[]> r(new uint8_t[32 * (size_t)n]);
            std::memset(r.get(), 0xA5, 32 * (size_t)n);
            NonceArgs a;
            a.version = version; a.n = n; a.msgs = msgs_bytes ? m.get() : nullptr; a.msg_off = o.get(); a.msgs_bytes = msgs_bytes;
            a.sk = s.get(); a.aux = has_aux ? x.get() : nullptr; a.pk_in = has_pk ? p.get() : nullptr; a.r = r.get();
            std::vector<uint32_t> perm(n), used(n);
            std::iota(perm.begin(), perm.end(), 0u);
            std::shuffle(perm.begin(), perm.end(), rng);
            for (uint32_t i : perm) used[i] = sign_nonce(a, i);
            for (uint32_t i = 0; i < n; i++) {
                uint64_t o0; uint32_t len;
                (void)msg_span(o0, len, a.msg_off, i, a.msgs_bytes);
                uint32_t h1[8];
                plume_nonce_h1(h1, version, has_pk ? a.pk_in + 64 * (size_t)i : nullptr, len ? a.msgs + o0 : nullptr, len);
                std::cout << hexw(h1) << " " << hex(r.get() + 32 * (size_t)i, 32) << " " << used[i] << "\n";
            }
        }
        cases++;
    }
    std::cout << "nonce_lanes ok " << cases << "\n";
    return 0;
}
