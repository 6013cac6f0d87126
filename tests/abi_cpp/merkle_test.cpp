// The single-item Merkle forms of include/plume.hpp against vectors tests/test_gpu_merkle_facades.py writes from the restatement (tests/_merkle.py).  Lines:
//   leaf ADDR20 AMOUNT32|- LEAF32                      merkle_leaf
//   tree SORT ROOT32 LEAF32...                         merkle_root; every merkle_proof passes merkle_verify, and fails with one bit flipped
//   member ROOT32 ADDR20 AMOUNT32|- PROOF32...         merkle_verify_address is true, and false for another address
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "plume.hpp"

using namespace plume_rustcrypto;

static std::vector<uint8_t> unhex(const std::string& h) {
    std::vector<uint8_t> out(h.size() / 2);
    for (size_t i = 0; i < out.size(); i++) out[i] = (uint8_t)std::stoul(h.substr(2 * i, 2), nullptr, 16);
    return out;
}
static Bytes32 b32(const std::string& h) { Bytes32 r{}; const auto v = unhex(h); if (v.size() != 32) throw std::runtime_error("32 bytes expected"); std::copy(v.begin(), v.end(), r.begin()); return r; }
static std::array<uint8_t, 20> b20(const std::string& h) { std::array<uint8_t, 20> r{}; const auto v = unhex(h); if (v.size() != 20) throw std::runtime_error("20 bytes expected"); std::copy(v.begin(), v.end(), r.begin()); return r; }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    int rows = 0;
    Engine eng(0);
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string kind, w;
        ss >> kind;
        std::vector<std::string> f;
        while (ss >> w) f.push_back(w);
        if (kind == "leaf") {
            const Bytes32 amount = f[1] == "-" ? Bytes32{} : b32(f[1]);
            if (merkle_leaf(b20(f[0]), f[1] == "-" ? nullptr : &amount, eng) != b32(f[2])) { std::printf("leaf differs: %s\n", line.c_str()); return 1; }
        } else if (kind == "tree") {
            std::vector<Bytes32> leaves;
            for (size_t k = 2; k < f.size(); k++) leaves.push_back(b32(f[k]));
            const bool sort = f[0] == "1";
            const Bytes32 root = b32(f[1]);
            if (merkle_root(leaves, sort, eng) != root) { std::printf("root differs: %s\n", line.c_str()); return 1; }
            for (size_t j = 0; j < leaves.size(); j++) {
                std::vector<Bytes32> proof = merkle_proof(leaves, j, sort, eng);
                if (!merkle_verify(leaves[j], proof, root, eng)) { std::printf("proof %zu fails\n", j); return 1; }
                if (!proof.empty()) {
                    proof[j % proof.size()][j % 32] ^= 1;
                    if (merkle_verify(leaves[j], proof, root, eng)) { std::printf("mutant %zu passes\n", j); return 1; }
                } else if (leaves.size() != 1) { std::printf("empty proof %zu\n", j); return 1; }
            }
        } else if (kind == "member") {
            const Bytes32 root = b32(f[0]), amount = f[2] == "-" ? Bytes32{} : b32(f[2]);
            std::vector<Bytes32> proof;
            for (size_t k = 3; k < f.size(); k++) proof.push_back(b32(f[k]));
            auto addr = b20(f[1]);
            if (!merkle_verify_address(addr, proof, root, f[2] == "-" ? nullptr : &amount, eng)) { std::printf("member refused: %s\n", line.c_str()); return 1; }
            addr[7] ^= 0x10;
            if (merkle_verify_address(addr, proof, root, f[2] == "-" ? nullptr : &amount, eng)) { std::printf("stranger accepted: %s\n", line.c_str()); return 1; }
        } else {
            return 2;
        }
        rows++;
    }
    if (rows < 5) return 2;
    std::printf("merkle_test ok (%d rows)\n", rows);
    return 0;
}
