// The lane bodies of the Merkle calls (csrc/plume_merkle.h, over keccak256_lanes of csrc/plume_keccak.h) as host loops, for tests/test_merkle_lanes.py; built by the
// Makefile beside it with g++ under AddressSanitizer + UBSan and -Werror.  The grid of every kernel is a plain loop over its lanes; the sort runs the launcher's own stage
// schedule (mrk_sort_schedule) with loops over tiles and pairs in place of workgroups and lanes, a tile being a heap array of tile * 9 words; the levels run from the deepest
// depth upward as the build does.
// usage: merkle_lanes MODE IN OUT.  IN starts with eight u32: a, b, n, m, depth, mis_in, mis_out, flags; then the mode's arrays, each of exactly its bytes.  Every input
// array is copied to `mis_in` bytes into an allocation that ENDS with its last byte (a load past it is a heap overflow); every output lies at an odd offset between guards
// of 32 bytes 0xAA, and OUT holds guards and all.
//   leaf    a = leaf_format, b = addr_format; items, amounts (format 2)                                        -> leaf (32 n), status (n; absent with flags & 2)
//   build   flags & 1 = sort, flags & 2 = no leaf_pos; leaves                                                  -> tree (32 (2n - 1)), leaf_pos (4 n, 4-byte aligned)
//   proof   tree, pos (4 m)                                                                                    -> proof (32 depth m), proof_len (m)
//   verify  a, b as for leaf; items, amounts (format 2), proof (32 depth m), proof_len (m), root (32)          -> status (m)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "plume_merkle.h"

using namespace plume;

constexpr size_t kGuard = 32;
struct Out {
    uint8_t* raw;
    uint8_t* p;
    size_t len, total;
    Out(size_t bytes, size_t mis) : len(bytes), total(kGuard + 16 + bytes + kGuard) {
        void* q = nullptr;
        if (posix_memalign(&q, 16, total) != 0) std::abort();
        raw = (uint8_t*)q;
        std::memset(raw, 0xAA, total);
        p = raw + kGuard + (mis & 15u);
    }
    ~Out() { std::free(raw); }
    Out(const Out&) = delete;
    Out& operator=(const Out&) = delete;
    bool untouched_outside() const {
        for (uint8_t* b = raw; b < p; b++) if (*b != 0xAA) return false;
        for (uint8_t* b = p + len; b < raw + total; b++) if (*b != 0xAA) return false;
        return true;
    }
    void dump(FILE* o) const { std::fwrite(p - kGuard, 1, kGuard + len + kGuard, o); }
};
// an input array that ends with the allocation
struct In {
    uint8_t* raw = nullptr;
    uint8_t* p = nullptr;
    std::vector<uint8_t> copy;
    bool read(FILE* f, size_t bytes, size_t mis) {
        copy.resize(bytes);
        if (bytes && std::fread(copy.data(), 1, bytes, f) != bytes) return false;
        raw = (uint8_t*)std::malloc(mis + bytes + (mis + bytes ? 0 : 1));
        if (!raw) return false;
        p = raw + mis;
        if (bytes) std::memcpy(p, copy.data(), bytes);
        return true;
    }
    bool unchanged() const { return copy.empty() || std::memcmp(p, copy.data(), copy.size()) == 0; }
    ~In() { std::free(raw); }
};
struct Head { uint32_t a, b, n, m, depth, mis_in, mis_out, flags; };

static int finish(const char* out, std::initializer_list<const Out*> arrays, std::initializer_list<const In*> inputs) {
    int rc = 0;
    for (const In* i : inputs) if (!i->unchanged()) rc = 3;
    FILE* o = std::fopen(out, "wb");
    if (!o) return 2;
    for (const Out* x : arrays) { if (!x->untouched_outside()) rc = 4; x->dump(o); }
    std::fclose(o);
    return rc;
}

static int run_leaf(const Head& h, FILE* f, const char* out) {
    const size_t n = h.n, W = mrk_item_width((int)h.a, (int)h.b);
    In items, amounts;
    if (!items.read(f, W * n, h.mis_in) || (h.a == PLUME_MRK_LEAF_ADDRESS_UINT256 && !amounts.read(f, 32 * n, h.mis_in + 1))) return 2;
    Out leaf(32 * n, h.mis_out), st((h.flags & 2u) ? 0 : n, h.mis_out + 3);
    MerkleLeafArgs a;
    a.leaf_format = (int)h.a; a.addr_format = (int)h.b; a.n = h.n; a.in = items.p; a.amount = amounts.p; a.leaf = leaf.p; a.status = (h.flags & 2u) ? nullptr : st.p;
    for (uint32_t i = h.n; i-- > 0;) mrk_leaf_item(a, i);
    return finish(out, {&leaf, &st}, {&items, &amounts});
}

static void host_sort(const MerkleSortArgs& a) {
    const size_t tiles = a.npad / a.tile;
    std::vector<uint32_t> s((size_t)PLUME_MRK_REC_WORDS * a.tile);                        // one workgroup's LDS
    mrk_sort_schedule(a.npad, a.tile,
        [&] {
            for (size_t b = 0; b < tiles; b++) {
                const size_t base = b * a.tile;
                for (uint32_t x = 0; x < a.tile; x++) mrk_tile_from_leaves(s.data(), a, base, x);
                for (uint32_t k = 2; k <= a.tile; k <<= 1)
                    for (uint32_t j = k >> 1; j; j >>= 1)
                        for (uint32_t t = a.tile / 2u; t-- > 0;) mrk_tile_cx(s.data(), a.tile, base, k, j, t);
                for (uint32_t x = 0; x < a.tile; x++) mrk_tile_to_ws(s.data(), a, base, x);
            }
        },
        [&](size_t k, size_t j) { for (size_t t = a.npad / 2u; t-- > 0;) mrk_global_cx(a, k, j, t); },
        [&](size_t k) {
            for (size_t b = 0; b < tiles; b++) {
                const size_t base = b * a.tile;
                for (uint32_t x = 0; x < a.tile; x++) mrk_tile_from_ws(s.data(), a, base, x);
                for (uint32_t j = a.tile >> 1; j; j >>= 1)
                    for (uint32_t t = 0; t < a.tile / 2u; t++) mrk_tile_cx(s.data(), a.tile, base, k, j, t);
                for (uint32_t x = 0; x < a.tile; x++) mrk_tile_to_ws(s.data(), a, base, x);
            }
        });
}

static int run_build(const Head& h, FILE* f, const char* out) {
    const size_t n = h.n;
    if (n == 0 || n > PLUME_MRK_MAX_N) return 2;
    In leaves;
    if (!leaves.read(f, 32 * n, h.mis_in)) return 2;
    const bool sorted = (h.flags & 1u) && n > 1, want_pos = !(h.flags & 2u);
    Out tree(32 * (2 * n - 1), h.mis_out), pos(want_pos ? 4 * n : 0, 4 * (h.mis_out & 3u));
    const uint32_t npad = mrk_next_pow2(h.n);
    std::vector<uint32_t> ws(sorted ? (size_t)PLUME_MRK_REC_WORDS * npad : 0);            // exactly the workspace the library allocates
    if (sorted) {
        MerkleSortArgs sa; sa.n = h.n; sa.npad = npad; sa.tile = npad < PLUME_MRK_TILE ? npad : PLUME_MRK_TILE; sa.leaf = leaves.p; sa.ws = ws.data();
        host_sort(sa);
    }
    MerkleTreeArgs ta; ta.n = h.n; ta.npad = npad; ta.leaf = leaves.p; ta.ws = sorted ? ws.data() : nullptr; ta.tree = tree.p; ta.leaf_pos = want_pos ? (uint32_t*)pos.p : nullptr;
    for (uint32_t i = 0; i < h.n; i++) mrk_place_item(ta, i);
    if (n >= 2) {
        for (uint32_t d = mrk_parent_depth(h.n) + 1u; d-- > 0u;) {
            const uint32_t cnt = mrk_depth_nodes(h.n, d);
            if (d <= PLUME_MRK_TOP_DEPTH && cnt > 256u) return 5;                          // the fused top's workgroup would be too small
            for (uint32_t t = cnt; t-- > 0;) mrk_node(tree.p, (size_t)mrk_depth_first(d) + t);
        }
    }
    return finish(out, {&tree, &pos}, {&leaves});
}

static int run_proof(const Head& h, FILE* f, const char* out) {
    const size_t n = h.n, m = h.m;
    if (n == 0) return 2;
    In tree, pos;
    if (!tree.read(f, 32 * (2 * n - 1), h.mis_in) || !pos.read(f, 4 * m, 4 * (h.mis_in & 3u))) return 2;
    Out proof(32 * (size_t)h.depth * m, h.mis_out), len(m, h.mis_out + 1);
    MerkleProofArgs a; a.n = h.n; a.m = h.m; a.depth = h.depth; a.tree = tree.p; a.pos = (const uint32_t*)pos.p; a.proof = proof.p; a.proof_len = len.p;
    for (uint32_t k = 0; k < h.m; k++) mrk_proof_item(a, k);
    return finish(out, {&proof, &len}, {&tree, &pos});
}

static int run_verify(const Head& h, FILE* f, const char* out) {
    const size_t m = h.m, W = mrk_item_width((int)h.a, (int)h.b);
    In items, amounts, proof, len, root;
    if (!items.read(f, W * m, h.mis_in) || (h.a == PLUME_MRK_LEAF_ADDRESS_UINT256 && !amounts.read(f, 32 * m, h.mis_in + 2)) || !proof.read(f, 32 * (size_t)h.depth * m, h.mis_in + 1) ||
        !len.read(f, m, h.mis_in) || !root.read(f, 32, h.mis_in + 3))
        return 2;
    Out st(m, h.mis_out);
    MerkleVerifyArgs a;
    a.leaf_format = (int)h.a; a.addr_format = (int)h.b; a.m = h.m; a.depth = h.depth; a.in = items.p; a.amount = amounts.p; a.proof = proof.p; a.proof_len = len.p;
    a.root = root.p; a.status = st.p;
    for (uint32_t k = h.m; k-- > 0;) mrk_verify_item(a, k);
    return finish(out, {&st}, {&items, &amounts, &proof, &len, &root});
}

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: merkle_lanes leaf|build|proof|verify IN OUT\n"); return 2; }
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    Head h;
    int rc = 2;
    if (std::fread(&h, 1, sizeof h, f) == sizeof h) {
        const std::string mode = argv[1];
        rc = mode == "leaf" ? run_leaf(h, f, argv[3]) : mode == "build" ? run_build(h, f, argv[3]) : mode == "proof" ? run_proof(h, f, argv[3])
           : mode == "verify" ? run_verify(h, f, argv[3]) : 2;
    }
    std::fclose(f);
    if (rc == 0) std::printf("merkle_lanes ok\n");
    return rc;
}
