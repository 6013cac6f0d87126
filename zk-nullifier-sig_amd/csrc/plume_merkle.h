// Keccak Merkle allow-lists (plume_merkle_*, include/plume_hip.h): the tree OpenZeppelin's StandardMerkleTree builds and MerkleProof.verify checks on chain.
//     leaf       the caller's 32 bytes (HASH32), Keccak(Keccak(0^12 || addr20)) (ADDRESS) or Keccak(Keccak(0^12 || addr20 || amount32)) (ADDRESS_UINT256)
//     node       hash_pair(a, b) = Keccak-256(min(a, b) || max(a, b)), the 32-byte values compared as big-endian numbers
//     tree       2n - 1 nodes of 32 bytes: tree[2n - 2 - i] = L[i], tree[i] = hash_pair(tree[2i + 1], tree[2i + 2]) for i = n - 2 .. 0, the root is tree[0]
//     L          the input order, or with PLUME_MRK_SORT_LEAVES the input sorted ascending by (leaf bytes, input index)
// Every Keccak here is ONE absorb of whole lanes (keccak256_lanes, plume_keccak.h): 32- and 64-byte preimages, the state in registers.  Values are kept as the eight
// little-endian words of the 32 bytes in memory order; "big-endian number" comparisons therefore run on byte-swapped words, first word first, and the smaller / larger child
// is picked word by word with selects -- no byte array, no run-time index.
// Per-lane bodies only (PLUME_HD): the kernels that call them are in plume_merkle_kernels.hip, and tests/merkle runs the same bodies as host loops.
//     k_merkle_leaf     mrk_leaf_item      one lane per item
//     k_merkle_sort_*   mrk_tile_*, mrk_cx a bitonic network over records {8 key words already byte-swapped, input index}, padded to a power of two with all-ones records
//                                          (they sort last through their index, which is >= n).  Records live as NINE word arrays (structure of arrays): stride `tile` in LDS,
//                                          stride npad in the workspace, so consecutive lanes touch consecutive words.  The order is total -- indices are distinct -- so the
//                                          result is sorted(range(n), key = (leaf, index)) exactly, whatever the network's pairing
//     k_merkle_place    mrk_place_item     the sorted (or the caller's) leaves to tree[2n - 2 - i], leaf_pos[input index] = 2n - 2 - i
//     k_merkle_level    mrk_node           one lane per parent of ONE depth d: nodes [2^d - 1, min(2^(d + 1) - 2, n - 2)].  The two children are 64 contiguous bytes
//     k_merkle_top      mrk_node           the depths of at most 256 nodes (0 .. 8) in one workgroup, a barrier between depths
//     k_merkle_proof    mrk_proof_item     one lane per requested index: the siblings on the way to the root
//     k_merkle_verify   mrk_verify_item    one lane per item: the leaf, then MerkleProof.processProof.  The walk is a run-time loop whose condition is a wavefront vote
//                                          (keccak_any), as in keccak_stream_digest
// Arrays of the caller may sit at any byte offset (leaf_pos and pos: 4-byte aligned): loads are 16-byte vectors when the address allows, words or bytes otherwise, and never
// reach past the last byte of an item; 32-byte records are written by recover_store (plume_recover.h).  Everything is public data: plain branches.
#pragma once
#include "plume_keccak.h"

#define PLUME_MRK_LEAF_HASH32 0            // PLUME_MERKLE_LEAF_* (include/plume_hip.h)
#define PLUME_MRK_LEAF_ADDRESS 1
#define PLUME_MRK_LEAF_ADDRESS_UINT256 2
#define PLUME_MRK_SORT_LEAVES 1            // PLUME_MERKLE_SORT_LEAVES
#define PLUME_MRK_MISMATCH 0u              // PLUME_MERKLE_*
#define PLUME_MRK_MATCH 1u
#define PLUME_MRK_INVALID 3u
#define PLUME_MRK_BAD_LEN 255u             // PLUME_MERKLE_BAD_PROOF
#define PLUME_MRK_MAX_N (1u << 26)
#define PLUME_MRK_MAX_DEPTH 64u            // proof slots per item a caller may ask for
#define PLUME_MRK_TILE 2048u               // records of an LDS tile: 9 words each, 72 KiB -- two workgroups per CU in the 160 KiB
#define PLUME_MRK_TOP_DEPTH 8u             // the deepest depth of at most 256 nodes
#define PLUME_MRK_REC_WORDS 9u

namespace plume {

struct MerkleLeafArgs {
    int leaf_format, addr_format;     // PLUME_MRK_LEAF_*, PLUME_ETHK_ADDR_RAW20 / RECORD64
    uint32_t n;
    const uint8_t* in;                // mrk_item_width bytes per item
    const uint8_t* amount;            // 32 bytes per item, big-endian (ADDRESS_UINT256 only)
    uint8_t* leaf;                    // 32 bytes per item
    uint8_t* status;                  // 1 byte per item, or NULL
};
struct MerkleSortArgs {
    uint32_t n, npad, tile;           // npad: n rounded up to a power of two; tile = min(npad, PLUME_MRK_TILE)
    const uint8_t* leaf;
    uint32_t* ws;                     // PLUME_MRK_REC_WORDS arrays of npad words
};
struct MerkleTreeArgs {
    uint32_t n, npad;
    const uint8_t* leaf;              // the input order (ws == NULL)
    const uint32_t* ws;               // the sorted records, or NULL
    uint8_t* tree;                    // (2n - 1) * 32 bytes
    uint32_t* leaf_pos;               // n words, or NULL
};
struct MerkleProofArgs {
    uint32_t n, m, depth;
    const uint8_t* tree;
    const uint32_t* pos;              // m tree indices
    uint8_t* proof;                   // m * depth * 32 bytes
    uint8_t* proof_len;               // m bytes
};
struct MerkleVerifyArgs {
    int leaf_format, addr_format;
    uint32_t m, depth;
    const uint8_t* in;                // mrk_item_width bytes per item
    const uint8_t* amount;
    const uint8_t* proof;             // m * depth * 32 bytes
    const uint8_t* proof_len;         // m bytes
    const uint8_t* root;              // 32 bytes
    uint8_t* status;                  // m bytes
};

PLUME_HD uint32_t mrk_item_width(int leaf_format, int addr_format) {
    return leaf_format == PLUME_MRK_LEAF_HASH32 ? 32u : addr_format == PLUME_ETHK_ADDR_RECORD64 ? 64u : 20u;
}
PLUME_HD uint32_t mrk_log2(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }      // floor(log2 v), v >= 1
PLUME_HD uint32_t mrk_next_pow2(uint32_t n) { return n <= 1u ? 1u : 2u << mrk_log2(n - 1u); }
// the parents of depth d of a tree of n >= 2 leaves: `first` and the count (0: the depth holds none)
PLUME_HD uint32_t mrk_depth_first(uint32_t d) { return (1u << d) - 1u; }
PLUME_HD uint32_t mrk_depth_nodes(uint32_t n, uint32_t d) {
    const uint32_t first = mrk_depth_first(d), full = (2u << d) - 2u, last = full < n - 2u ? full : n - 2u;
    return last < first ? 0u : last - first + 1u;
}
// the depth of the deepest parent, node n - 2 (n >= 2)
PLUME_HD uint32_t mrk_parent_depth(uint32_t n) { return mrk_log2(n - 1u); }

// NW words at any alignment, never a byte past them
template <int NW>
PLUME_HD void mrk_load_words(uint32_t* w, const uint8_t* p) {
    if (NW % 4 == 0 && ((uintptr_t)p & 15u) == 0) {
        PLUME_UNROLL for (int k = 0; k < NW / 4; k++) {
            const recover_quad v = ((const recover_quad*)p)[k];
            PLUME_UNROLL for (int j = 0; j < 4; j++) w[4 * k + j] = v.w[j];
        }
    } else if (((uintptr_t)p & 3u) == 0) {
        PLUME_UNROLL for (int k = 0; k < NW; k++) w[k] = ((const uint32_t*)p)[k];
    } else {
        PLUME_UNROLL for (int k = 0; k < NW; k++) w[k] = (uint32_t)p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) | ((uint32_t)p[4 * k + 3] << 24);
    }
}

// the leaf of item i; false: a RECORD64 whose first 44 bytes are not zero -- the leaf is then all zero
PLUME_HD bool mrk_leaf(uint32_t leaf[8], int leaf_format, int addr_format, const uint8_t* in, const uint8_t* amount, size_t i) {
    if (leaf_format == PLUME_MRK_LEAF_HASH32) { mrk_load_words<8>(leaf, in + 32 * i); return true; }
    uint32_t m[16], h[8];
    PLUME_UNROLL for (int k = 0; k < 16; k++) m[k] = 0u;                                  // abi.encode(address): 12 zero bytes, then the address
    bool ok = true;
    if (addr_format == PLUME_ETHK_ADDR_RECORD64) {
        uint32_t rec[16], nz = 0;
        mrk_load_words<16>(rec, in + 64 * i);
        PLUME_UNROLL for (int k = 0; k < 11; k++) nz |= rec[k];
        PLUME_UNROLL for (int k = 0; k < 5; k++) m[3 + k] = rec[11 + k];
        ok = nz == 0u;
    } else {
        eth_load20(m + 3, in + 20 * i);
    }
    if (leaf_format == PLUME_MRK_LEAF_ADDRESS_UINT256) {
        mrk_load_words<8>(m + 8, amount + 32 * i);                                       // big-endian already: abi.encode(uint256) is the 32 bytes
        keccak256_lanes<8, 8>(h, m);
    } else {
        keccak256_lanes<4, 8>(h, m);
    }
    keccak256_lanes<4, 8>(leaf, h);
    PLUME_UNROLL for (int k = 0; k < 8; k++) leaf[k] = ok ? leaf[k] : 0u;
    return ok;
}

// lane i of k_merkle_leaf
PLUME_HD void mrk_leaf_item(const MerkleLeafArgs& a, uint32_t i) {
    uint32_t r[16];
    PLUME_UNROLL for (int k = 8; k < 16; k++) r[k] = 0u;
    const bool ok = mrk_leaf(r, a.leaf_format, a.addr_format, a.in, a.amount, i);
    recover_store<32>(a.leaf + 32 * (size_t)i, r);
    if (a.status) a.status[i] = (uint8_t)(ok ? PLUME_MRK_MATCH : PLUME_MRK_INVALID);
}

// out = Keccak-256(min(a, b) || max(a, b)); out may be a
PLUME_HD void mrk_hash_pair(uint32_t out[8], const uint32_t a[8], const uint32_t b[8]) {
    bool lt = false, decided = false;
    PLUME_UNROLL for (int k = 0; k < 8; k++) {
        const uint32_t x = bswap32(a[k]), y = bswap32(b[k]);
        lt = decided ? lt : x < y;
        decided = decided || x != y;
    }
    const bool a_first = lt || !decided;
    uint32_t m[16];
    PLUME_UNROLL for (int k = 0; k < 8; k++) { m[k] = a_first ? a[k] : b[k]; m[8 + k] = a_first ? b[k] : a[k]; }
    keccak256_lanes<8, 8>(out, m);
}

// parent i from its children, nodes 2i + 1 and 2i + 2: 64 contiguous bytes
PLUME_HD void mrk_node(uint8_t* tree, size_t i) {
    uint32_t c[16], r[16];
    mrk_load_words<16>(c, tree + 32 * (2 * i + 1));
    PLUME_UNROLL for (int k = 8; k < 16; k++) r[k] = 0u;
    mrk_hash_pair(r, c, c + 8);
    recover_store<32>(tree + 32 * i, r);
}

// ------------------------------------------------------------------------------------------------ the sort
struct mrk_rec { uint32_t k[8]; uint32_t idx; };
PLUME_HD void mrk_rec_load(mrk_rec& r, const uint32_t* s, size_t stride, size_t i) {
    PLUME_UNROLL for (int k = 0; k < 8; k++) r.k[k] = s[k * stride + i];
    r.idx = s[8 * stride + i];
}
PLUME_HD void mrk_rec_store(uint32_t* s, size_t stride, size_t i, const mrk_rec& r) {
    PLUME_UNROLL for (int k = 0; k < 8; k++) s[k * stride + i] = r.k[k];
    s[8 * stride + i] = r.idx;
}
// (key, index) of a below (key, index) of b: a total order, indices being distinct
PLUME_HD bool mrk_rec_less(const mrk_rec& a, const mrk_rec& b) {
    bool lt = a.idx < b.idx;
    PLUME_UNROLL for (int k = 7; k >= 0; k--) lt = a.k[k] != b.k[k] ? a.k[k] < b.k[k] : lt;
    return lt;
}
// compare-exchange of records i < l: ascending leaves the smaller one at i
PLUME_HD void mrk_cx(uint32_t* s, size_t stride, size_t i, size_t l, bool asc) {
    mrk_rec a, b;
    mrk_rec_load(a, s, stride, i);
    mrk_rec_load(b, s, stride, l);
    if (mrk_rec_less(b, a) == asc) { mrk_rec_store(s, stride, i, b); mrk_rec_store(s, stride, l, a); }
}
// pair t of the compare-exchange distance j (a power of two): the lower index; the upper one is i | j
PLUME_HD size_t mrk_pair_low(size_t t, size_t j) { return ((t & ~(j - 1)) << 1) | (t & (j - 1)); }
// pair t of stage (k, j), j < tile, inside a tile (stride `tile`) whose first record has index base among all npad
PLUME_HD void mrk_tile_cx(uint32_t* s, uint32_t tile, size_t base, size_t k, uint32_t j, uint32_t t) {
    const size_t i = mrk_pair_low(t, j);
    mrk_cx(s, tile, i, i | j, ((base + i) & k) == 0);
}
// pair t of stage (k, j), j >= tile, in the workspace
PLUME_HD void mrk_global_cx(const MerkleSortArgs& a, size_t k, size_t j, size_t t) {
    const size_t i = mrk_pair_low(t, j);
    mrk_cx(a.ws, a.npad, i, i | j, (i & k) == 0);
}
// record x of the tile at base, from the leaves: the key is the leaf's words byte-swapped, so that word order and numeric order of the words give the order of the bytes
PLUME_HD void mrk_tile_from_leaves(uint32_t* s, const MerkleSortArgs& a, size_t base, uint32_t x) {
    mrk_rec r;
    const size_t g = base + x;
    PLUME_UNROLL for (int k = 0; k < 8; k++) r.k[k] = 0xFFFFFFFFu;
    r.idx = (uint32_t)g;
    if (g < a.n) {
        uint32_t w[8];
        mrk_load_words<8>(w, a.leaf + 32 * g);
        PLUME_UNROLL for (int k = 0; k < 8; k++) r.k[k] = bswap32(w[k]);
    }
    mrk_rec_store(s, a.tile, x, r);
}
PLUME_HD void mrk_tile_from_ws(uint32_t* s, const MerkleSortArgs& a, size_t base, uint32_t x) {
    PLUME_UNROLL for (uint32_t k = 0; k < PLUME_MRK_REC_WORDS; k++) s[k * a.tile + x] = a.ws[k * (size_t)a.npad + base + x];
}
PLUME_HD void mrk_tile_to_ws(const uint32_t* s, const MerkleSortArgs& a, size_t base, uint32_t x) {
    PLUME_UNROLL for (uint32_t k = 0; k < PLUME_MRK_REC_WORDS; k++) a.ws[k * (size_t)a.npad + base + x] = s[k * a.tile + x];
}

// lane i of k_merkle_place
PLUME_HD void mrk_place_item(const MerkleTreeArgs& a, uint32_t i) {
    uint32_t r[16], idx = i;
    PLUME_UNROLL for (int k = 8; k < 16; k++) r[k] = 0u;
    if (a.ws) {
        PLUME_UNROLL for (int k = 0; k < 8; k++) r[k] = bswap32(a.ws[k * (size_t)a.npad + i]);
        idx = a.ws[8 * (size_t)a.npad + i];
    } else {
        mrk_load_words<8>(r, a.leaf + 32 * (size_t)i);
    }
    const uint32_t t = 2u * a.n - 2u - i;
    recover_store<32>(a.tree + 32 * (size_t)t, r);
    if (a.leaf_pos && idx < a.n) a.leaf_pos[idx] = t;                                    // (the padding sorts last: the first n records are the leaves)
}

// lane k of k_merkle_proof
PLUME_HD void mrk_proof_item(const MerkleProofArgs& a, uint32_t k) {
    const uint32_t t0 = a.pos[k], total = 2u * a.n - 1u;
    const uint32_t len = t0 < total ? mrk_log2(t0 + 1u) : PLUME_MRK_BAD_LEN;
    const bool ok = t0 < total && len <= a.depth;
    uint8_t* out = a.proof + 32 * (size_t)a.depth * k;
    uint32_t t = ok ? t0 : 0u;
    PLUME_NOUNROLL for (uint32_t s = 0; s < a.depth; s++) {
        uint32_t r[16];
        PLUME_UNROLL for (int j = 0; j < 16; j++) r[j] = 0u;
        if (t > 0u) {
            const uint32_t sib = (t & 1u) ? t + 1u : t - 1u;                             // (a left child's right sibling exists: every parent has two children)
            mrk_load_words<8>(r, a.tree + 32 * (size_t)sib);
            t = (t - 1u) >> 1;
        }
        recover_store<32>(out + 32 * (size_t)s, r);
    }
    a.proof_len[k] = (uint8_t)(ok ? len : PLUME_MRK_BAD_LEN);
}

// lane k of k_merkle_verify.  Every lane of a wavefront that is active at the call makes the walk's vote (a lane with nothing left only keeps its wavefront company)
PLUME_HD void mrk_verify_item(const MerkleVerifyArgs& a, uint32_t k) {
    uint32_t h[8];
    const bool leaf_ok = mrk_leaf(h, a.leaf_format, a.addr_format, a.in, a.amount, k);
    const uint32_t len = a.proof_len[k];
    const bool ok = leaf_ok && len <= a.depth;
    const uint32_t cnt = ok ? len : 0u;
    const uint8_t* p = a.proof + 32 * (size_t)a.depth * k;
    PLUME_NOUNROLL for (uint32_t s = 0; keccak_any(s < cnt); s++) {
        if (s < cnt) {
            uint32_t e[8];
            mrk_load_words<8>(e, p + 32 * (size_t)s);
            mrk_hash_pair(h, h, e);
        }
    }
    uint32_t root[8], diff = 0;
    mrk_load_words<8>(root, a.root);
    PLUME_UNROLL for (int j = 0; j < 8; j++) diff |= root[j] ^ h[j];
    a.status[k] = (uint8_t)(!ok ? PLUME_MRK_INVALID : diff == 0u ? PLUME_MRK_MATCH : PLUME_MRK_MISMATCH);
}

// The stage schedule of the sort, for the launcher and for the host loops of tests/merkle alike: `local` runs every stage of distance below the tile for the blocks k <= tile
// (from the leaves into the workspace), `global` one stage (k, j) with j >= tile, `merge` the stages j = tile / 2 .. 1 of block size k.
template <class L, class G, class M>
inline void mrk_sort_schedule(uint32_t npad, uint32_t tile, L local, G global, M merge) {
    local();
    for (uint64_t k = 2ull * tile; k <= npad; k <<= 1) {
        for (uint64_t j = k >> 1; j >= tile; j >>= 1) global((size_t)k, (size_t)j);
        merge((size_t)k);
    }
}

}  // namespace plume
