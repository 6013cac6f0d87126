// TEST INFRASTRUCTURE ONLY.  plume_merkle_* on the library's host side (csrc/plume_merkle_capi.hip) on the mock HIP runtime, under
// the sanitizers (tests/test_merkle_hostsim.py).
// usage: merkle_driver VECTORS SEED.  VECTORS is written by the test from the Python restatement (tests/_merkle.py): u32 count, then per tree u32 leaf_format, addr_format,
// sort, n, depth; the items, the amounts (format 2), the leaves, n leaf status bytes, the tree, leaf_pos, the proofs of the input items in depth slots, n proof lengths.
// Every call must reproduce those bytes: the host forms with chunks smaller than n, pageable and page-locked arrays, optional arrays absent; the device forms chained on
// a caller stream (which must not have run anything when the calls return, under the lazy scheduler); plume_init_multi contexts over three and eight mock devices (leaf
// and verify split over the shards, build and proofs run on the first); argument errors; then every allocation of a build, a proof and a verify call fails in turn: an
// error code, the outputs of a repeated call right, nothing leaked.  A context that only ever did this builds no table.
#define DRIVER_NAME "merkle_driver"
#include "driver_prelude.h"

struct Tree {
    uint32_t leaf_format = 0, addr_format = 0, sort = 0, n = 0, depth = 0;
    size_t W = 0;
    std::vector<uint8_t> items, amounts, leaves, leaf_status, tree, proofs, proof_len;
    std::vector<uint32_t> leaf_pos;
};
static std::vector<Tree> g_trees;

static void read_vectors(const char* path) {
    FILE* f = std::fopen(path, "rb");
    REQUIRE(f);
    uint32_t count = 0;
    REQUIRE(std::fread(&count, 4, 1, f) == 1 && count >= 10);
    auto rd = [&](std::vector<uint8_t>& v, size_t bytes) { v.resize(bytes); REQUIRE(bytes == 0 || std::fread(v.data(), 1, bytes, f) == bytes); };
    for (uint32_t k = 0; k < count; k++) {
        Tree t;
        uint32_t h[5];
        REQUIRE(std::fread(h, 4, 5, f) == 5);
        t.leaf_format = h[0]; t.addr_format = h[1]; t.sort = h[2]; t.n = h[3]; t.depth = h[4];
        t.W = t.leaf_format == PLUME_MERKLE_LEAF_HASH32 ? 32 : t.addr_format == PLUME_ETH_ADDR_RECORD64 ? 64 : 20;
        const size_t n = t.n;
        REQUIRE(n >= 1 && t.depth == plume_merkle_max_proof_len(n));
        rd(t.items, t.W * n); rd(t.amounts, t.leaf_format == PLUME_MERKLE_LEAF_ADDRESS_UINT256 ? 32 * n : 0); rd(t.leaves, 32 * n); rd(t.leaf_status, n);
        rd(t.tree, 32 * (2 * n - 1));
        t.leaf_pos.resize(n);
        REQUIRE(std::fread(t.leaf_pos.data(), 4, n, f) == n);
        rd(t.proofs, 32 * (size_t)t.depth * n); rd(t.proof_len, n);
        g_trees.push_back(std::move(t));
    }
    std::fclose(f);
}

static bool is(const Arr& a, const std::vector<uint8_t>& v) { return v.size() == a.bytes && (a.bytes == 0 || std::memcmp(a.p, v.data(), a.bytes) == 0); }

// the four calls over one tree of the vectors, each on arrays of its own; mutate: one bit of every proof is flipped before verify
struct Chain {
    const Tree& t;
    int kind;
    bool with_optional, mutate;
    Arr items, amounts, leaf, lst, tree, pos, proof, len, vproof, vst;
    std::vector<uint8_t> want_vst, vproof0;
    Chain(const Tree& t_, int k, bool opt, bool mut)
        : t(t_), kind(k), with_optional(opt), mutate(mut), items(t_.items.size(), k, t_.items.data()), amounts(t_.amounts.size(), k, t_.amounts.data()), leaf(32 * (size_t)t_.n, k),
          lst(t_.n, k), tree(t_.tree.size(), k), pos(4 * (size_t)t_.n, k), proof(t_.proofs.size(), k), len(t_.n, k), vproof(t_.proofs.size(), k, t_.proofs.data()), vst(t_.n, k) {
        want_vst.resize(t.n);
        for (size_t j = 0; j < t.n; j++) {
            const bool valid = t.leaf_status[j] == PLUME_MERKLE_MATCH;
            const size_t ln = t.proof_len[j];
            if (mutate && ln) vproof.p[32 * t.depth * j + 32 * (j % ln) + j % 32] ^= (uint8_t)(1u << (j % 8));
            want_vst[j] = (uint8_t)(!valid ? PLUME_MERKLE_INVALID : mutate && ln ? PLUME_MERKLE_MISMATCH : PLUME_MERKLE_MATCH);
        }
        vproof0.assign(vproof.p, vproof.p + vproof.bytes);
    }
    const uint8_t* amt() const { return t.amounts.empty() ? nullptr : amounts.p; }
    int run_leaf(plume_ctx* c, hipStream_t st) {
        uint8_t* s = with_optional ? lst.p : nullptr;
        return kind == 2 ? plume_merkle_leaf_batch_device(c, (int)t.leaf_format, (int)t.addr_format, t.n, items.p, amt(), leaf.p, s, st)
                         : plume_merkle_leaf_batch(c, (int)t.leaf_format, (int)t.addr_format, t.n, items.p, amt(), leaf.p, s);
    }
    // from_vectors: the leaves of the vectors (the host forms are independent calls); otherwise the leaves the leaf call wrote (the device chain)
    int run_build(plume_ctx* c, hipStream_t st, const uint8_t* leaves) {
        uint32_t* lp = with_optional ? (uint32_t*)pos.p : nullptr;
        return kind == 2 ? plume_merkle_tree_build_device(c, t.sort ? PLUME_MERKLE_SORT_LEAVES : 0, t.n, leaves, tree.p, lp, st)
                         : plume_merkle_tree_build(c, t.sort ? PLUME_MERKLE_SORT_LEAVES : 0, t.n, leaves, tree.p, lp);
    }
    int run_proof(plume_ctx* c, hipStream_t st, const uint8_t* tr, const uint32_t* ps) {
        return kind == 2 ? plume_merkle_proof_batch_device(c, t.n, tr, t.n, ps, t.depth, proof.p, len.p, st) : plume_merkle_proof_batch(c, t.n, tr, t.n, ps, t.depth, proof.p, len.p);
    }
    int run_verify(plume_ctx* c, hipStream_t st, const uint8_t* ln, const uint8_t* root) {
        return kind == 2 ? plume_merkle_verify_batch_device(c, (int)t.leaf_format, (int)t.addr_format, t.n, items.p, amt(), t.depth, vproof.p, ln, root, vst.p, st)
                         : plume_merkle_verify_batch(c, (int)t.leaf_format, (int)t.addr_format, t.n, items.p, amt(), t.depth, vproof.p, ln, root, vst.p);
    }
    bool untouched() const { return leaf.untouched() && lst.untouched() && tree.untouched() && pos.untouched() && proof.untouched() && len.untouched() && vst.untouched(); }
    void check() {
        REQUIRE(is(leaf, t.leaves) && is(tree, t.tree) && is(proof, t.proofs) && is(len, t.proof_len) && is(vst, want_vst));
        if (with_optional) REQUIRE(is(lst, t.leaf_status) && std::memcmp(pos.p, t.leaf_pos.data(), 4 * (size_t)t.n) == 0); else REQUIRE(lst.untouched() && pos.untouched());
        REQUIRE(is(items, t.items) && (t.amounts.empty() || is(amounts, t.amounts)) && is(vproof, vproof0));
    }
};

static void host_forms(plume_ctx* ctx, const char* what, size_t chunk) {
    if (chunk) REQUIRE(plume_set_chunk(ctx, chunk) == 0);
    for (size_t k = 0; k < g_trees.size(); k++) {
        const Tree& t = g_trees[k];
        if (chunk == 1 && t.n > 16) continue;
        g_what = std::string(what) + ", tree " + std::to_string(k) + ": n " + std::to_string(t.n) + ", leaf format " + std::to_string(t.leaf_format) + ", sort " + std::to_string(t.sort) +
                 ", chunk " + std::to_string(chunk);
        Chain c(t, (int)(rng() & 1), (rng() & 3) != 0, (k & 1) != 0);
        REQUIRE(c.run_leaf(ctx, nullptr) == 0);
        REQUIRE(c.run_build(ctx, nullptr, t.leaves.data()) == 0);
        REQUIRE(c.run_proof(ctx, nullptr, t.tree.data(), t.leaf_pos.data()) == 0);
        REQUIRE(c.run_verify(ctx, nullptr, t.proof_len.data(), t.tree.data()) == 0);
        c.check();
    }
    REQUIRE(plume_set_chunk(ctx, (size_t)1 << 20) == 0);
}

// leaf -> build -> proof -> verify queued back to back on one caller stream, every call reading what the one before wrote; compared after one synchronise
static void device_forms(plume_ctx* ctx) {
    const bool lazy = std::getenv("PLUME_MOCK_SCHED") == nullptr;
    hipStream_t st = nullptr;
    REQUIRE(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
    for (size_t k = 0; k < g_trees.size(); k++) {
        const Tree& t = g_trees[k];
        g_what = "device forms, tree " + std::to_string(k) + ": n " + std::to_string(t.n);
        Chain c(t, 2, true, false);
        REQUIRE(c.run_leaf(ctx, st) == 0 && c.run_build(ctx, st, c.leaf.p) == 0 && c.run_proof(ctx, st, c.tree.p, (const uint32_t*)c.pos.p) == 0 &&
                c.run_verify(ctx, st, c.len.p, c.tree.p) == 0);
        // (verify reads the proofs of the vectors, the lengths and the root the chain made)
        if (lazy) REQUIRE(c.untouched());                                              // enqueued, not run: the device forms do not synchronise
        REQUIRE(hipStreamSynchronize(st) == hipSuccess);
        c.check();
    }
    REQUIRE(hipStreamDestroy(st) == hipSuccess);
}

static void arguments(plume_ctx* ctx) {
    g_what = "arguments";
    const Tree& t = g_trees[0];
    std::vector<uint8_t> leaf(32 * 4, 1), tree(32 * 7, kFill), st(4, kFill), len(4, 0), proof(32 * 2 * 4, 0);
    std::vector<uint32_t> pos(4, 0);
    REQUIRE(plume_merkle_tree_build(nullptr, 0, 4, leaf.data(), tree.data(), nullptr) == PLUME_ERR_ARG);
    REQUIRE(plume_merkle_tree_build(ctx, 0, 0, leaf.data(), tree.data(), nullptr) == PLUME_ERR_ARG && plume_merkle_tree_build(ctx, 1, ((size_t)1 << 26) + 1, leaf.data(), tree.data(), nullptr) == PLUME_ERR_ARG);
    REQUIRE(plume_merkle_tree_build(ctx, 2, 4, leaf.data(), tree.data(), nullptr) == PLUME_ERR_ARG && plume_merkle_tree_build(ctx, 1, 4, nullptr, tree.data(), nullptr) == PLUME_ERR_ARG &&
            plume_merkle_tree_build(ctx, 1, 4, leaf.data(), nullptr, nullptr) == PLUME_ERR_ARG);
    REQUIRE(all_of(tree.data(), tree.size(), kFill));
    REQUIRE(plume_merkle_leaf_batch(ctx, 3, 0, 4, leaf.data(), nullptr, tree.data(), nullptr) == PLUME_ERR_ARG && plume_merkle_leaf_batch(ctx, -1, 0, 4, leaf.data(), nullptr, tree.data(), nullptr) == PLUME_ERR_ARG);
    REQUIRE(plume_merkle_leaf_batch(ctx, 1, PLUME_ETH_ADDR_EIP55, 4, leaf.data(), nullptr, tree.data(), nullptr) == PLUME_ERR_ARG);
    REQUIRE(plume_merkle_leaf_batch(ctx, 2, 0, 4, leaf.data(), nullptr, tree.data(), nullptr) == PLUME_ERR_ARG);        // no amounts
    REQUIRE(plume_merkle_leaf_batch(ctx, 1, 0, 4, nullptr, nullptr, tree.data(), nullptr) == PLUME_ERR_ARG && plume_merkle_leaf_batch(ctx, 1, 0, 4, leaf.data(), nullptr, nullptr, nullptr) == PLUME_ERR_ARG);
    REQUIRE(plume_merkle_leaf_batch(ctx, 1, 0, 0, nullptr, nullptr, nullptr, nullptr) == 0);                            // an empty batch is no error
    REQUIRE(plume_merkle_proof_batch(ctx, 0, tree.data(), 4, pos.data(), 2, proof.data(), len.data()) == PLUME_ERR_ARG);
    REQUIRE(plume_merkle_proof_batch(ctx, 4, tree.data(), 4, pos.data(), 65, proof.data(), len.data()) == PLUME_ERR_ARG);
    REQUIRE(plume_merkle_proof_batch(ctx, 4, tree.data(), 4, nullptr, 2, proof.data(), len.data()) == PLUME_ERR_ARG && plume_merkle_proof_batch(ctx, 4, tree.data(), 4, pos.data(), 2, nullptr, len.data()) == PLUME_ERR_ARG);
    REQUIRE(plume_merkle_proof_batch(ctx, 4, tree.data(), 0, nullptr, 2, nullptr, nullptr) == 0);
    REQUIRE(plume_merkle_verify_batch(ctx, 0, 0, 4, leaf.data(), nullptr, 2, proof.data(), len.data(), leaf.data(), nullptr) == PLUME_ERR_ARG);
    REQUIRE(plume_merkle_verify_batch(ctx, 0, 0, 4, leaf.data(), nullptr, 2, proof.data(), len.data(), nullptr, st.data()) == PLUME_ERR_ARG);
    REQUIRE(plume_merkle_verify_batch(ctx, 0, 2, 4, leaf.data(), nullptr, 2, proof.data(), len.data(), leaf.data(), st.data()) == PLUME_ERR_ARG);
    REQUIRE(plume_merkle_verify_batch(ctx, 0, 0, 4, leaf.data(), nullptr, 0, nullptr, len.data(), leaf.data(), st.data()) == 0 && st[0] == PLUME_MERKLE_MATCH);   // depth 0: leaf == root
    REQUIRE(plume_merkle_max_proof_len(0) == 0 && plume_merkle_max_proof_len(1) == 0 && plume_merkle_max_proof_len(2) == 1 && plume_merkle_max_proof_len(3) == 2 &&
            plume_merkle_max_proof_len(4) == 2 && plume_merkle_max_proof_len(5) == 3 && plume_merkle_max_proof_len((size_t)1 << 26) == 26);
    plume_ctx* multi = nullptr;
    int ids[2] = {0, 1};
    REQUIRE(plume_init_multi(&multi, ids, 2) == 0);
    Chain d(t, 2, true, false);
    REQUIRE(d.run_leaf(multi, nullptr) == PLUME_ERR_ARG && d.run_build(multi, nullptr, d.leaf.p) == PLUME_ERR_ARG && d.run_proof(multi, nullptr, d.tree.p, (const uint32_t*)d.pos.p) == PLUME_ERR_ARG &&
            d.run_verify(multi, nullptr, d.len.p, d.tree.p) == PLUME_ERR_ARG);       // device pointers belong to one GPU
    REQUIRE(d.untouched());
    plume_destroy(multi);
}

// every allocation of one host-form call fails in turn; which: 0 build, 1 proof, 2 verify, 3 leaf
static void failing_allocations(int which) {
    const Outstanding before;
    const Tree* tp = nullptr;
    for (const Tree& t : g_trees) if (t.sort && t.n >= 13 && t.leaf_format == PLUME_MERKLE_LEAF_ADDRESS_UINT256) tp = &t;
    REQUIRE(tp);
    const Tree& t = *tp;
    auto call = [&](Chain& c, plume_ctx* ctx) {
        return which == 0 ? c.run_build(ctx, nullptr, t.leaves.data()) : which == 1 ? c.run_proof(ctx, nullptr, t.tree.data(), t.leaf_pos.data())
             : which == 2 ? c.run_verify(ctx, nullptr, t.proof_len.data(), t.tree.data()) : c.run_leaf(ctx, nullptr);
    };
    auto right = [&](Chain& c) {
        return which == 0 ? is(c.tree, t.tree) && std::memcmp(c.pos.p, t.leaf_pos.data(), 4 * (size_t)t.n) == 0 : which == 1 ? is(c.proof, t.proofs) && is(c.len, t.proof_len)
             : which == 2 ? is(c.vst, c.want_vst) : is(c.leaf, t.leaves) && is(c.lst, t.leaf_status);
    };
    plume_ctx* ctx = nullptr;
    REQUIRE(plume_init(&ctx, 0) == 0);
    (void)mockhip::fail_allocation(-1);
    { Chain c(t, 0, true, false); g_what = "allocations: counting call " + std::to_string(which); REQUIRE(call(c, ctx) == 0 && right(c)); }
    const long made = mockhip::fail_allocation(-1);
    REQUIRE(made == (which == 0 ? 4 : which == 1 ? 4 : which == 2 ? 6 : 4));            // build: leaves, tree, leaf_pos, the sort's records; proof: tree, pos, proof, len; verify:
                                                                                        // root, items, amounts, proof, len, status; leaf: items, amounts, leaf, status -- and no table
    plume_destroy(ctx);
    for (long k = 0; k < made; k++) {
        g_what = "allocations: call " + std::to_string(which) + ", number " + std::to_string(k) + " fails";
        REQUIRE(plume_init(&ctx, 0) == 0);
        Chain c(t, (int)(k & 1), true, false);
        (void)mockhip::fail_allocation(k);
        REQUIRE(call(c, ctx) == PLUME_ERR_HIP && std::string(plume_last_error()).find("hipMalloc") != std::string::npos);
        REQUIRE(c.untouched());
        (void)mockhip::fail_allocation(-1);
        REQUIRE(call(c, ctx) == 0 && right(c));                                         // the context is usable afterwards
        plume_destroy(ctx);
    }
    REQUIRE(Outstanding() == before);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    read_vectors(argv[1]);
    const unsigned long long seed = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1;
    rng.seed(seed);
    plume_ctx* ctx = nullptr;
    REQUIRE(plume_init(&ctx, 0) == 0);
    const long dev_after_init = mockhip::outstanding(0);
    host_forms(ctx, "one device, host forms, one chunk", 0);
    host_forms(ctx, "one device, host forms, chunks of 7", 7);
    host_forms(ctx, "one device, host forms, chunks of 1", 1);
    device_forms(ctx);
    g_what = "no table";
    REQUIRE(mockhip::outstanding(0) <= dev_after_init + 8);                             // staging (five inputs, two outputs) and the sort's records: no table
    for (int devices : {3, 8}) {
        plume_ctx* multi = nullptr;
        int ids[8] = {0, 1, 2, 3, 4, 5, 6, 7};
        REQUIRE(plume_init_multi(&multi, ids, devices) == 0);
        REQUIRE(plume_num_shards(multi) == devices);
        host_forms(multi, devices == 3 ? "three devices, host forms" : "eight devices, host forms", devices == 3 ? 5 : 0);
        plume_destroy(multi);
    }
    arguments(ctx);
    plume_destroy(ctx);
    for (int which = 0; which < 4; which++) failing_allocations(which);
    REQUIRE(mockhip::outstanding(0) == 0 && mockhip::outstanding(2) == 0 && mockhip::outstanding(3) == 0);
    std::printf("merkle_driver seed %llu: ok\n", seed);
    return 0;
}
