// The Merkle calls (include/plume_hip.h, plume_merkle_leaf_batch*, plume_merkle_tree_build*, plume_merkle_proof_batch*, plume_merkle_verify_batch*): their C ABI and
// their host side.  leaf and verify are the address call over again: per-item kernels on the caller's arrays, no table, no workspace, through serial_host_call_any (verify's
// root is a whole-call input).  build and proof work on ONE tree, so their host-pointer forms never split: a plume_init_multi context runs them on its first shard, the whole
// tree staged in that context's first slot (proof: serial_host_call with the tree as a whole-call input; build: one piece, serial_host_piece).  build's sort keeps its
// records in ctx->mrksort (36 B per padded leaf), so the device form holds the workspace like the transaction sender does.  fused_top = 0 (env PLUME_MERKLE_FUSED_TOP=0,
// the A/B knob of tests/gpu_debug/merkle_timing.py) runs one k_merkle_level launch per depth instead of k_merkle_top.
#include <cstdlib>

#include "../../include/plume_hip.h"
#include "plume_capi_ctx.h"
#include "plume_merkle_launch.h"

using namespace plume;

extern "C" size_t plume_merkle_max_proof_len(size_t n) {
    size_t v = n ? 2 * n - 1 : 0, d = 0;
    while (v > 1) { v >>= 1; d++; }
    return d;
}
static int merkle_formats_ok(int leaf_format, int addr_format) {
    if (leaf_format != PLUME_MRK_LEAF_HASH32 && leaf_format != PLUME_MRK_LEAF_ADDRESS && leaf_format != PLUME_MRK_LEAF_ADDRESS_UINT256)
        return fail(PLUME_ERR_ARG, "leaf_format must be 0, 1 or 2");
    if (addr_format != PLUME_ETHK_ADDR_RAW20 && addr_format != PLUME_ETHK_ADDR_RECORD64) return fail(PLUME_ERR_ARG, "addr_format must be 0 or 1: a leaf is made of address bytes, not of EIP-55 text");
    return 0;
}
static int merkle_leaf_args_ok(int leaf_format, int addr_format, size_t n, const void* in, const void* amount, const void* leaf) {
    if (int rc = merkle_formats_ok(leaf_format, addr_format)) return rc;
    if (n && (!in || !leaf || (leaf_format == PLUME_MRK_LEAF_ADDRESS_UINT256 && !amount))) return fail(PLUME_ERR_ARG, "null array");
    if (n > 0xFFFFFFF0u) return fail(PLUME_ERR_ARG, "n too large");
    return 0;
}
static int merkle_leaf_device(plume_ctx* ctx, int leaf_format, int addr_format, size_t n, const uint8_t* in, const uint8_t* amount, uint8_t* leaf, uint8_t* status,
                              hipStream_t st) {
    if (n == 0) return 0;
    MerkleLeafArgs a; a.leaf_format = leaf_format; a.addr_format = addr_format; a.n = (uint32_t)n; a.in = in; a.amount = amount; a.leaf = leaf; a.status = status;
    ctx->timer.begin(st);
    launch_merkle_leaf(a, st); ctx->timer.stage("merkle_leaf", st);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int plume_merkle_leaf_batch_device(plume_ctx* ctx, int leaf_format, int addr_format, size_t n, const uint8_t* address, const uint8_t* amount, uint8_t* leaf32,
                                              uint8_t* status, void* stream) {
    Route rt_(ctx, stream); ctx = rt_.lane; const hipStream_t st_ = rt_.st;
    if (int rc = bind(ctx)) return rc;
    if (int rc = merkle_leaf_args_ok(leaf_format, addr_format, n, address, amount, leaf32)) return rc;
    return merkle_leaf_device(ctx, leaf_format, addr_format, n, address, amount, leaf32, status, st_);
}
extern "C" int plume_merkle_leaf_batch(plume_ctx* ctx, int leaf_format, int addr_format, size_t n, const uint8_t* address, const uint8_t* amount, uint8_t* leaf32,
                                       uint8_t* status) {
    if (!ctx) return fail(PLUME_ERR_ARG, "null context");
    if (int rc = merkle_leaf_args_ok(leaf_format, addr_format, n, address, amount, leaf32)) return rc;
    if (leaf_format != PLUME_MRK_LEAF_ADDRESS_UINT256) amount = nullptr;
    const HostCall call{nullptr, nullptr, {{address, mrk_item_width(leaf_format, addr_format)}, {amount, 32}}, {{leaf32, 32}, {status, 1}}};
    return serial_host_call_any(ctx, n, call, [&](HostSlot& sl, size_t cnt, plume_ctx* on) -> int {
        return merkle_leaf_device(on, leaf_format, addr_format, cnt, sl.in[0].as<uint8_t>(), amount ? sl.in[1].as<uint8_t>() : nullptr, sl.out[0].as<uint8_t>(),
                                  status ? sl.out[1].as<uint8_t>() : nullptr, on->stream);
    });
}
static int merkle_build_args_ok(int flags, size_t n, const void* leaf, const void* tree) {
    if (int rc = merkle_formats_ok(PLUME_MRK_LEAF_HASH32, PLUME_ETHK_ADDR_RAW20)) return rc;
    if (flags & ~PLUME_MRK_SORT_LEAVES) return fail(PLUME_ERR_ARG, "unknown flag bits");
    if (n == 0 || n > PLUME_MRK_MAX_N) return fail(PLUME_ERR_ARG, "a tree has between 1 and 2^26 leaves");
    if (!leaf || !tree) return fail(PLUME_ERR_ARG, "null array");
    return 0;
}
static int merkle_build_device(plume_ctx* ctx, int flags, size_t n, const uint8_t* leaf, uint8_t* tree, uint32_t* leaf_pos, hipStream_t st) {
    const bool sorted = (flags & PLUME_MRK_SORT_LEAVES) && n > 1;
    const uint32_t npad = mrk_next_pow2((uint32_t)n);
    if (int rc = ws_acquire(ctx, st)) return rc;
    WsHold hold(ctx, st);
    if (sorted && ctx->mrksort.ensure((size_t)PLUME_MRK_REC_WORDS * 4 * npad)) return PLUME_ERR_HIP;
    ctx->timer.begin(st);
    if (sorted) {
        MerkleSortArgs sa; sa.n = (uint32_t)n; sa.npad = npad; sa.tile = npad < PLUME_MRK_TILE ? npad : PLUME_MRK_TILE; sa.leaf = leaf; sa.ws = ctx->mrksort.as<uint32_t>();
        launch_merkle_sort(sa, st); ctx->timer.stage("merkle_sort", st);
    }
    MerkleTreeArgs ta; ta.n = (uint32_t)n; ta.npad = npad; ta.leaf = leaf; ta.ws = sorted ? ctx->mrksort.as<uint32_t>() : nullptr; ta.tree = tree; ta.leaf_pos = leaf_pos;
    launch_merkle_place(ta, st); ctx->timer.stage("merkle_place", st);
    if (n >= 2) {
        const char* e = std::getenv("PLUME_MERKLE_FUSED_TOP");                           // A/B knob (tests/gpu_debug/merkle_timing.py): 0 = one launch per depth all the way up
        const bool fused = !(e && std::atoi(e) == 0);
        uint32_t d = mrk_parent_depth((uint32_t)n) + 1u;
        const uint32_t stop = fused ? PLUME_MRK_TOP_DEPTH + 1u : 0u;
        if (d > stop) {
            while (d-- > stop) launch_merkle_level(tree, (uint32_t)n, d, st);
            d = stop;
            ctx->timer.stage("merkle_levels", st);
        }
        if (fused) { launch_merkle_top(tree, (uint32_t)n, d - 1u, st); ctx->timer.stage("merkle_top", st); }
    }
    HIPCHK(hipGetLastError());
    return hold.release();
}
extern "C" int plume_merkle_tree_build_device(plume_ctx* ctx, int flags, size_t n, const uint8_t* leaf32, uint8_t* tree, uint32_t* leaf_pos, void* stream) {
    Route rt_(ctx, stream); ctx = rt_.lane; const hipStream_t st_ = rt_.st;
    if (int rc = bind(ctx)) return rc;
    if (int rc = merkle_build_args_ok(flags, n, leaf32, tree)) return rc;
    return merkle_build_device(ctx, flags, n, leaf32, tree, leaf_pos, st_);
}
// one piece whatever the chunk size is: the tree is built where all of its leaves are
extern "C" int plume_merkle_tree_build(plume_ctx* ctx, int flags, size_t n, const uint8_t* leaf32, uint8_t* tree, uint32_t* leaf_pos) {
    if (!ctx) return fail(PLUME_ERR_ARG, "null context");
    if (int rc = merkle_build_args_ok(flags, n, leaf32, tree)) return rc;
    if (!ctx->shards.empty()) ctx = ctx->shards[0];                             // one tree: one device holds all of it
    HIPCHK(hipSetDevice(ctx->device));
    const HostCall call{nullptr, nullptr, {{leaf32, 32}}, {{tree, 32 * (2 * n - 1), false, true}, {leaf_pos, 4}}};
    return serial_host_piece(ctx, call, 0, n, [&](HostSlot& sl, size_t, plume_ctx* on) -> int {
        return merkle_build_device(on, flags, n, sl.in[0].as<uint8_t>(), sl.out[0].as<uint8_t>(), leaf_pos ? sl.out[1].as<uint32_t>() : nullptr, on->stream);
    });
}
static int merkle_proof_args_ok(size_t n, const void* tree, size_t m, const void* pos, size_t depth, const void* proof, const void* proof_len) {
    if (int rc = merkle_formats_ok(PLUME_MRK_LEAF_HASH32, PLUME_ETHK_ADDR_RAW20)) return rc;
    if (n == 0 || n > PLUME_MRK_MAX_N) return fail(PLUME_ERR_ARG, "a tree has between 1 and 2^26 leaves");
    if (depth > PLUME_MRK_MAX_DEPTH) return fail(PLUME_ERR_ARG, "depth above 64");
    if (m > 0xFFFFFFF0u) return fail(PLUME_ERR_ARG, "m too large");
    if (m && (!tree || !pos || !proof_len || (depth && !proof))) return fail(PLUME_ERR_ARG, "null array");
    return 0;
}
static int merkle_proof_device(plume_ctx* ctx, size_t n, const uint8_t* tree, size_t m, const uint32_t* pos, size_t depth, uint8_t* proof, uint8_t* proof_len, hipStream_t st) {
    if (m == 0) return 0;
    MerkleProofArgs a; a.n = (uint32_t)n; a.m = (uint32_t)m; a.depth = (uint32_t)depth; a.tree = tree; a.pos = pos; a.proof = proof; a.proof_len = proof_len;
    ctx->timer.begin(st);
    launch_merkle_proof(a, st); ctx->timer.stage("merkle_proof", st);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int plume_merkle_proof_batch_device(plume_ctx* ctx, size_t n, const uint8_t* tree, size_t m, const uint32_t* pos, size_t depth, uint8_t* proof,
                                               uint8_t* proof_len, void* stream) {
    Route rt_(ctx, stream); ctx = rt_.lane; const hipStream_t st_ = rt_.st;
    if (int rc = bind(ctx)) return rc;
    if (int rc = merkle_proof_args_ok(n, tree, m, pos, depth, proof, proof_len)) return rc;
    return merkle_proof_device(ctx, n, tree, m, pos, depth, proof, proof_len, st_);
}
extern "C" int plume_merkle_proof_batch(plume_ctx* ctx, size_t n, const uint8_t* tree, size_t m, const uint32_t* pos, size_t depth, uint8_t* proof, uint8_t* proof_len) {
    if (!ctx) return fail(PLUME_ERR_ARG, "null context");
    if (int rc = merkle_proof_args_ok(n, tree, m, pos, depth, proof, proof_len)) return rc;
    if (m == 0) return 0;
    if (!ctx->shards.empty()) ctx = ctx->shards[0];                             // the tree is staged once: one device answers every index
    const size_t pb = 32 * depth;
    const HostCall call{nullptr, nullptr, {{tree, 32 * (2 * n - 1), false, true}, {pos, 4}}, {{pb ? proof : nullptr, pb}, {proof_len, 1}}};
    return serial_host_call(ctx, m, call, [&](HostSlot& sl, size_t cnt, plume_ctx* on) -> int {
        return merkle_proof_device(on, n, sl.in[0].as<uint8_t>(), cnt, sl.in[1].as<uint32_t>(), depth, pb ? sl.out[0].as<uint8_t>() : nullptr, sl.out[1].as<uint8_t>(), on->stream);
    });
}
static int merkle_verify_args_ok(int leaf_format, int addr_format, size_t m, const void* in, const void* amount, size_t depth, const void* proof, const void* proof_len,
                                 const void* root, const void* status) {
    if (int rc = merkle_formats_ok(leaf_format, addr_format)) return rc;
    if (depth > PLUME_MRK_MAX_DEPTH) return fail(PLUME_ERR_ARG, "depth above 64");
    if (m > 0xFFFFFFF0u) return fail(PLUME_ERR_ARG, "m too large");
    if (m && (!in || !proof_len || !root || !status || (depth && !proof) || (leaf_format == PLUME_MRK_LEAF_ADDRESS_UINT256 && !amount))) return fail(PLUME_ERR_ARG, "null array");
    return 0;
}
static int merkle_verify_device(plume_ctx* ctx, int leaf_format, int addr_format, size_t m, const uint8_t* in, const uint8_t* amount, size_t depth, const uint8_t* proof,
                                const uint8_t* proof_len, const uint8_t* root, uint8_t* status, hipStream_t st) {
    if (m == 0) return 0;
    MerkleVerifyArgs a; a.leaf_format = leaf_format; a.addr_format = addr_format; a.m = (uint32_t)m; a.depth = (uint32_t)depth; a.in = in; a.amount = amount; a.proof = proof;
    a.proof_len = proof_len; a.root = root; a.status = status;
    ctx->timer.begin(st);
    launch_merkle_verify(a, st); ctx->timer.stage("merkle_verify", st);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int plume_merkle_verify_batch_device(plume_ctx* ctx, int leaf_format, int addr_format, size_t m, const uint8_t* address_or_leaf, const uint8_t* amount,
                                                size_t depth, const uint8_t* proof, const uint8_t* proof_len, const uint8_t* root32, uint8_t* status, void* stream) {
    Route rt_(ctx, stream); ctx = rt_.lane; const hipStream_t st_ = rt_.st;
    if (int rc = bind(ctx)) return rc;
    if (int rc = merkle_verify_args_ok(leaf_format, addr_format, m, address_or_leaf, amount, depth, proof, proof_len, root32, status)) return rc;
    return merkle_verify_device(ctx, leaf_format, addr_format, m, address_or_leaf, amount, depth, proof, proof_len, root32, status, st_);
}
extern "C" int plume_merkle_verify_batch(plume_ctx* ctx, int leaf_format, int addr_format, size_t m, const uint8_t* address_or_leaf, const uint8_t* amount, size_t depth,
                                         const uint8_t* proof, const uint8_t* proof_len, const uint8_t* root32, uint8_t* status) {
    if (!ctx) return fail(PLUME_ERR_ARG, "null context");
    if (int rc = merkle_verify_args_ok(leaf_format, addr_format, m, address_or_leaf, amount, depth, proof, proof_len, root32, status)) return rc;
    if (leaf_format != PLUME_MRK_LEAF_ADDRESS_UINT256) amount = nullptr;
    const size_t pb = 32 * depth;
    const HostCall call{nullptr, nullptr, {{address_or_leaf, mrk_item_width(leaf_format, addr_format)}, {amount, 32}, {pb ? proof : nullptr, pb}, {proof_len, 1}, {root32, 32, false, true}},
                        {{status, 1}}};
    return serial_host_call_any(ctx, m, call, [&](HostSlot& sl, size_t cnt, plume_ctx* on) -> int {
        return merkle_verify_device(on, leaf_format, addr_format, cnt, sl.in[0].as<uint8_t>(), amount ? sl.in[1].as<uint8_t>() : nullptr, depth,
                                    pb ? sl.in[2].as<uint8_t>() : nullptr, sl.in[3].as<uint8_t>(), sl.in[4].as<uint8_t>(), sl.out[0].as<uint8_t>(), on->stream);
    });
}
