// C ABI of the Merkle calls (include/plume_hip.h, plume_merkle_*): hands the launchers of plume_merkle_kernels.hip to the host side of plume_capi.hip as hooks.  Kept apart
// from plume_capi.hip so that the CPU build of that file (tests/hostsim) links without these launchers.
#include "../../include/plume_hip.h"
#include "plume_capi_internal.h"
#include "plume_merkle_launch.h"

using namespace plume;

static const MerkleLaunch kMerkleLaunch = {launch_merkle_leaf, launch_merkle_sort, launch_merkle_place, launch_merkle_level, launch_merkle_top, launch_merkle_proof,
                                           launch_merkle_verify};

extern "C" size_t plume_merkle_max_proof_len(size_t n) {
    size_t v = n ? 2 * n - 1 : 0, d = 0;
    while (v > 1) { v >>= 1; d++; }
    return d;
}
extern "C" int plume_merkle_leaf_batch(plume_ctx* ctx, int leaf_format, int addr_format, size_t n, const uint8_t* address, const uint8_t* amount, uint8_t* leaf32,
                                       uint8_t* status) {
    return capi_merkle_leaf(ctx, leaf_format, addr_format, n, address, amount, leaf32, status, &kMerkleLaunch);
}
extern "C" int plume_merkle_leaf_batch_device(plume_ctx* ctx, int leaf_format, int addr_format, size_t n, const uint8_t* address, const uint8_t* amount, uint8_t* leaf32,
                                              uint8_t* status, void* stream) {
    return capi_merkle_leaf_device(ctx, leaf_format, addr_format, n, address, amount, leaf32, status, stream, &kMerkleLaunch);
}
extern "C" int plume_merkle_tree_build(plume_ctx* ctx, int flags, size_t n, const uint8_t* leaf32, uint8_t* tree, uint32_t* leaf_pos) {
    return capi_merkle_tree_build(ctx, flags, n, leaf32, tree, leaf_pos, &kMerkleLaunch);
}
extern "C" int plume_merkle_tree_build_device(plume_ctx* ctx, int flags, size_t n, const uint8_t* leaf32, uint8_t* tree, uint32_t* leaf_pos, void* stream) {
    return capi_merkle_tree_build_device(ctx, flags, n, leaf32, tree, leaf_pos, stream, &kMerkleLaunch);
}
extern "C" int plume_merkle_proof_batch(plume_ctx* ctx, size_t n, const uint8_t* tree, size_t m, const uint32_t* pos, size_t depth, uint8_t* proof, uint8_t* proof_len) {
    return capi_merkle_proof(ctx, n, tree, m, pos, depth, proof, proof_len, &kMerkleLaunch);
}
extern "C" int plume_merkle_proof_batch_device(plume_ctx* ctx, size_t n, const uint8_t* tree, size_t m, const uint32_t* pos, size_t depth, uint8_t* proof,
                                               uint8_t* proof_len, void* stream) {
    return capi_merkle_proof_device(ctx, n, tree, m, pos, depth, proof, proof_len, stream, &kMerkleLaunch);
}
extern "C" int plume_merkle_verify_batch(plume_ctx* ctx, int leaf_format, int addr_format, size_t m, const uint8_t* address_or_leaf, const uint8_t* amount, size_t depth,
                                         const uint8_t* proof, const uint8_t* proof_len, const uint8_t* root32, uint8_t* status) {
    return capi_merkle_verify(ctx, leaf_format, addr_format, m, address_or_leaf, amount, depth, proof, proof_len, root32, status, &kMerkleLaunch);
}
extern "C" int plume_merkle_verify_batch_device(plume_ctx* ctx, int leaf_format, int addr_format, size_t m, const uint8_t* address_or_leaf, const uint8_t* amount,
                                                size_t depth, const uint8_t* proof, const uint8_t* proof_len, const uint8_t* root32, uint8_t* status, void* stream) {
    return capi_merkle_verify_device(ctx, leaf_format, addr_format, m, address_or_leaf, amount, depth, proof, proof_len, root32, status, stream, &kMerkleLaunch);
}
