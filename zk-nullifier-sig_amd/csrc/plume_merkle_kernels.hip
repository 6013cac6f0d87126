// gfx950 kernels of the Merkle calls (plume_merkle.h holds the per-lane bodies).
// k_merkle_leaf, k_merkle_verify, k_merkle_level, k_merkle_top: one lane per item / parent, 256-thread workgroups, the Keccak state in registers like k_eth_address.
// k_merkle_top runs the depths of at most 256 parents in ONE workgroup: depth d + 1 is written by the lanes of this workgroup, the barrier (with its workgroup-scope
// fence) makes it visible to the lanes that hash depth d.  Small allow-lists are the common case, and for them this is the whole tree above the leaves in one launch.
// k_merkle_sort_local / _merge: a tile of at most 2048 records in LDS as nine word arrays (72 KiB: two workgroups per CU), 256 lanes, four pairs per lane and stage, a
// barrier between stages.  Lanes of a wavefront take consecutive pairs: consecutive words of each array for distances of 32 and more, a two-way bank conflict (stride two
// words) for the shortest distances.  k_merkle_sort_global: one stage of a distance of at least the tile, one lane per pair, coalesced through the same layout.
#include "plume_merkle_launch.h"

namespace plume {

constexpr int kMerkleBlock = 256;

__global__ __launch_bounds__(kMerkleBlock) void k_merkle_leaf(MerkleLeafArgs a) {
    const uint32_t i = blockIdx.x * kMerkleBlock + threadIdx.x;
    if (i < a.n) mrk_leaf_item(a, i);
}

__global__ __launch_bounds__(kMerkleBlock) void k_merkle_verify(MerkleVerifyArgs a) {
    const uint32_t i = blockIdx.x * kMerkleBlock + threadIdx.x;
    if (i < a.m) mrk_verify_item(a, i);
}

__global__ __launch_bounds__(kMerkleBlock) void k_merkle_proof(MerkleProofArgs a) {
    const uint32_t i = blockIdx.x * kMerkleBlock + threadIdx.x;
    if (i < a.m) mrk_proof_item(a, i);
}

__global__ __launch_bounds__(kMerkleBlock) void k_merkle_place(MerkleTreeArgs a) {
    const uint32_t i = blockIdx.x * kMerkleBlock + threadIdx.x;
    if (i < a.n) mrk_place_item(a, i);
}

__global__ __launch_bounds__(kMerkleBlock) void k_merkle_level(uint8_t* tree, uint32_t n, uint32_t d) {
    const uint32_t t = blockIdx.x * kMerkleBlock + threadIdx.x;
    if (t < mrk_depth_nodes(n, d)) mrk_node(tree, (size_t)mrk_depth_first(d) + t);
}

__global__ __launch_bounds__(kMerkleBlock) void k_merkle_top(uint8_t* tree, uint32_t n, uint32_t dtop) {
    PLUME_NOUNROLL for (uint32_t d = dtop + 1u; d-- > 0u;) {
        if (threadIdx.x < mrk_depth_nodes(n, d)) mrk_node(tree, (size_t)mrk_depth_first(d) + threadIdx.x);
        __syncthreads();
    }
}

__global__ __launch_bounds__(kMerkleBlock) void k_merkle_sort_local(MerkleSortArgs a) {
    __shared__ uint32_t s[PLUME_MRK_REC_WORDS * PLUME_MRK_TILE];
    const size_t base = (size_t)blockIdx.x * a.tile;
    for (uint32_t x = threadIdx.x; x < a.tile; x += kMerkleBlock) mrk_tile_from_leaves(s, a, base, x);
    __syncthreads();
    PLUME_NOUNROLL for (uint32_t k = 2; k <= a.tile; k <<= 1) {
        PLUME_NOUNROLL for (uint32_t j = k >> 1; j; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < a.tile / 2u; t += kMerkleBlock) mrk_tile_cx(s, a.tile, base, k, j, t);
            __syncthreads();
        }
    }
    for (uint32_t x = threadIdx.x; x < a.tile; x += kMerkleBlock) mrk_tile_to_ws(s, a, base, x);
}

__global__ __launch_bounds__(kMerkleBlock) void k_merkle_sort_merge(MerkleSortArgs a, size_t k) {
    __shared__ uint32_t s[PLUME_MRK_REC_WORDS * PLUME_MRK_TILE];
    const size_t base = (size_t)blockIdx.x * a.tile;
    for (uint32_t x = threadIdx.x; x < a.tile; x += kMerkleBlock) mrk_tile_from_ws(s, a, base, x);
    __syncthreads();
    PLUME_NOUNROLL for (uint32_t j = a.tile >> 1; j; j >>= 1) {
        for (uint32_t t = threadIdx.x; t < a.tile / 2u; t += kMerkleBlock) mrk_tile_cx(s, a.tile, base, k, j, t);
        __syncthreads();
    }
    for (uint32_t x = threadIdx.x; x < a.tile; x += kMerkleBlock) mrk_tile_to_ws(s, a, base, x);
}

__global__ __launch_bounds__(kMerkleBlock) void k_merkle_sort_global(MerkleSortArgs a, size_t k, size_t j) {
    const size_t t = (size_t)blockIdx.x * kMerkleBlock + threadIdx.x;
    if (t < a.npad / 2u) mrk_global_cx(a, k, j, t);
}

static dim3 merkle_grid(size_t lanes) { return dim3((unsigned)((lanes + kMerkleBlock - 1) / kMerkleBlock)); }

void launch_merkle_leaf(const MerkleLeafArgs& a, hipStream_t st) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_merkle_leaf, merkle_grid(a.n), dim3(kMerkleBlock), 0, st, a);
}
void launch_merkle_verify(const MerkleVerifyArgs& a, hipStream_t st) {
    if (!a.m) return;
    hipLaunchKernelGGL(k_merkle_verify, merkle_grid(a.m), dim3(kMerkleBlock), 0, st, a);
}
void launch_merkle_proof(const MerkleProofArgs& a, hipStream_t st) {
    if (!a.m) return;
    hipLaunchKernelGGL(k_merkle_proof, merkle_grid(a.m), dim3(kMerkleBlock), 0, st, a);
}
void launch_merkle_place(const MerkleTreeArgs& a, hipStream_t st) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_merkle_place, merkle_grid(a.n), dim3(kMerkleBlock), 0, st, a);
}
void launch_merkle_level(uint8_t* tree, uint32_t n, uint32_t d, hipStream_t st) {
    const uint32_t cnt = n >= 2u ? mrk_depth_nodes(n, d) : 0u;
    if (!cnt) return;
    hipLaunchKernelGGL(k_merkle_level, merkle_grid(cnt), dim3(kMerkleBlock), 0, st, tree, n, d);
}
void launch_merkle_top(uint8_t* tree, uint32_t n, uint32_t dtop, hipStream_t st) {
    if (n < 2u || dtop > PLUME_MRK_TOP_DEPTH) return;
    hipLaunchKernelGGL(k_merkle_top, dim3(1), dim3(kMerkleBlock), 0, st, tree, n, dtop);
}
void launch_merkle_sort(const MerkleSortArgs& a, hipStream_t st) {
    if (!a.n) return;
    const dim3 tiles(a.npad / a.tile), blk(kMerkleBlock);
    mrk_sort_schedule(a.npad, a.tile,
        [&] { hipLaunchKernelGGL(k_merkle_sort_local, tiles, blk, 0, st, a); },
        [&](size_t k, size_t j) { hipLaunchKernelGGL(k_merkle_sort_global, merkle_grid(a.npad / 2u), blk, 0, st, a, k, j); },
        [&](size_t k) { hipLaunchKernelGGL(k_merkle_sort_merge, tiles, blk, 0, st, a, k); });
}

}  // namespace plume
