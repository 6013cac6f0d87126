// Host-visible launchers of the Merkle kernels (plume_merkle_kernels.hip; per-lane bodies in plume_merkle.h).
#pragma once
#include <hip/hip_runtime.h>

#include "plume_merkle.h"

namespace plume {

// k_merkle_leaf: the leaf and the status of every item
void launch_merkle_leaf(const MerkleLeafArgs& a, hipStream_t st);
// k_merkle_sort_local, then per block size k > tile the k_merkle_sort_global stages and one k_merkle_sort_merge: the records of the leaves, sorted, in a.ws
void launch_merkle_sort(const MerkleSortArgs& a, hipStream_t st);
// k_merkle_place: the leaves at the end of the tree, leaf_pos
void launch_merkle_place(const MerkleTreeArgs& a, hipStream_t st);
// k_merkle_level: the parents of depth d
void launch_merkle_level(uint8_t* tree, uint32_t n, uint32_t d, hipStream_t st);
// k_merkle_top: the parents of depths dtop .. 0 (dtop <= PLUME_MRK_TOP_DEPTH) in one workgroup
void launch_merkle_top(uint8_t* tree, uint32_t n, uint32_t dtop, hipStream_t st);
// k_merkle_proof: the siblings of every requested index
void launch_merkle_proof(const MerkleProofArgs& a, hipStream_t st);
// k_merkle_verify: leaf and processProof of every item against a.root
void launch_merkle_verify(const MerkleVerifyArgs& a, hipStream_t st);

}  // namespace plume
