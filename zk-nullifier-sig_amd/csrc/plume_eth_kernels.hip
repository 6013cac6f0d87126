// gfx950 kernels of plume_eth_address_batch and plume_eth_message_hash_batch (plume_keccak.h holds the per-lane bodies).
// k_eth_address: Keccak-256 of every public key, its last 20 bytes as an address record, a status.
// One lane per item, 256-thread workgroups.  No launch-bounds floor beyond the block size: the lane holds the 25-lane state twice (50 register pairs) for the
// permutation and a field element or three for the curve equation; the resources the compiler settles on are in DESIGN.md.
#include "plume_eth_launch.h"

namespace plume {

constexpr int kEthBlock = 256;

__global__ __launch_bounds__(kEthBlock) void k_eth_address(EthArgs a) {
    const uint32_t i = blockIdx.x * kEthBlock + threadIdx.x;
    if (i < a.n) eth_address_item(a, i);
}

// Keccak-256 of every ragged message, plain or behind the EIP-191 prefix: the same state twice and a handful of words for the stream's position
__global__ __launch_bounds__(kEthBlock) void k_eth_message_hash(EthHashArgs a) {
    const uint32_t i = blockIdx.x * kEthBlock + threadIdx.x;
    if (i < a.n) eth_message_hash_item(a, i);
}

void launch_eth_address(const EthArgs& a, hipStream_t st) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_eth_address, dim3((a.n + kEthBlock - 1) / kEthBlock), dim3(kEthBlock), 0, st, a);
}
void launch_eth_message_hash(const EthHashArgs& a, hipStream_t st) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_eth_message_hash, dim3((a.n + kEthBlock - 1) / kEthBlock), dim3(kEthBlock), 0, st, a);
}

}  // namespace plume
