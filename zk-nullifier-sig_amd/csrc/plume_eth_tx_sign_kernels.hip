// gfx950 kernels of plume_eth_tx_sign_batch (plume_eth_tx_sign.h holds the per-lane bodies).
// k_eth_tx_sign_frame: frames every unsigned transaction and stages its Keccak-256 for the sign stages.  k_eth_tx_sign_assemble: the signed item into its slot.
// One lane per item, 256-thread workgroups, like k_eth_tx_parse.
#include "plume_eth_tx_sign_launch.h"

namespace plume {

constexpr int kEthTxSignBlock = 256;

__global__ __launch_bounds__(kEthTxSignBlock) void k_eth_tx_sign_frame(EthTxSignArgs a) {
    const uint32_t i = blockIdx.x * kEthTxSignBlock + threadIdx.x;
    if (i < a.n) eth_tx_sign_frame_item(a, i);
}

__global__ __launch_bounds__(kEthTxSignBlock) void k_eth_tx_sign_assemble(EthTxSignArgs a) {
    const uint32_t i = blockIdx.x * kEthTxSignBlock + threadIdx.x;
    if (i < a.n) eth_tx_sign_assemble_item(a, i);
}

void launch_eth_tx_sign_frame(const EthTxSignArgs& a, hipStream_t st) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_eth_tx_sign_frame, dim3((a.n + kEthTxSignBlock - 1) / kEthTxSignBlock), dim3(kEthTxSignBlock), 0, st, a);
}
void launch_eth_tx_sign_assemble(const EthTxSignArgs& a, hipStream_t st) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_eth_tx_sign_assemble, dim3((a.n + kEthTxSignBlock - 1) / kEthTxSignBlock), dim3(kEthTxSignBlock), 0, st, a);
}

}  // namespace plume
