// gfx950 kernel of plume_eth_tx_parse_batch and plume_eth_tx_sender_batch (plume_eth_tx.h holds the per-lane body).
// k_eth_tx_parse: frames every raw transaction, Keccak-256 of its unsigned payload, the signature fields as the recover stages take them.
// One lane per item, 256-thread workgroups, like k_eth_message_hash: the same state twice, the stream's lanes and a handful of words for the walk over the top-level items.
#include "plume_eth_tx_launch.h"

namespace plume {

constexpr int kEthTxBlock = 256;

__global__ __launch_bounds__(kEthTxBlock) void k_eth_tx_parse(EthTxArgs a) {
    const uint32_t i = blockIdx.x * kEthTxBlock + threadIdx.x;
    if (i < a.n) eth_tx_parse_item(a, i);
}

void launch_eth_tx_parse(const EthTxArgs& a, hipStream_t st) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_eth_tx_parse, dim3((a.n + kEthTxBlock - 1) / kEthTxBlock), dim3(kEthTxBlock), 0, st, a);
}

}  // namespace plume
