// Host-visible launcher of the transaction kernel (plume_eth_tx_kernels.hip; per-lane body in plume_eth_tx.h).
#pragma once
#include <hip/hip_runtime.h>

#include "plume_eth_tx.h"

namespace plume {

// k_eth_tx_parse: the signing hash, r, s, the parity, the chain id, the type and the status of every raw transaction (plume_eth_tx.h)
void launch_eth_tx_parse(const EthTxArgs& a, hipStream_t st);

}  // namespace plume
