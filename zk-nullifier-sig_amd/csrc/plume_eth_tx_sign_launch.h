// Host-visible launchers of the transaction signer's kernels (plume_eth_tx_sign_kernels.hip; per-lane bodies in plume_eth_tx_sign.h).
#pragma once
#include <hip/hip_runtime.h>

#include "plume_eth_tx_sign.h"

namespace plume {

// k_eth_tx_sign_frame: the framing of every unsigned transaction and its signing hash, into the staging
void launch_eth_tx_sign_frame(const EthTxSignArgs& a, hipStream_t st);
// k_eth_tx_sign_assemble: the signed transaction into its slot, out_len, status and the optional records
void launch_eth_tx_sign_assemble(const EthTxSignArgs& a, hipStream_t st);

}  // namespace plume
