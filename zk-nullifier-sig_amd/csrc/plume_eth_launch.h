// Host-visible launchers of the Ethereum-address and message-hash kernels (plume_eth_kernels.hip; per-lane body in plume_keccak.h).
#pragma once
#include <hip/hip_runtime.h>

#include "plume_keccak.h"

namespace plume {

// k_eth_address: the address record and the status of every item, from the caller's keys alone (plume_keccak.h)
void launch_eth_address(const EthArgs& a, hipStream_t st);
// k_eth_message_hash: the 32-byte digest of every ragged message (plume_keccak.h)
void launch_eth_message_hash(const EthHashArgs& a, hipStream_t st);

}  // namespace plume
