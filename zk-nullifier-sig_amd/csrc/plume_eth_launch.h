// Host-visible launcher of the Ethereum-address kernel (plume_eth_kernels.hip; per-lane body in plume_keccak.h).
#pragma once
#include <hip/hip_runtime.h>

#include "plume_keccak.h"

namespace plume {

// k_eth_address: the address record and the status of every item, from the caller's keys alone (plume_keccak.h)
void launch_eth_address(const EthArgs& a, hipStream_t st);

}  // namespace plume
