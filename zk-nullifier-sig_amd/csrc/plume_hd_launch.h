// Host-visible launchers of the key-derivation kernels (plume_hd_kernels.hip; per-lane bodies in plume_hd.h).
#pragma once
#include <hip/hip_runtime.h>

#include "plume_hd.h"

namespace plume {

// k_hd_master: HMAC-SHA512("Bitcoin seed", seed) into the caller's sk, chain and status
void launch_hd_master(const HdArgs& a, hipStream_t st);
// k_hd_priv_load / k_hd_pub_load: the parent records into the workspace
void launch_hd_priv_load(const HdArgs& a, hipStream_t st);
void launch_hd_pub_load(const HdArgs& a, hipStream_t st);
// k_hd_gmul: k G of the workspace's k, by the comb at level a.uniform
void launch_hd_gmul(const HdArgs& a, hipStream_t st);
// k_hd_priv_step / k_hd_pub_step: level a.level
void launch_hd_priv_step(const HdArgs& a, hipStream_t st);
void launch_hd_pub_step(const HdArgs& a, hipStream_t st);
// k_hd_finish: the caller's records and status
void launch_hd_finish(const HdArgs& a, hipStream_t st);

}  // namespace plume
