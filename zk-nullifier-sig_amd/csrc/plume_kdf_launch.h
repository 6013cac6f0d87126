// Host-visible launchers of the PBKDF2 kernels (plume_kdf_kernels.hip; per-lane bodies in plume_kdf.h).
#pragma once
#include <hip/hip_runtime.h>

#include "plume_kdf.h"

namespace plume {

// k_kdf_key: the midstates and U_1 of every item into a.ws
void launch_kdf_key(const KdfArgs& a, hipStream_t st);
// k_kdf_iter: a.iters rounds on a.ws
void launch_kdf_iter(const KdfArgs& a, hipStream_t st);
// k_kdf_finish: the caller's records and status
void launch_kdf_finish(const KdfArgs& a, hipStream_t st);

}  // namespace plume
