// Host-visible launchers of the ECDSA recovery kernels (plume_ecdsa_kernels.hip; per-lane bodies in plume_ecdsa.h).
#pragma once
#include <hip/hip_runtime.h>

#include "plume_ecdsa.h"

namespace plume {

// k_ecdsa_prepare: validation, R, r^-1, u1, the digits of u2, table job i; empties the redo list
void launch_ecdsa_prepare(const EcdsaArgs& a, hipStream_t st);
// k_ecdsa_mul + k_ecdsa_mul_redo: Q = u2 R + u1 G (Jacobian), the second launch redoing with checked additions whatever the first one filed
void launch_ecdsa_mul(const EcdsaArgs& a, hipStream_t st);
// k_ecdsa_finalize: Keccak-256, the records and the status, from the affine results
void launch_ecdsa_finalize(const EcdsaArgs& a, hipStream_t st);

}  // namespace plume
