// Host-visible launchers of the ECDSA signing kernels (plume_ecdsa_sign_kernels.hip; per-lane bodies in plume_ecdsa_sign.h).
#pragma once
#include <hip/hip_runtime.h>

#include "plume_ecdsa_sign.h"

namespace plume {

// k_ecdsa_sign_nonce: the range check of sk and the RFC 6979 nonce of every item, into the workspace
void launch_ecdsa_sign_nonce(const EcdsaSignArgs& a, hipStream_t st);
// k_ecdsa_sign_gmul (level 0) / k_ecdsa_sign_gmul_uniform<1|2>: k G -- and sk G when a.ntask is 2 -- by the comb, Jacobian
void launch_ecdsa_sign_gmul(const EcdsaSignArgs& a, hipStream_t st);
// k_ecdsa_sign_finalize: r, k^-1, s, low-s, v, the stores, from the affine results
void launch_ecdsa_sign_finalize(const EcdsaSignArgs& a, hipStream_t st);
// k_ecdsa_sign_release: the self-check's gate between the staging and the caller's arrays
void launch_ecdsa_sign_release(const EcdsaSignReleaseArgs& a, hipStream_t st);

}  // namespace plume
