// Host-visible launcher of the derived-nonce kernel (plume_nonce_kernels.hip; per-lane body in plume_nonce.h).
#pragma once
#include <hip/hip_runtime.h>

#include "plume_launch.h"
#include "plume_nonce.h"

namespace plume {

// k_sign_nonce: a.r[i] = the RFC 6979 nonce of item i (plume_nonce.h), one lane per item
void launch_sign_nonce(const NonceArgs& a, hipStream_t st);

}  // namespace plume
