// Host-visible launcher of the self-check's release kernel (plume_selfcheck_kernels.hip; per-lane body in plume_selfcheck.h).
#pragma once
#include <hip/hip_runtime.h>

#include "plume_selfcheck.h"

namespace plume {

// k_sign_release: the caller's six record arrays and status array from the staging, gated by the signer's status and the check's verdict (plume_selfcheck.h)
void launch_sign_release(const ReleaseArgs& a, hipStream_t st);

}  // namespace plume
