// Host-visible launcher of the recovery call's last kernel (plume_recover_kernels.hip; per-lane body in plume_recover.h).
#pragma once
#include <hip/hip_runtime.h>

#include "plume_recover.h"

namespace plume {

// k_recover_finalize: r_point, hashed_to_curve_r, hashed_to_curve and the status of every item, from what the V2 verify pipeline left in the workspace (plume_recover.h)
void launch_recover_finalize(const RecoverArgs& a, hipStream_t st);

}  // namespace plume
