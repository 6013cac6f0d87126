// gfx950 kernel of the signer's self-check gate (plume_selfcheck.h holds the per-lane body and the layout).  A copy kernel: blockIdx.y is the record (pk, nullifier,
// c, s, r_point, hashed_to_curve_r, status), a lane owns one 16-byte quad of that record's caller array, so a wavefront stores 1 KiB of consecutive bytes.
#include "plume_selfcheck_launch.h"

namespace plume {

constexpr int kReleaseBlock = 256;

__global__ __launch_bounds__(kReleaseBlock) void k_sign_release(ReleaseArgs a) {
    sign_release_lane(a, (int)blockIdx.y, (size_t)blockIdx.x * kReleaseBlock + threadIdx.x);
}

void launch_sign_release(const ReleaseArgs& a, hipStream_t st) {
    size_t quads = 0;
    for (int k = 0; k < PLUME_RELEASE_RECORDS; k++) { const size_t q = release_quads(a, k); if (q > quads) quads = q; }
    if (!quads) return;
    hipLaunchKernelGGL(k_sign_release, dim3((unsigned)((quads + kReleaseBlock - 1) / kReleaseBlock), PLUME_RELEASE_RECORDS), dim3(kReleaseBlock), 0, st, a);
}

}  // namespace plume
