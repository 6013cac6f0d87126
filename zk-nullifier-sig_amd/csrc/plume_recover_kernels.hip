// gfx950 kernel of plume_recover_batch (plume_recover.h holds the per-lane body): the last stage of a V2 verify pipeline that writes the two recomputed points and H
// instead of a verdict.  One lane per item, 256-thread workgroups.
// Launch bounds: like k_verify_finalize (plume_kernels.hip, PLUME_FINAL_WAVES) the lane holds up to six encodings and the SHA-256 schedule of a 198-byte preimage; at a
// floor of four waves per SIMD that kernel spilled ~200 registers, so this one asks for two as well.
#include "plume_recover_launch.h"

namespace plume {

constexpr int kRecoverBlock = 256;
constexpr int kRecoverWaves = 2;

__global__ __launch_bounds__(kRecoverBlock, kRecoverWaves) void k_recover_finalize(RecoverArgs a) {
    const uint32_t i = blockIdx.x * kRecoverBlock + threadIdx.x;
    if (i < a.n) recover_finalize(a, i);
}

void launch_recover_finalize(const RecoverArgs& a, hipStream_t st) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_recover_finalize, dim3((a.n + kRecoverBlock - 1) / kRecoverBlock), dim3(kRecoverBlock), 0, st, a);
}

}  // namespace plume
