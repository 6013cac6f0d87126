// gfx950 kernels of plume_hd_master_batch, plume_hd_derive_priv_batch and plume_hd_derive_pub_batch (plume_hd.h holds the per-lane bodies).  One lane per item,
// 256-thread workgroups; the conversion to affine between the levels is the existing kernel (launch_normalize).
//   k_hd_master                  four SHA-512 compressions, three record stores
//   k_hd_priv_load, k_hd_pub_load  a range check / a point validation, stores into the workspace
//   k_hd_gmul                    the comb of G with the digit-dependent schedule (level 0); k_hd_gmul_uniform<1|2>: the uniform schedule, and the scanned table.  The
//                                floor of four waves the signer's comb kernels have
//   k_hd_priv_step               the HMAC and a sum mod n
//   k_hd_pub_step                the HMAC, the comb and one mixed addition
//   k_hd_finish                  one or two Keccak permutations, up to five record stores
// The resources the compiler settles on are in profiles/hd_kernel_resources.txt.
#define PLUME_COLD_DBL_INLINE   // plume_ec.h: the additions' cold doubling inlined, so that no kernel here has a scratch frame
#include "plume_hd_launch.h"

namespace plume {

constexpr int kHdBlock = 256;
constexpr int kHdGmulWaves = 4;

__global__ __launch_bounds__(kHdBlock) void k_hd_master(HdArgs a) {
    const uint32_t i = blockIdx.x * kHdBlock + threadIdx.x;
    if (i < a.n) hd_master_item(a, i);
}
__global__ __launch_bounds__(kHdBlock) void k_hd_priv_load(HdArgs a) {
    const uint32_t i = blockIdx.x * kHdBlock + threadIdx.x;
    if (i < a.n) hd_priv_load(a, i);
}
__global__ __launch_bounds__(kHdBlock) void k_hd_pub_load(HdArgs a) {
    const uint32_t i = blockIdx.x * kHdBlock + threadIdx.x;
    if (i < a.n) hd_pub_load(a, i);
}
__global__ __launch_bounds__(kHdBlock, kHdGmulWaves) void k_hd_gmul(HdArgs a) {
    const uint32_t i = blockIdx.x * kHdBlock + threadIdx.x;
    if (i < a.n) hd_gmul<0>(a, i);
}
template <int LEVEL>
__global__ __launch_bounds__(kHdBlock, kHdGmulWaves) void k_hd_gmul_uniform(HdArgs a) {
    const uint32_t i = blockIdx.x * kHdBlock + threadIdx.x;
    if (i < a.n) hd_gmul<LEVEL>(a, i);
}
__global__ __launch_bounds__(kHdBlock) void k_hd_priv_step(HdArgs a) {
    const uint32_t i = blockIdx.x * kHdBlock + threadIdx.x;
    if (i < a.n) hd_priv_step(a, i);
}
__global__ __launch_bounds__(kHdBlock) void k_hd_pub_step(HdArgs a) {
    const uint32_t i = blockIdx.x * kHdBlock + threadIdx.x;
    if (i < a.n) hd_pub_step(a, i);
}
__global__ __launch_bounds__(kHdBlock) void k_hd_finish(HdArgs a) {
    const uint32_t i = blockIdx.x * kHdBlock + threadIdx.x;
    if (i < a.n) hd_finish(a, i);
}

static inline unsigned hd_blocks(size_t n) { return (unsigned)((n + kHdBlock - 1) / kHdBlock); }

void launch_hd_master(const HdArgs& a, hipStream_t st) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_hd_master, dim3(hd_blocks(a.n)), dim3(kHdBlock), 0, st, a);
}
void launch_hd_priv_load(const HdArgs& a, hipStream_t st) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_hd_priv_load, dim3(hd_blocks(a.n)), dim3(kHdBlock), 0, st, a);
}
void launch_hd_pub_load(const HdArgs& a, hipStream_t st) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_hd_pub_load, dim3(hd_blocks(a.n)), dim3(kHdBlock), 0, st, a);
}
void launch_hd_gmul(const HdArgs& a, hipStream_t st) {
    if (!a.n) return;
    const dim3 grid(hd_blocks(a.n)), block(kHdBlock);
    if (a.uniform == 2) hipLaunchKernelGGL(k_hd_gmul_uniform<2>, grid, block, 0, st, a);
    else if (a.uniform) hipLaunchKernelGGL(k_hd_gmul_uniform<1>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(k_hd_gmul, grid, block, 0, st, a);
}
void launch_hd_priv_step(const HdArgs& a, hipStream_t st) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_hd_priv_step, dim3(hd_blocks(a.n)), dim3(kHdBlock), 0, st, a);
}
void launch_hd_pub_step(const HdArgs& a, hipStream_t st) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_hd_pub_step, dim3(hd_blocks(a.n)), dim3(kHdBlock), 0, st, a);
}
void launch_hd_finish(const HdArgs& a, hipStream_t st) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_hd_finish, dim3(hd_blocks(a.n)), dim3(kHdBlock), 0, st, a);
}

}  // namespace plume
