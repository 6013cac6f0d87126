// gfx950 kernels of plume_ecdsa_sign_batch (plume_ecdsa_sign.h holds the per-lane bodies).  One lane per item (per task in the comb stage), 256-thread workgroups; the
// conversion to affine between the comb and finalize is the existing kernel (launch_normalize).
//   k_ecdsa_sign_nonce           RFC 6979's HMAC-SHA-256 chain with the state in registers, as k_sign_nonce: no floor beyond the block size
//   k_ecdsa_sign_gmul            the comb of G with the digit-dependent schedule (level 0); k_ecdsa_sign_gmul_uniform<1|2>: the uniform schedule, and the scanned table.
//                                The floor of four waves the signer's own comb kernels have (k_sign_gmul, k_sign_gmul_uniform)
//   k_ecdsa_sign_finalize        an inversion mod n (20 x 30 divsteps), two products mod n, four record stores: the floor of three waves of k_ecdsa_prepare
//   k_ecdsa_sign_release         a copy under a 64-byte comparison
// The resources the compiler settles on are in DESIGN.md.
#include "plume_ecdsa_sign_launch.h"

namespace plume {

constexpr int kEcdsaSignBlock = 256;
constexpr int kEcdsaSignGmulWaves = 4;
constexpr int kEcdsaSignFinalizeWaves = 3;

__global__ __launch_bounds__(kEcdsaSignBlock) void k_ecdsa_sign_nonce(EcdsaSignArgs a) {
    const uint32_t i = blockIdx.x * kEcdsaSignBlock + threadIdx.x;
    if (i < a.n) (void)ecdsa_sign_nonce(a, i);
}

// blocks [0, nb): k G; blocks [nb, 2 nb), with the self-check: sk G
__global__ __launch_bounds__(kEcdsaSignBlock, kEcdsaSignGmulWaves) void k_ecdsa_sign_gmul(EcdsaSignArgs a) {
    const uint32_t nb = (a.n + kEcdsaSignBlock - 1) / kEcdsaSignBlock;
    const uint32_t which = blockIdx.x >= nb ? 1u : 0u;
    const uint32_t i = (which ? blockIdx.x - nb : blockIdx.x) * kEcdsaSignBlock + threadIdx.x;
    if (i < a.n) ecdsa_sign_gmul<0>(a, i, which);
}
template <int LEVEL>
__global__ __launch_bounds__(kEcdsaSignBlock, kEcdsaSignGmulWaves) void k_ecdsa_sign_gmul_uniform(EcdsaSignArgs a) {
    const uint32_t nb = (a.n + kEcdsaSignBlock - 1) / kEcdsaSignBlock;
    const uint32_t which = blockIdx.x >= nb ? 1u : 0u;
    const uint32_t i = (which ? blockIdx.x - nb : blockIdx.x) * kEcdsaSignBlock + threadIdx.x;
    if (i < a.n) ecdsa_sign_gmul<LEVEL>(a, i, which);
}

__global__ __launch_bounds__(kEcdsaSignBlock, kEcdsaSignFinalizeWaves) void k_ecdsa_sign_finalize(EcdsaSignArgs a) {
    const uint32_t i = blockIdx.x * kEcdsaSignBlock + threadIdx.x;
    if (i < a.n) ecdsa_sign_finalize(a, i);
}

__global__ __launch_bounds__(kEcdsaSignBlock) void k_ecdsa_sign_release(EcdsaSignReleaseArgs a) {
    const uint32_t i = blockIdx.x * kEcdsaSignBlock + threadIdx.x;
    if (i < a.n) ecdsa_sign_release(a, i);
}

static inline unsigned ecdsa_sign_blocks(size_t n) { return (unsigned)((n + kEcdsaSignBlock - 1) / kEcdsaSignBlock); }

void launch_ecdsa_sign_nonce(const EcdsaSignArgs& a, hipStream_t st) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_ecdsa_sign_nonce, dim3(ecdsa_sign_blocks(a.n)), dim3(kEcdsaSignBlock), 0, st, a);
}
void launch_ecdsa_sign_gmul(const EcdsaSignArgs& a, hipStream_t st) {
    if (!a.n) return;
    const dim3 grid(a.ntask * ecdsa_sign_blocks(a.n)), block(kEcdsaSignBlock);
    if (a.uniform == 2) hipLaunchKernelGGL(k_ecdsa_sign_gmul_uniform<2>, grid, block, 0, st, a);
    else if (a.uniform) hipLaunchKernelGGL(k_ecdsa_sign_gmul_uniform<1>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(k_ecdsa_sign_gmul, grid, block, 0, st, a);
}
void launch_ecdsa_sign_finalize(const EcdsaSignArgs& a, hipStream_t st) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_ecdsa_sign_finalize, dim3(ecdsa_sign_blocks(a.n)), dim3(kEcdsaSignBlock), 0, st, a);
}
void launch_ecdsa_sign_release(const EcdsaSignReleaseArgs& a, hipStream_t st) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_ecdsa_sign_release, dim3(ecdsa_sign_blocks(a.n)), dim3(kEcdsaSignBlock), 0, st, a);
}

}  // namespace plume
