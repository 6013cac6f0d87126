// gfx950 kernels of plume_ecdsa_recover_batch (plume_ecdsa.h holds the per-lane bodies).  One lane per item, 256-thread workgroups; the table stage and the conversion to
// affine between them are the existing kernels (launch_tables, launch_normalize).
//   k_ecdsa_prepare    a square root (253 squarings), an inversion mod n (20 x 30 divsteps), three products mod n, one GLV split: a floor of three waves per SIMD, the
//                      budget of the other kernels that hold an exponentiation (k_verify_ingest)
//   k_ecdsa_mul        the signer's chain (k_sign_hmul) with one joint slot of 65 positions and the comb's fifteen additions behind it: its floor of four waves, and 65
//                      bytes of LDS per lane for the digit codes (16.25 KiB per workgroup)
//   k_ecdsa_mul_redo   the same lane body with checked additions over the items the hot kernel filed; workgroups of one wavefront, grid-stride, like k_verify_msm_redo:
//                      an honest batch's launch finds nothing
//   k_ecdsa_finalize   the Keccak state twice (50 register pairs) and two 16-word records: no floor beyond the block size, like k_eth_address
// The resources the compiler settles on are in DESIGN.md.
#include <algorithm>

#include "plume_ecdsa_launch.h"

namespace plume {

constexpr int kEcdsaBlock = 256;
constexpr int kEcdsaRedoBlock = 64;
constexpr int kEcdsaPrepareWaves = 3;
constexpr int kEcdsaMulWaves = 4;

__global__ __launch_bounds__(kEcdsaBlock, kEcdsaPrepareWaves) void k_ecdsa_prepare(EcdsaArgs a) {
    const uint32_t i = blockIdx.x * kEcdsaBlock + threadIdx.x;
    if (i == 0) a.redo[0] = 0;                 // the redo list of the multiplication launch behind this one starts empty
    if (i < a.n) ecdsa_prepare(a, i);
}

__global__ __launch_bounds__(kEcdsaBlock, kEcdsaMulWaves) void k_ecdsa_mul(EcdsaArgs a) {
    __shared__ int8_t s_dig[PLUME_NPOS * kEcdsaBlock];
    const uint32_t i = blockIdx.x * kEcdsaBlock + threadIdx.x;
    if (i < a.n) ecdsa_mul<false>(a, i, s_dig + threadIdx.x, kEcdsaBlock);      // (the rows hold digits of s / r: public parts of a signature, nothing to wipe)
}

__global__ __launch_bounds__(kEcdsaRedoBlock, kEcdsaMulWaves) void k_ecdsa_mul_redo(EcdsaArgs a) {
    __shared__ int8_t s_dig[PLUME_NPOS * kEcdsaRedoBlock];
    const uint32_t count = a.redo[0] < a.n ? a.redo[0] : a.n;
    for (uint32_t k = blockIdx.x * kEcdsaRedoBlock + threadIdx.x; k < count; k += gridDim.x * kEcdsaRedoBlock) {
        const uint32_t i = a.redo[1 + k];
        if (i < a.n) ecdsa_mul<true>(a, i, s_dig + threadIdx.x, kEcdsaRedoBlock);
    }
}

__global__ __launch_bounds__(kEcdsaBlock) void k_ecdsa_finalize(EcdsaArgs a) {
    const uint32_t i = blockIdx.x * kEcdsaBlock + threadIdx.x;
    if (i < a.n) ecdsa_finalize(a, i);
}

static inline unsigned ecdsa_blocks(size_t n) { return (unsigned)((n + kEcdsaBlock - 1) / kEcdsaBlock); }

void launch_ecdsa_prepare(const EcdsaArgs& a, hipStream_t st) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_ecdsa_prepare, dim3(ecdsa_blocks(a.n)), dim3(kEcdsaBlock), 0, st, a);
}
void launch_ecdsa_mul(const EcdsaArgs& a, hipStream_t st) {      // (a.redo[0] was zeroed by k_ecdsa_prepare)
    if (!a.n) return;
    hipLaunchKernelGGL(k_ecdsa_mul, dim3(ecdsa_blocks(a.n)), dim3(kEcdsaBlock), 0, st, a);
    const unsigned redo_blocks = std::min(ecdsa_blocks(a.n) * (kEcdsaBlock / kEcdsaRedoBlock), 4096u);   // grid-stride: enough lanes for a wholly crafted batch to fill the chip
    hipLaunchKernelGGL(k_ecdsa_mul_redo, dim3(redo_blocks), dim3(kEcdsaRedoBlock), 0, st, a);
}
void launch_ecdsa_finalize(const EcdsaArgs& a, hipStream_t st) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_ecdsa_finalize, dim3(ecdsa_blocks(a.n)), dim3(kEcdsaBlock), 0, st, a);
}

}  // namespace plume
