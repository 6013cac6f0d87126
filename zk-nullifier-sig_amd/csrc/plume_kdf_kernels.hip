// gfx950 kernels of plume_pbkdf2_sha512_batch (plume_kdf.h holds the per-lane bodies).  One lane per item, 256-thread workgroups.
//   k_kdf_key      the password (hashed first when longer than 128 bytes), the two midstates, U_1: ragged, and cheap beside the loop
//   k_kdf_iter     the hot path: a.iters rounds of two compressions from 32 words of workspace and back.  Two waves per SIMD is the floor: one wave alone issues a
//                  VALU instruction every four cycles, two every two
//   k_kdf_finish   up to 64 byte stores and the status
// The resources the compiler settles on are in profiles/kdf_kernel_resources.txt: no kernel here has a scratch frame.
#include "plume_kdf_launch.h"

namespace plume {

constexpr int kKdfBlock = 256;
constexpr int kKdfIterWaves = 2;

__global__ __launch_bounds__(kKdfBlock) void k_kdf_key(KdfArgs a) {
    const uint32_t i = blockIdx.x * kKdfBlock + threadIdx.x;
    if (i < a.n) kdf_key_item(a, i);
}
__global__ __launch_bounds__(kKdfBlock, kKdfIterWaves) void k_kdf_iter(KdfArgs a) {
    const uint32_t i = blockIdx.x * kKdfBlock + threadIdx.x;
    if (i < a.n) kdf_iter_item(a, i);
}
__global__ __launch_bounds__(kKdfBlock) void k_kdf_finish(KdfArgs a) {
    const uint32_t i = blockIdx.x * kKdfBlock + threadIdx.x;
    if (i < a.n) kdf_finish_item(a, i);
}

static inline unsigned kdf_blocks(size_t n) { return (unsigned)((n + kKdfBlock - 1) / kKdfBlock); }

void launch_kdf_key(const KdfArgs& a, hipStream_t st) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_kdf_key, dim3(kdf_blocks(a.n)), dim3(kKdfBlock), 0, st, a);
}
void launch_kdf_iter(const KdfArgs& a, hipStream_t st) {
    if (!a.n || !a.iters) return;
    hipLaunchKernelGGL(k_kdf_iter, dim3(kdf_blocks(a.n)), dim3(kKdfBlock), 0, st, a);
}
void launch_kdf_finish(const KdfArgs& a, hipStream_t st) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_kdf_finish, dim3(kdf_blocks(a.n)), dim3(kKdfBlock), 0, st, a);
}

}  // namespace plume
