// gfx950 kernel of the derived-nonce signer (plume_nonce.h holds the per-lane body and the method).  One lane per item, 256-lane workgroups: h1 over the
// ragged message, then RFC 6979's HMAC-SHA-256 chain (16 compressions plain, 18 hedged) with the state in registers; the nonce leaves the lane through
// eight vector stores into the context's workspace, where the sign kernels read it as SignArgs::r.
#include "plume_nonce_launch.h"

namespace plume {

__global__ __launch_bounds__(kBlock) void k_sign_nonce(NonceArgs a) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < a.n) (void)sign_nonce(a, i);
}

void launch_sign_nonce(const NonceArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_sign_nonce, dim3((unsigned)((a.n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a);
}

}  // namespace plume
