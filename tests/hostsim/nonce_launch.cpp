// TEST INFRASTRUCTURE ONLY: the launcher of csrc/plume_nonce_launch.h for the CPU build of the library's host side (tests/test_nonce_hostsim.py), in the style of
// host_launch.cpp: a launch queues on the mock runtime's stream a plain loop over the same grid as k_sign_nonce (csrc/plume_nonce_kernels.hip), calling the same
// per-lane body (csrc/plume_nonce.h) on the same buffers.  Lanes run last-to-first.
#include "plume_nonce_launch.h"

namespace plume {

void launch_sign_nonce(const NonceArgs& a0, hipStream_t st) {
    mockhip::launch(st, [a = a0] { for (uint32_t i = a.n; i-- > 0;) (void)sign_nonce(a, i); });
}

}  // namespace plume
