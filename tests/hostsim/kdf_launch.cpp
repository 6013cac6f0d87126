// TEST INFRASTRUCTURE ONLY: the launchers of csrc/plume_kdf_launch.h for the CPU build of the library's host side (tests/test_kdf_hostsim.py), in the style of
// hd_launch.cpp: a launch queues on the mock runtime's stream a plain loop over the same grid as the kernel (csrc/plume_kdf_kernels.hip), calling the same per-lane body
// (csrc/plume_kdf.h) on the same buffers.  Lanes run last-to-first.
#include "plume_kdf_launch.h"

namespace plume {

void launch_kdf_key(const KdfArgs& a0, hipStream_t st) {
    if (!a0.n) return;
    mockhip::launch(st, [a0] { for (uint32_t i = a0.n; i-- > 0;) kdf_key_item(a0, i); });
}
void launch_kdf_iter(const KdfArgs& a0, hipStream_t st) {
    if (!a0.n || !a0.iters) return;
    mockhip::launch(st, [a0] { for (uint32_t i = a0.n; i-- > 0;) kdf_iter_item(a0, i); });
}
void launch_kdf_finish(const KdfArgs& a0, hipStream_t st) {
    if (!a0.n) return;
    mockhip::launch(st, [a0] { for (uint32_t i = a0.n; i-- > 0;) kdf_finish_item(a0, i); });
}

}  // namespace plume
