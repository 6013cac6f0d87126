// TEST INFRASTRUCTURE ONLY: the launchers of csrc/plume_hd_launch.h for the CPU build of the library's host side (tests/test_hd_hostsim.py), in the style of
// host_launch.cpp: a launch queues on the mock runtime's stream a plain loop over the same grid as the kernel (csrc/plume_hd_kernels.hip), calling the same per-lane body
// (csrc/plume_hd.h) on the same buffers.  Lanes run last-to-first.
// One mutant of the LAUNCHER, for the test that shows the driver notices: -DHD_MUTANT_KEEPS_FAILED lets the finish step leave a byte of the chain code of an item that
// reports a status, as a step that skipped the zeroing of a failed item would.
#include "plume_hd_launch.h"

namespace plume {

void launch_hd_master(const HdArgs& a0, hipStream_t st) {
    if (!a0.n) return;
    mockhip::launch(st, [a0] { for (uint32_t i = a0.n; i-- > 0;) hd_master_item(a0, i); });
}
void launch_hd_priv_load(const HdArgs& a0, hipStream_t st) {
    if (!a0.n) return;
    mockhip::launch(st, [a0] { for (uint32_t i = a0.n; i-- > 0;) hd_priv_load(a0, i); });
}
void launch_hd_pub_load(const HdArgs& a0, hipStream_t st) {
    if (!a0.n) return;
    mockhip::launch(st, [a0] { for (uint32_t i = a0.n; i-- > 0;) hd_pub_load(a0, i); });
}
void launch_hd_gmul(const HdArgs& a0, hipStream_t st) {
    if (!a0.n) return;
    mockhip::launch(st, [a0] {
        for (uint32_t i = a0.n; i-- > 0;) {
            if (a0.uniform == 2) hd_gmul<2>(a0, i); else if (a0.uniform == 1) hd_gmul<1>(a0, i); else hd_gmul<0>(a0, i);
        }
    });
}
void launch_hd_priv_step(const HdArgs& a0, hipStream_t st) {
    if (!a0.n) return;
    mockhip::launch(st, [a0] { for (uint32_t i = a0.n; i-- > 0;) hd_priv_step(a0, i); });
}
void launch_hd_pub_step(const HdArgs& a0, hipStream_t st) {
    if (!a0.n) return;
    mockhip::launch(st, [a0] { for (uint32_t i = a0.n; i-- > 0;) hd_pub_step(a0, i); });
}
void launch_hd_finish(const HdArgs& a0, hipStream_t st) {
    if (!a0.n) return;
    mockhip::launch(st, [a0] {
        for (uint32_t i = a0.n; i-- > 0;) {
            hd_finish(a0, i);
#if defined(HD_MUTANT_KEEPS_FAILED)
            if (a0.status[i] && a0.child_chain) a0.child_chain[32 * (size_t)i + 5] = 0x5A;
#endif
        }
    });
}

}  // namespace plume
