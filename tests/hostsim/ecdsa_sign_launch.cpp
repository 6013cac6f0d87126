// TEST INFRASTRUCTURE ONLY: the launchers of csrc/plume_ecdsa_sign_launch.h and the message-hash launcher of csrc/plume_eth_launch.h for the CPU build of the library's
// host side (tests/test_ecdsa_sign_hostsim.py), in the style of host_launch.cpp: a launch queues on the mock runtime's stream a plain loop over the same grid as the kernel
// (csrc/plume_ecdsa_sign_kernels.hip, k_eth_message_hash in csrc/plume_eth_kernels.hip), calling the same per-lane body on the same buffers.  Lanes run last-to-first.
// One mutant of a LAUNCHER, for the test that shows the driver notices: -DECDSA_SIGN_MUTANT_DROPS_STREAM queues the finalize loop on the null stream instead of the stream
// it was given, so nothing orders it behind the conversion to affine or before the download.
#include "plume_ecdsa_sign_launch.h"
#include "plume_eth_launch.h"

namespace plume {

void launch_ecdsa_sign_nonce(const EcdsaSignArgs& a0, hipStream_t st) {
    if (!a0.n) return;
    mockhip::launch(st, [a0] { for (uint32_t i = a0.n; i-- > 0;) (void)ecdsa_sign_nonce(a0, i); });
}
void launch_ecdsa_sign_gmul(const EcdsaSignArgs& a0, hipStream_t st) {
    if (!a0.n) return;
    mockhip::launch(st, [a0] {
        for (uint32_t which = a0.ntask; which-- > 0;)
            for (uint32_t i = a0.n; i-- > 0;) {
                if (a0.uniform == 2) ecdsa_sign_gmul<2>(a0, i, which);
                else if (a0.uniform) ecdsa_sign_gmul<1>(a0, i, which);
                else ecdsa_sign_gmul<0>(a0, i, which);
            }
    });
}
void launch_ecdsa_sign_finalize(const EcdsaSignArgs& a0, hipStream_t st) {
    if (!a0.n) return;
#if defined(ECDSA_SIGN_MUTANT_DROPS_STREAM)
    st = nullptr;
#endif
    mockhip::launch(st, [a0] { for (uint32_t i = a0.n; i-- > 0;) ecdsa_sign_finalize(a0, i); });
}
void launch_ecdsa_sign_release(const EcdsaSignReleaseArgs& a0, hipStream_t st) {
    if (!a0.n) return;
    mockhip::launch(st, [a0] { for (uint32_t i = a0.n; i-- > 0;) ecdsa_sign_release(a0, i); });
}
void launch_eth_message_hash(const EthHashArgs& a0, hipStream_t st) {
    if (!a0.n) return;
    mockhip::launch(st, [a0] { for (uint32_t i = a0.n; i-- > 0;) eth_message_hash_item(a0, i); });
}

}  // namespace plume
