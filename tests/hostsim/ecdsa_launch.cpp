// TEST INFRASTRUCTURE ONLY: the launchers of csrc/plume_ecdsa_launch.h for the CPU build of the library's host side (tests/test_ecdsa_hostsim.py), in the style of
// host_launch.cpp: a launch queues on the mock runtime's stream a plain loop over the same grid as the kernel (csrc/plume_ecdsa_kernels.hip), calling the same per-lane
// body (csrc/plume_ecdsa.h) on the same buffers.  Lanes run last-to-first; the multiplication's second launch redoes what the first one filed, as on the device.
// One mutant of a LAUNCHER, for the test that shows the driver notices: -DECDSA_MUTANT_DROPS_STREAM queues the finalize loop on the null stream instead of the stream it
// was given, so nothing orders it behind the conversion to affine or before the download (host form) or the caller's synchronise (device form).
#include <vector>

#include "plume_ecdsa_launch.h"

namespace plume {

void launch_ecdsa_prepare(const EcdsaArgs& a0, hipStream_t st) {
    mockhip::launch(st, [a0] {
        a0.redo[0] = 0;
        for (uint32_t i = a0.n; i-- > 0;) ecdsa_prepare(a0, i);
    });
}
void launch_ecdsa_mul(const EcdsaArgs& a0, hipStream_t st) {
    mockhip::launch(st, [a0] {
        std::vector<int8_t> dig(PLUME_NPOS);
        for (uint32_t i = a0.n; i-- > 0;) ecdsa_mul<false>(a0, i, dig.data(), 1);
    });
    mockhip::launch(st, [a0] {
        std::vector<int8_t> dig(PLUME_NPOS);
        const uint32_t count = a0.redo[0] < a0.n ? a0.redo[0] : a0.n;
        for (uint32_t k = 0; k < count; k++) ecdsa_mul<true>(a0, a0.redo[1 + k], dig.data(), 1);
    });
}
void launch_ecdsa_finalize(const EcdsaArgs& a0, hipStream_t st) {
#if defined(ECDSA_MUTANT_DROPS_STREAM)
    st = nullptr;
#endif
    mockhip::launch(st, [a0] {
        for (uint32_t i = a0.n; i-- > 0;) ecdsa_finalize(a0, i);
    });
}

}  // namespace plume
