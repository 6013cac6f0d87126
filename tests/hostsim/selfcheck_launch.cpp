// TEST INFRASTRUCTURE ONLY: the launcher of csrc/plume_selfcheck_launch.h for the CPU build of the library's host side (tests/test_selfcheck_hostsim.py), in the style of
// host_launch.cpp: a launch queues on the mock runtime's stream a plain loop over the same grid as k_sign_release (csrc/plume_selfcheck_kernels.hip), calling the same
// per-lane body (csrc/plume_selfcheck.h) on the same buffers.  Lanes run last-to-first.
// Two mutants of the LAUNCHER, for the tests that show the driver notices: -DSELFCHECK_MUTANT_IGNORES_VERDICT releases every item as staged; -DSELFCHECK_RELEASE_NOTHING
// writes nothing at all (the driver's "prefill" mode then proves that nothing but the release kernel writes the caller's arrays).
#include <vector>

#include "plume_selfcheck_launch.h"

namespace plume {

void launch_sign_release(const ReleaseArgs& a0, hipStream_t st) {
#if defined(SELFCHECK_RELEASE_NOTHING)
    (void)a0; (void)st;
#else
    mockhip::launch(st, [a0] {
        ReleaseArgs a = a0;
#if defined(SELFCHECK_MUTANT_IGNORES_VERDICT)
        const std::vector<uint8_t> ones(a.n, 1);
        a.verdict = ones.data();
#endif
        for (int k = PLUME_RELEASE_RECORDS; k-- > 0;)
            for (size_t g = release_quads(a, k); g-- > 0;) sign_release_lane(a, k, g);
    });
#endif
}

}  // namespace plume
