// TEST INFRASTRUCTURE ONLY: the launcher of csrc/plume_recover_launch.h for the CPU build of the library's host side (tests/test_recover_hostsim.py), in the style of
// host_launch.cpp: a launch queues on the mock runtime's stream a plain loop over the same grid as k_recover_finalize (csrc/plume_recover_kernels.hip), calling the same
// per-lane body (csrc/plume_recover.h) on the same buffers.  Lanes run last-to-first.
// Two mutants of the LAUNCHER, for the tests that show the driver notices: -DRECOVER_MUTANT_WRITES_REJECTED treats every item as accepted (points for items the ingest
// stage rejected); -DRECOVER_MUTANT_WRONG_VERSION hashes the other version's preimage.
#include <vector>

#include "plume_recover_launch.h"

namespace plume {

void launch_recover_finalize(const RecoverArgs& a0, hipStream_t st) {
    mockhip::launch(st, [a0] {
        RecoverArgs a = a0;
#if defined(RECOVER_MUTANT_WRITES_REJECTED)
        const std::vector<uint8_t> none(a.n, 0);
        a.itemflags = none.data();
#endif
#if defined(RECOVER_MUTANT_WRONG_VERSION)
        a.version = 3 - a.version;
#endif
        for (uint32_t i = a.n; i-- > 0;) recover_finalize(a, i);
    });
}

}  // namespace plume
