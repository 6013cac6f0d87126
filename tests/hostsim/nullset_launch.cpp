// TEST INFRASTRUCTURE ONLY: the launchers of csrc/plume_nullset_launch.h for the CPU build of the library's host side (tests/test_nullset_hostsim.py), in the style of
// host_launch.cpp: each launch queues on the mock runtime's stream a plain loop over the same grid as the kernel of that name in csrc/plume_nullset_kernels.hip, calling the
// same per-lane bodies (csrc/plume_nullset.h) on the same buffers.  The probe lanes run last-to-first, so a claimant is usually NOT the item with the smallest id.
#include <vector>

#include "plume_nullset_launch.h"

namespace plume {

static inline unsigned ns_blocks(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }
static constexpr uint64_t kNsExportSlots = (uint64_t)kBlock * PLUME_NS_EXPORT_PER_LANE;

size_t nullset_blockcnt_bytes(size_t n) { return (size_t)ns_blocks(n) * 4; }
void launch_nullset_insert(const NullsetInsertArgs& a0, hipStream_t st) {
    mockhip::launch(st, [a = a0] { for (uint32_t i = a.n; i-- > 0;) nullset_probe(a, i); });
    mockhip::launch(st, [a = a0] {
        for (unsigned b = 0; b < ns_blocks(a.n); b++) {
            uint32_t c = 0;
            for (unsigned t = 0; t < (unsigned)kBlock; t++) { const uint32_t i = b * kBlock + t; if (i < a.n && nullset_commit(a, i)) c++; }
            a.blockcnt[b] = c;
        }
    });
    mockhip::launch(st, [a = a0] {
        unsigned long long c = 0;
        for (unsigned b = 0; b < ns_blocks(a.n); b++) c += a.blockcnt[b];
        *a.size += c;
        if (a.n_fresh) *a.n_fresh = c;
    });
}
void launch_nullset_contains(const NullsetQueryArgs& a0, hipStream_t st) {
    mockhip::launch(st, [a = a0] { for (uint32_t i = 0; i < a.n; i++) nullset_contains(a, i); });
}
void launch_nullset_rehash(const NullsetTable& from0, uint64_t from_cap, const NullsetTable& to0, hipStream_t st) {
    mockhip::launch(st, [from = from0, to = to0, from_cap] { for (uint64_t s = 0; s < from_cap; s++) nullset_rehash(from, to, s); });
}
size_t nullset_export_blocks(uint64_t cap) { return (size_t)((cap + kNsExportSlots - 1) / kNsExportSlots); }
void launch_nullset_export(const NullsetExportArgs& a0, hipStream_t st) {
    const uint64_t nb = nullset_export_blocks(a0.cap);
    mockhip::launch(st, [a = a0, nb] {
        for (uint64_t b = 0; b < nb; b++) {
            uint32_t c = 0;
            for (uint64_t s = b * kNsExportSlots; s < (b + 1) * kNsExportSlots && s < a.cap; s++) c += nullset_slot_full(a.t, s) ? 1 : 0;
            a.blockcnt[b] = c;
        }
    });
    mockhip::launch(st, [a = a0, nb] {
        unsigned long long run = 0;
        for (uint64_t b = 0; b < nb; b++) { const uint32_t v = a.blockcnt[b]; a.blockcnt[b] = (uint32_t)run; run += v; }
        *a.count = run;
    });
    mockhip::launch(st, [a = a0, nb] {
        for (uint64_t b = 0; b < nb; b++) {
            uint64_t row = a.blockcnt[b];
            for (uint64_t s = b * kNsExportSlots; s < (b + 1) * kNsExportSlots && s < a.cap; s++)
                if (nullset_slot_full(a.t, s) && row < a.rows) nullset_copy_out(a.t, s, a.out + 64 * row++);
        }
    });
}

}  // namespace plume
