// Host-visible launchers of the persistent nullifier set's kernels (plume_nullset_kernels.hip; per-lane bodies in plume_nullset.h).
#pragma once
#include <hip/hip_runtime.h>

#include "plume_launch.h"
#include "plume_nullset.h"

namespace plume {

size_t nullset_blockcnt_bytes(size_t n);                       // size of NullsetInsertArgs::blockcnt
// probe, commit, sum.  a.minid must hold all ones (the caller's memset on the same stream) and the table must stay at most half full after the call
void launch_nullset_insert(const NullsetInsertArgs& a, hipStream_t st);
void launch_nullset_contains(const NullsetQueryArgs& a, hipStream_t st);
// every record of `from` (from_cap slots) into `to`, whose tags must all be EMPTY
void launch_nullset_rehash(const NullsetTable& from, uint64_t from_cap, const NullsetTable& to, hipStream_t st);
size_t nullset_export_blocks(uint64_t cap);                   // entries of NullsetExportArgs::blockcnt
void launch_nullset_export(const NullsetExportArgs& a, hipStream_t st);   // count, scan, scatter

}  // namespace plume
