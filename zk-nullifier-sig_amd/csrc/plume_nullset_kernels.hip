// gfx950 kernels of the persistent nullifier set (plume_nullset.h holds the per-lane bodies and the method).  One lane per item (insert, contains), per old
// slot (rehash) or per 16 slots (export); 256-lane workgroups.  All of it is HBM-bound random access: a 64-byte read of the item's own record, about 1.3 tag
// probes at load <= 1/2, a 64-byte gather only where a fingerprint matches or a slot is pending, two atomics per claimant.
#include "plume_nullset_launch.h"

namespace plume {

static inline unsigned ns_blocks(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }
constexpr uint64_t kNsExportSlots = (uint64_t)kBlock * PLUME_NS_EXPORT_PER_LANE;

__global__ __launch_bounds__(kBlock) void k_nullset_probe(NullsetInsertArgs a) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < a.n) nullset_probe(a, i);
}
__global__ __launch_bounds__(kBlock) void k_nullset_commit(NullsetInsertArgs a) {
    __shared__ uint32_t s_cnt[kBlock / 64];
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const bool f = i < a.n ? nullset_commit(a, i) : false;
    const unsigned long long b = __ballot(f);
    if ((threadIdx.x & 63u) == 0) s_cnt[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
        for (int w = 0; w < kBlock / 64; w++) c += s_cnt[w];
        a.blockcnt[blockIdx.x] = c;
    }
}
// one workgroup: the call's fresh items, added to the set's size
__global__ __launch_bounds__(kBlock) void k_nullset_sum(NullsetInsertArgs a, uint32_t nb) {
    __shared__ unsigned long long s_sum[kBlock];
    unsigned long long c = 0;
    for (uint32_t k = threadIdx.x; k < nb; k += kBlock) c += a.blockcnt[k];
    s_sum[threadIdx.x] = c;
    __syncthreads();
    for (int stride = kBlock / 2; stride > 0; stride >>= 1) {
        if ((int)threadIdx.x < stride) s_sum[threadIdx.x] += s_sum[threadIdx.x + stride];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *a.size += s_sum[0];
        if (a.n_fresh) *a.n_fresh = s_sum[0];
    }
}
__global__ __launch_bounds__(kBlock) void k_nullset_contains(NullsetQueryArgs a) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < a.n) nullset_contains(a, i);
}
__global__ __launch_bounds__(kBlock) void k_nullset_rehash(NullsetTable from, uint64_t from_cap, NullsetTable to) {
    const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s < from_cap) nullset_rehash(from, to, s);
}

// export, 1: FULL slots per block of kNsExportSlots (lane t takes slots base + k * 256 + t: coalesced tag reads)
__global__ __launch_bounds__(kBlock) void k_nullset_export_count(NullsetExportArgs a) {
    __shared__ uint32_t s_cnt[kBlock / 64];
    const uint64_t base = (uint64_t)blockIdx.x * kNsExportSlots;
    uint32_t c = 0;
    for (uint32_t k = 0; k < PLUME_NS_EXPORT_PER_LANE; k++) {
        const uint64_t s = base + (uint64_t)k * kBlock + threadIdx.x;
        const bool f = s < a.cap && nullset_slot_full(a.t, s);
        c += (uint32_t)__popcll(__ballot(f));
    }
    if ((threadIdx.x & 63u) == 0) s_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < kBlock / 64; w++) t += s_cnt[w];
        a.blockcnt[blockIdx.x] = t;
    }
}
// export, 2: one workgroup turns the block counts into first output rows (exclusive scan, in place) and writes the total
__global__ __launch_bounds__(kBlock) void k_nullset_export_scan(NullsetExportArgs a, uint32_t nb) {
    __shared__ unsigned long long s_sum[kBlock];
    const uint32_t per = (nb + kBlock - 1) / kBlock, lo = threadIdx.x * per, hi = lo + per < nb ? lo + per : nb;
    unsigned long long c = 0;
    for (uint32_t k = lo; k < hi; k++) c += a.blockcnt[k];
    s_sum[threadIdx.x] = c;
    __syncthreads();
    for (int stride = 1; stride < kBlock; stride <<= 1) {           // inclusive Hillis-Steele scan of the lanes' range sums
        const unsigned long long v = (int)threadIdx.x >= stride ? s_sum[threadIdx.x - stride] : 0;
        __syncthreads();
        s_sum[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned long long run = s_sum[threadIdx.x] - c;
    for (uint32_t k = lo; k < hi; k++) { const uint32_t v = a.blockcnt[k]; a.blockcnt[k] = (uint32_t)run; run += v; }
    if (threadIdx.x == kBlock - 1) *a.count = s_sum[kBlock - 1];
}
// export, 3: each block writes its records from its first output row on (order inside the block: by slot)
__global__ __launch_bounds__(kBlock) void k_nullset_export_scatter(NullsetExportArgs a) {
    __shared__ uint32_t s_cnt[kBlock / 64];
    const uint64_t base = (uint64_t)blockIdx.x * kNsExportSlots;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t row = a.blockcnt[blockIdx.x];
    for (uint32_t k = 0; k < PLUME_NS_EXPORT_PER_LANE; k++) {
        const uint64_t s = base + (uint64_t)k * kBlock + threadIdx.x;
        const bool f = s < a.cap && nullset_slot_full(a.t, s);
        const unsigned long long b = __ballot(f);
        if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < kBlock / 64; w++) { before += w < wave ? s_cnt[w] : 0; total += s_cnt[w]; }
        const uint64_t dst = row + before + (uint32_t)__popcll(b & ((1ull << lane) - 1));
        if (f && dst < a.rows) nullset_copy_out(a.t, s, a.out + 64 * dst);
        row += total;
        __syncthreads();
    }
}

size_t nullset_blockcnt_bytes(size_t n) { return (size_t)ns_blocks(n) * 4; }
void launch_nullset_insert(const NullsetInsertArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_nullset_probe, dim3(ns_blocks(a.n)), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(k_nullset_commit, dim3(ns_blocks(a.n)), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(k_nullset_sum, dim3(1), dim3(kBlock), 0, st, a, (uint32_t)ns_blocks(a.n));
}
void launch_nullset_contains(const NullsetQueryArgs& a, hipStream_t st) { hipLaunchKernelGGL(k_nullset_contains, dim3(ns_blocks(a.n)), dim3(kBlock), 0, st, a); }
void launch_nullset_rehash(const NullsetTable& from, uint64_t from_cap, const NullsetTable& to, hipStream_t st) {
    hipLaunchKernelGGL(k_nullset_rehash, dim3(ns_blocks(from_cap)), dim3(kBlock), 0, st, from, from_cap, to);
}
size_t nullset_export_blocks(uint64_t cap) { return (size_t)((cap + kNsExportSlots - 1) / kNsExportSlots); }
void launch_nullset_export(const NullsetExportArgs& a, hipStream_t st) {
    const uint32_t nb = (uint32_t)nullset_export_blocks(a.cap);
    hipLaunchKernelGGL(k_nullset_export_count, dim3(nb), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(k_nullset_export_scan, dim3(1), dim3(kBlock), 0, st, a, nb);
    hipLaunchKernelGGL(k_nullset_export_scatter, dim3(nb), dim3(kBlock), 0, st, a);
}

}  // namespace plume
