// GPU build of the key-derivation lane bodies -- TEST INFRASTRUCTURE ONLY (never linked into the product library).  One kernel, one lane per element, 64-lane workgroups;
// the element's kind picks the body, so one wavefront runs all of them side by side:
//   kind 0   hd_priv_tweak:   a = IL, b = k_par (32 big-endian bytes each)         ->  out[0:32] = the child, status
//   kind 1   hd_pub_tweak:    a = IL, b || c = K_par as x || y                      ->  out = the child as x || y (zero for the identity), status
//   kind 2   hmac_sha512_37:  a = the key, b || c[0:5] = the 37 bytes of data       ->  out = the 64 digest bytes, status 0
// hg_tweaks allocates, builds the comb the public tweak needs (PLUME_COMB_W = 10: 2 MiB), copies in, launches, synchronises, copies back and frees; returns non-zero on any
// HIP error (text: hg_last_error()) and never aborts.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "plume_hd.h"

using namespace plume;

static std::string g_err;

namespace {
constexpr unsigned kWave = 64;

__global__ __launch_bounds__(kWave) void k_comb_bases(uint32_t* base18) {
    const uint32_t w = blockIdx.x * kWave + threadIdx.x;
    if (w < PLUME_COMB_WINDOWS) fixed_window_base(base18 + (size_t)w * 2 * PLUME_FE_W, PLUME_COMB_W * w);
}
__global__ __launch_bounds__(kWave) void k_comb_rows(uint32_t* rows, const uint32_t* base18) {
    const size_t lane = (size_t)blockIdx.x * kWave + threadIdx.x;
    if (lane < (size_t)PLUME_COMB_ENTRIES * PLUME_COMB_WINDOWS) fixed_table_lane(rows, base18, PLUME_COMB_ENTRIES, lane);
}
__global__ __launch_bounds__(kWave) void k_hd_tweaks(uint32_t count, const uint8_t* kind, const uint8_t* a, const uint8_t* b, const uint8_t* c, const uint32_t* comb, uint8_t* out,
                                                     uint32_t* status) {
    const uint32_t i = blockIdx.x * kWave + threadIdx.x;
    if (i >= count) return;
    const uint8_t *pa = a + 32 * (size_t)i, *pb = b + 32 * (size_t)i, *pc = c + 32 * (size_t)i;
    uint8_t* po = out + 64 * (size_t)i;
    uint32_t st = 0, rec[16];
    PLUME_UNROLL for (int j = 0; j < 16; j++) rec[j] = 0u;
    if (kind[i] == 0) {
        sc il, kp, kc;
        sc_from_be_aligned(il, pa); sc_from_be_aligned(kp, pb);
        st = hd_priv_tweak(kc, il, kp);
        sc_to_record(rec, kc);
    } else if (kind[i] == 1) {
        sc il;
        fe x, y;
        sc_from_be_aligned(il, pa);
        fe_from_be_aligned(x, pb); fe_from_be_aligned(y, pc);
        jac ch;
        st = hd_pub_tweak(ch, il, x, y, comb);
        if (!ch.inf) {
            fe zi, zi2, ax, ay;
            uint32_t xw[8], yw[8];
            fe_inv(zi, ch.z); fe_sqr(zi2, zi);
            fe_mul(ax, ch.x, zi2); fe_mul(zi2, zi2, zi); fe_mul(ay, ch.y, zi2);
            fe_normalize(ax); fe_normalize(ay);
            fe_to_words(xw, ax); fe_to_words(yw, ay);
            recover_record(rec, PLUME_RCV_FMT_AFFINE64, xw, yw, false);
        }
    } else {
        uint32_t key[8], body[8];
        be_words_load(key, pa);
        PLUME_UNROLL for (int j = 0; j < 8; j++) {
            const int p = 1 + 4 * j;                                            // data bytes 1 .. 32: b[1 .. 32) and c[0]
            uint32_t w = 0;
            PLUME_UNROLL for (int q = 0; q < 4; q++) w = (w << 8) | (p + q < 32 ? pb[p + q] : pc[p + q - 32]);
            body[j] = w;
        }
        const uint32_t idx = ((uint32_t)pc[1] << 24) | ((uint32_t)pc[2] << 16) | ((uint32_t)pc[3] << 8) | pc[4];
        Hmac512Key hk;
        hmac_sha512_key32(hk, key);
        uint64_t d[8];
        hmac_sha512_37(d, hk, pb[0], body, idx);
        PLUME_UNROLL for (int j = 0; j < 8; j++) { rec[2 * j] = bswap32((uint32_t)(d[j] >> 32)); rec[2 * j + 1] = bswap32((uint32_t)d[j]); }
    }
    recover_store<64>(po, rec);
    status[i] = st;
}

struct Bufs {
    std::vector<void*> p;
    bool ok = true;
    bool check(hipError_t e, const char* what) {
        if (e != hipSuccess && ok) { ok = false; g_err = std::string("hg_tweaks: ") + what + ": " + hipGetErrorString(e); }
        return e == hipSuccess;
    }
    void* alloc(size_t bytes) {
        void* q = nullptr;
        if (!ok || !check(hipMalloc(&q, bytes ? bytes : 1), "hipMalloc")) return nullptr;
        p.push_back(q);
        return q;
    }
    void* in(const void* host, size_t bytes) {
        void* q = alloc(bytes);
        if (q && bytes) check(hipMemcpy(q, host, bytes, hipMemcpyHostToDevice), "hipMemcpy (in)");
        return q;
    }
    ~Bufs() { for (void* q : p) (void)hipFree(q); }
};
}  // namespace

extern "C" {
const char* hg_last_error(void) { return g_err.c_str(); }

int hg_tweaks(uint32_t count, const uint8_t* kind, const uint8_t* a, const uint8_t* b, const uint8_t* c, uint8_t* out, uint32_t* status) {
    g_err.clear();
    Bufs m;
    uint32_t* base = (uint32_t*)m.alloc((size_t)PLUME_COMB_WINDOWS * 2 * PLUME_FE_WORDS * 4);
    uint32_t* comb = (uint32_t*)m.alloc((size_t)PLUME_COMB_WORDS * 4);
    const uint8_t *dk = (const uint8_t*)m.in(kind, count), *da = (const uint8_t*)m.in(a, 32 * (size_t)count), *db = (const uint8_t*)m.in(b, 32 * (size_t)count),
                  *dc = (const uint8_t*)m.in(c, 32 * (size_t)count);
    uint8_t* dout = (uint8_t*)m.alloc(64 * (size_t)count);
    uint32_t* dst = (uint32_t*)m.alloc(4 * (size_t)count);
    if (!m.ok) return 1;
    hipLaunchKernelGGL(k_comb_bases, dim3((PLUME_COMB_WINDOWS + kWave - 1) / kWave), dim3(kWave), 0, 0, base);
    hipLaunchKernelGGL(k_comb_rows, dim3((unsigned)(((size_t)PLUME_COMB_ENTRIES * PLUME_COMB_WINDOWS + kWave - 1) / kWave)), dim3(kWave), 0, 0, comb, base);
    if (count) hipLaunchKernelGGL(k_hd_tweaks, dim3((count + kWave - 1) / kWave), dim3(kWave), 0, 0, count, dk, da, db, dc, comb, dout, dst);
    if (!m.check(hipGetLastError(), "kernel launch") || !m.check(hipDeviceSynchronize(), "hipDeviceSynchronize")) return 1;
    if (count) { m.check(hipMemcpy(out, dout, 64 * (size_t)count, hipMemcpyDeviceToHost), "hipMemcpy (out)"); m.check(hipMemcpy(status, dst, 4 * (size_t)count, hipMemcpyDeviceToHost), "hipMemcpy (out)"); }
    return m.ok ? 0 : 1;
}
}
