// GPU build of the unit-test lane bodies -- TEST INFRASTRUCTURE ONLY (never linked into the product library).
// tests/devsim/lane_ops.h holds the per-element bodies that tests/devsim/devsim.cpp loops over on the host; here the same bodies run on gfx950, one lane per element in
// 64-lane workgroups, so that the DEVICE branch of every product in plume_fe_mul.inc (the inline-asm multiply-add chains), the device forms of mad_i64 / sel32 / opaque_*
// and the GPU's double precision meet the same edge cases as the host branch does.  The op is a template parameter of every kernel (one instantiation per op, chosen by
// a host-side switch): each op is compiled the way a production kernel sees it.  The dg_* functions mirror their ds_* twins argument for argument; each allocates, copies
// in, launches, synchronises, copies back and frees, returns non-zero on any HIP error (text: dg_last_error()) and never aborts.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "lane_ops.h"

namespace L = plume_lanes;

static std::string g_err;

namespace {
constexpr unsigned kWave = 64;

// one call's device buffers: the first error is kept, everything after it is skipped, every buffer is freed at the end
class Call {
    const char* name_;
    std::vector<void*> bufs_;
    bool ok_ = true;
    void* alloc(size_t bytes) {
        void* p = nullptr;
        if (!check(hipMalloc(&p, bytes ? bytes : 1), "hipMalloc")) return nullptr;
        bufs_.push_back(p);
        return p;
    }
public:
    explicit Call(const char* name) : name_(name) { g_err.clear(); }
    bool ok() const { return ok_; }
    bool check(hipError_t e, const char* what) {
        if (e != hipSuccess && ok_) { ok_ = false; g_err = std::string(name_) + ": " + what + ": " + hipGetErrorString(e); }
        return e == hipSuccess;
    }
    void fail(const char* what) { if (ok_) { ok_ = false; g_err = std::string(name_) + ": " + what; } }
    template <class T> T* in(const T* host, size_t count) {
        if (!ok_) return nullptr;
        T* p = (T*)alloc(count * sizeof(T));
        if (p && count) check(hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy (in)");
        return ok_ ? p : nullptr;
    }
    template <class T> T* out(size_t count) {
        if (!ok_) return nullptr;
        T* p = (T*)alloc(count * sizeof(T));
        if (p && count) check(hipMemset(p, 0, count * sizeof(T)), "hipMemset");
        return ok_ ? p : nullptr;
    }
    template <class T> void back(T* host, const T* dev, size_t count) {
        if (ok_ && count) check(hipMemcpy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost), "hipMemcpy (out)");
    }
    void sync() {
        if (!ok_) return;
        if (check(hipGetLastError(), "kernel launch")) check(hipDeviceSynchronize(), "hipDeviceSynchronize");
    }
    int finish() {
        for (void* p : bufs_) check(hipFree(p), "hipFree");
        bufs_.clear();
        return ok_ ? 0 : 1;
    }
};
inline dim3 grid_for(size_t count) { return dim3((unsigned)((count + kWave - 1) / kWave)); }

template <int OP>
__global__ __launch_bounds__(64) void k_fe_op(size_t count, const uint32_t* a, const uint32_t* b, uint32_t* out) {
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    if (i < count) L::fe_op<OP>(a + 8 * i, b + 8 * i, out + 8 * i);
}
template <int OP>
__global__ __launch_bounds__(64) void k_fe_raw(size_t count, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* e, uint32_t* out) {
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    if (i < count) L::fe_raw<OP>(a + 9 * i, b + 9 * i, c + 9 * i, e + 9 * i, out + L::kFeRawOutWords * i);
}
template <int OP>
__global__ __launch_bounds__(64) void k_group_raw(size_t count, const uint32_t* px, const uint32_t* py, const uint32_t* pz, const uint32_t* qx, const uint32_t* qy, uint32_t* out) {
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    if (i < count) L::group_raw<OP>(px + 9 * i, py + 9 * i, pz + 9 * i, qx + 9 * i, qy + 9 * i, out + 27 * i);
}
template <int OP>
__global__ __launch_bounds__(64) void k_sc_op(size_t count, const uint32_t* a, const uint32_t* b, uint32_t* out) {
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    if (i < count) L::sc_op<OP>(a + 8 * i, b + 8 * i, out + 8 * i);
}
__global__ __launch_bounds__(64) void k_glv(size_t count, const uint32_t* k, uint32_t* out, int8_t* digits) {
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    if (i < count) L::glv(k + 8 * i, out + 10 * i, digits + PLUME_NPOS * i);
}
__global__ __launch_bounds__(64) void k_sha256(const uint8_t* data, uint32_t len, uint8_t* out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) L::sha256(data, len, out);
}
__global__ __launch_bounds__(64) void k_eis_half_gcd(uint32_t n, const uint8_t* c_be, uint8_t* out, uint8_t* tau_be, uint8_t* okf) {
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    if (i < n) L::eis_half_gcd_lane(c_be + 32 * i, out + 64 * i, tau_be + 32 * i, okf + i);
}
template <int WHICH>
__global__ __launch_bounds__(64) void k_eis_consistent(uint32_t n, const uint8_t* c_be, uint8_t* out) {
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    if (i < n) L::eis_consistent_lane<WHICH>(c_be + 32 * i, out + i);
}
__global__ __launch_bounds__(64) void k_eisd_entries(uint32_t* out) {
    const uint32_t idx = blockIdx.x * kWave + threadIdx.x;
    if (idx < 81u) L::eisd_entries_lane(idx, out + 2 * idx);
}
template <int OP>
__global__ __launch_bounds__(64) void k_h2c_op(size_t count, const uint32_t* in, uint32_t* out) {
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    if (i < count) L::h2c_op<OP>(in + L::kH2cInWords * i, out + L::kH2cOutWords * i);
}
template <int CAP, bool AUX>
__global__ __launch_bounds__(64) void k_rfc6979(size_t count, const uint32_t* q, const uint32_t* x, const uint32_t* h1, const uint32_t* aux, uint32_t* k, uint32_t* used) {
    const size_t i = (size_t)blockIdx.x * kWave + threadIdx.x;
    if (i < count) L::rfc6979_lane<CAP, AUX>(q + 8 * i, x + 8 * i, h1 + 8 * i, aux + 8 * i, k + 8 * i, used + i);
}
}  // namespace

extern "C" {
const char* dg_last_error(void) { return g_err.c_str(); }

int dg_fe_op(int op, size_t count, const uint32_t* a, const uint32_t* b, uint32_t* out) {
    Call c("dg_fe_op");
    const uint32_t *da = c.in(a, 8 * count), *db = c.in(b, 8 * count);
    uint32_t* dout = c.out<uint32_t>(8 * count);
    if (c.ok() && count && !L::dispatch<L::kFeOps>(op, [&](auto OP) { hipLaunchKernelGGL(k_fe_op<decltype(OP)::value>, grid_for(count), dim3(kWave), 0, 0, count, da, db, dout); }))
        c.fail("no such op");
    c.sync();
    c.back(out, dout, 8 * count);
    return c.finish();
}
int dg_fe_raw(int op, size_t count, const uint32_t* a, const uint32_t* b, const uint32_t* cc, const uint32_t* e, uint32_t* out) {
    Call c("dg_fe_raw");
    const uint32_t *da = c.in(a, 9 * count), *db = c.in(b, 9 * count), *dc = c.in(cc, 9 * count), *de = c.in(e, 9 * count);
    uint32_t* dout = c.out<uint32_t>(L::kFeRawOutWords * count);
    if (c.ok() && count && !L::dispatch<L::kFeRawOps>(op, [&](auto OP) { hipLaunchKernelGGL(k_fe_raw<decltype(OP)::value>, grid_for(count), dim3(kWave), 0, 0, count, da, db, dc, de, dout); }))
        c.fail("no such op");
    c.sync();
    c.back(out, dout, L::kFeRawOutWords * count);
    return c.finish();
}
int dg_group_raw(int op, size_t count, const uint32_t* px, const uint32_t* py, const uint32_t* pz, const uint32_t* qx, const uint32_t* qy, uint32_t* out) {
    Call c("dg_group_raw");
    const uint32_t *dpx = c.in(px, 9 * count), *dpy = c.in(py, 9 * count), *dpz = c.in(pz, 9 * count), *dqx = c.in(qx, 9 * count), *dqy = c.in(qy, 9 * count);
    uint32_t* dout = c.out<uint32_t>(27 * count);
    if (c.ok() && count && !L::dispatch<L::kGroupRawOps>(op, [&](auto OP) {
            hipLaunchKernelGGL(k_group_raw<decltype(OP)::value>, grid_for(count), dim3(kWave), 0, 0, count, dpx, dpy, dpz, dqx, dqy, dout); }))
        c.fail("no such op");
    c.sync();
    c.back(out, dout, 27 * count);
    return c.finish();
}
int dg_sc_op(int op, size_t count, const uint32_t* a, const uint32_t* b, uint32_t* out) {
    Call c("dg_sc_op");
    const uint32_t *da = c.in(a, 8 * count), *db = c.in(b, 8 * count);
    uint32_t* dout = c.out<uint32_t>(8 * count);
    if (c.ok() && count && !L::dispatch<L::kScOps>(op, [&](auto OP) { hipLaunchKernelGGL(k_sc_op<decltype(OP)::value>, grid_for(count), dim3(kWave), 0, 0, count, da, db, dout); }))
        c.fail("no such op");
    c.sync();
    c.back(out, dout, 8 * count);
    return c.finish();
}
int dg_glv(size_t count, const uint32_t* k, uint32_t* out, int8_t* digits) {
    Call c("dg_glv");
    const uint32_t* dk = c.in(k, 8 * count);
    uint32_t* dout = c.out<uint32_t>(10 * count);
    int8_t* ddig = c.out<int8_t>((size_t)PLUME_NPOS * count);
    if (c.ok() && count) hipLaunchKernelGGL(k_glv, grid_for(count), dim3(kWave), 0, 0, count, dk, dout, ddig);
    c.sync();
    c.back(out, dout, 10 * count);
    c.back(digits, ddig, (size_t)PLUME_NPOS * count);
    return c.finish();
}
int dg_sha256(const uint8_t* data, uint32_t len, uint8_t out[32]) {
    Call c("dg_sha256");
    const uint8_t* dd = c.in(data, len);
    uint8_t* dout = c.out<uint8_t>(32);
    if (c.ok()) hipLaunchKernelGGL(k_sha256, dim3(1), dim3(kWave), 0, 0, dd, len, dout);
    c.sync();
    c.back(out, dout, 32);
    return c.finish();
}
int dg_eisd_entries(uint32_t* out) {
    Call c("dg_eisd_entries");
    uint32_t* dout = c.out<uint32_t>(162);
    if (c.ok()) hipLaunchKernelGGL(k_eisd_entries, dim3(2), dim3(kWave), 0, 0, dout);
    c.sync();
    c.back(out, dout, 162);
    return c.finish();
}
int dg_eis_half_gcd(uint32_t n, const uint8_t* c_be, uint8_t* out, uint8_t* tau_be, uint8_t* okf) {
    Call c("dg_eis_half_gcd");
    const uint8_t* dc = c.in(c_be, 32 * (size_t)n);
    uint8_t *dout = c.out<uint8_t>(64 * (size_t)n), *dtau = c.out<uint8_t>(32 * (size_t)n), *dok = c.out<uint8_t>(n);
    if (c.ok() && n) hipLaunchKernelGGL(k_eis_half_gcd, grid_for(n), dim3(kWave), 0, 0, n, dc, dout, dtau, dok);
    c.sync();
    c.back(out, dout, 64 * (size_t)n);
    c.back(tau_be, dtau, 32 * (size_t)n);
    c.back(okf, dok, n);
    return c.finish();
}
int dg_eis_consistent(uint32_t n, const uint8_t* c_be, int which, uint8_t* out) {
    Call c("dg_eis_consistent");
    const uint8_t* dc = c.in(c_be, 32 * (size_t)n);
    uint8_t* dout = c.out<uint8_t>(n);
    if (c.ok() && n && !L::dispatch<L::kEisTampers>(which, [&](auto W) { hipLaunchKernelGGL(k_eis_consistent<decltype(W)::value>, grid_for(n), dim3(kWave), 0, 0, n, dc, dout); }))
        c.fail("no such tamper");
    c.sync();
    c.back(out, dout, n);
    return c.finish();
}
int dg_h2c_op(int op, size_t count, const uint32_t* in, uint32_t* out) {
    Call c("dg_h2c_op");
    const uint32_t* din = c.in(in, L::kH2cInWords * count);
    uint32_t* dout = c.out<uint32_t>(L::kH2cOutWords * count);
    if (c.ok() && count && !L::dispatch<L::kH2cOps>(op, [&](auto OP) { hipLaunchKernelGGL(k_h2c_op<decltype(OP)::value>, grid_for(count), dim3(kWave), 0, 0, count, din, dout); }))
        c.fail("no such op");
    c.sync();
    c.back(out, dout, L::kH2cOutWords * count);
    return c.finish();
}
int dg_rfc6979(int cap, int aux_on, size_t count, const uint32_t* q, const uint32_t* x, const uint32_t* h1, const uint32_t* aux, uint32_t* k, uint32_t* used) {
    Call c("dg_rfc6979");
    const uint32_t *dq = c.in(q, 8 * count), *dx = c.in(x, 8 * count), *dh = c.in(h1, 8 * count), *da = c.in(aux, 8 * count);
    uint32_t *dk = c.out<uint32_t>(8 * count), *du = c.out<uint32_t>(count);
    if (c.ok() && count && !L::dispatch_nonce(cap, aux_on, [&](auto CAP, auto AUX) {
            hipLaunchKernelGGL((k_rfc6979<decltype(CAP)::value, decltype(AUX)::value>), grid_for(count), dim3(kWave), 0, 0, count, dq, dx, dh, da, dk, du); }))
        c.fail("no such cap");
    c.sync();
    c.back(k, dk, 8 * count);
    c.back(used, du, count);
    return c.finish();
}
}
