// The key derivation (include/plume_hip.h, plume_hd_master_batch*, plume_hd_derive_priv_batch*, plume_hd_derive_pub_batch*): its C ABI and its host side.  master is one
// kernel on the caller's arrays: no table, no workspace.  The derive calls use the signer's table of G (the public form: the comb) and its result array, and ctx->hdws for k,
// the chain code and the status of every item between the levels (65 B / item): load, then per level the comb (private form: at the context's uniform level), the conversion
// to affine and the step kernel, then finish into the caller's arrays.  They join the ws_free chain and are cut by plume_set_sub_batches as an ECDSA signing call is.  Behind
// the last finish the staging and the Jacobian images are wiped on the call's stream; a call that fails half way wipes them too (StageWipe), in front of ws_free.  The
// host-pointer forms are serial calls (serial_host_call_any): sk, chain codes and seeds staged as secrets -- inputs and outputs --, a shared parent or path as whole-call
// inputs.
#include <cstring>

#include "../../include/plume_hip.h"
#include "plume_capi_ctx.h"
#include "plume_hd_launch.h"

using namespace plume;

static_assert(PLUME_HD_MAX_DEPTH == PLUME_HDK_MAX_DEPTH && PLUME_HD_SHARED_PARENT == PLUME_HDK_SHARED_PARENT && PLUME_HD_SHARED_PATH == PLUME_HDK_SHARED_PATH &&
                  PLUME_STATUS_HD_NO_KEY == PLUME_ST_HD_NO_KEY && PLUME_STATUS_HD_HARDENED == PLUME_ST_HD_HARDENED,
              "the header and the kernels state the same constants");

static int hd_master_args_ok(size_t n, const void* seed, size_t seed_len, const void* sk, const void* chain, const void* status) {
    if (seed_len < 16 || seed_len > 64) return fail(PLUME_ERR_ARG, "seed_len must be 16 .. 64");
    if (n && (!seed || !sk || !chain || !status)) return fail(PLUME_ERR_ARG, "null array");
    if (n > 0xFFFFFFF0u / 64) return fail(PLUME_ERR_ARG, "n too large");
    return 0;
}
static int hd_master_device(plume_ctx* ctx, size_t n, const uint8_t* seed, size_t seed_len, uint8_t* sk, uint8_t* chain, uint8_t* status, hipStream_t st) {
    if (n == 0) return 0;
    HdArgs a;
    memset(&a, 0, sizeof a);
    a.n = (uint32_t)n; a.seed_len = (uint32_t)seed_len; a.parent = seed; a.child_sk = sk; a.child_chain = chain; a.status = status;
    ctx->timer.begin(st);
    launch_hd_master(a, st); ctx->timer.stage("hd_master", st);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int plume_hd_master_batch_device(plume_ctx* ctx, size_t n, const uint8_t* seed, size_t seed_len, uint8_t* sk, uint8_t* chain, uint8_t* status, void* stream) {
    Route rt_(ctx, stream); ctx = rt_.lane; const hipStream_t st_ = rt_.st;
    if (int rc = bind(ctx)) return rc;
    if (int rc = hd_master_args_ok(n, seed, seed_len, sk, chain, status)) return rc;
    return hd_master_device(ctx, n, seed, seed_len, sk, chain, status, st_);
}
extern "C" int plume_hd_master_batch(plume_ctx* ctx, size_t n, const uint8_t* seed, size_t seed_len, uint8_t* sk, uint8_t* chain, uint8_t* status) {
    if (!ctx) return fail(PLUME_ERR_ARG, "null context");
    if (int rc = hd_master_args_ok(n, seed, seed_len, sk, chain, status)) return rc;
    const HostCall call{nullptr, nullptr, {{seed, seed_len, true}}, {{sk, 32, true}, {chain, 32, true}, {status, 1}}};
    return serial_host_call_any(ctx, n, call, [&](HostSlot& sl, size_t cnt, plume_ctx* on) -> int {
        return hd_master_device(on, cnt, sl.in[0].as<uint8_t>(), seed_len, sl.out[0].as<uint8_t>(), sl.out[1].as<uint8_t>(), sl.out[2].as<uint8_t>(), on->stream);
    });
}
static int hd_derive_args_ok(bool pub, int flags, int pk_format, int addr_format, size_t n, const void* parent, const void* parent_chain, const void* path, size_t depth,
                             const void* child_sk, const void* child_pk, const void* status) {
    if (flags & ~(PLUME_HDK_SHARED_PARENT | PLUME_HDK_SHARED_PATH)) return fail(PLUME_ERR_ARG, "unknown flag bits");
    if (pk_format != PLUME_ETHK_PK_AFFINE64 && pk_format != PLUME_ETHK_PK_SEC1) return fail(PLUME_ERR_ARG, "pk_format must be 0 or 1");
    if (addr_format != PLUME_ETHK_ADDR_RAW20 && addr_format != PLUME_ETHK_ADDR_RECORD64 && addr_format != PLUME_ETHK_ADDR_EIP55) return fail(PLUME_ERR_ARG, "addr_format must be 0, 1 or 2");
    if (depth < 1 || depth > PLUME_HDK_MAX_DEPTH) return fail(PLUME_ERR_ARG, "depth must be 1 .. PLUME_HD_MAX_DEPTH");
    if (n && (!parent || !parent_chain || !path || !status || (pub ? !child_pk : !child_sk))) return fail(PLUME_ERR_ARG, "null array");
    if (n > 0xFFFFFFF0u / 64) return fail(PLUME_ERR_ARG, "n too large");
    return 0;
}
static int hd_derive_device(plume_ctx* ctx, bool pub, int flags, int pk_format, int addr_format, size_t n, const uint8_t* parent, const uint8_t* parent_chain,
                            const uint8_t* path, size_t depth, uint8_t* child_sk, uint8_t* child_chain, uint8_t* child_pk, uint8_t* address, uint8_t* status, hipStream_t st) {
    if (n == 0) return 0;
    if (n > ctx->chunk) return fail(PLUME_ERR_ARG, "n exceeds the chunk size (plume_set_chunk)");
    if (int rc = pub ? need_gcomb(ctx) : need_sign_tables(ctx)) return rc;      // built before anything is queued
    if (int rc = ws_acquire(ctx, st)) return rc;
    WsHold hold(ctx, st);
    const std::vector<size_t> cut = sub_batch_bounds(ctx, n);
    const size_t res_bytes = (size_t)PLUME_JAC_WORDS * 4 * n;
    if (ctx->hdws.ensure((size_t)PLUME_HDK_WS_BYTES * n) || ctx->res.ensure(res_bytes) || ctx->resinf.ensure(n)) return PLUME_ERR_HIP;
    struct StageWipe {                                                          // every path out of here, in front of ws_free (~WsHold runs later): k, the chain codes, the images of k G
        plume_ctx* ctx; size_t ws, res; hipStream_t st;
        ~StageWipe() { (void)hipMemsetAsync(ctx->hdws.p, 0, ws, st); (void)hipMemsetAsync(ctx->res.p, 0, res, st); }
    };
    uint8_t* const ws = ctx->hdws.as<uint8_t>();
    const size_t pw = pub ? eth_pk_width(pk_format) : 32, kw = eth_pk_width(pk_format), aw = eth_address_width(addr_format);
    const bool one_parent = (flags & PLUME_HDK_SHARED_PARENT) != 0, one_path = (flags & PLUME_HDK_SHARED_PATH) != 0;
    StageTimer& t = ctx->timer;
    t.begin(st);
    {
        StageWipe wipe{ctx, (size_t)PLUME_HDK_WS_BYTES * n, res_bytes, st};
        for (size_t s = 0; s + 1 < cut.size(); s++) {
            const size_t lo = cut[s], cnt = cut[s + 1] - cut[s];
            HdArgs a;                                                           // the slice [lo, lo + cnt) as a batch of its own
            memset(&a, 0, sizeof a);
            a.flags = flags; a.pk_format = pk_format; a.addr_format = addr_format; a.uniform = ctx->sign_uniform; a.n = (uint32_t)cnt; a.depth = (uint32_t)depth;
            a.parent = parent + (one_parent ? 0 : pw * lo); a.parent_chain = parent_chain + (one_parent ? 0 : 32 * lo); a.path = path + (one_path ? 0 : 4 * depth * lo);
            a.child_sk = child_sk ? child_sk + 32 * lo : nullptr; a.child_chain = child_chain ? child_chain + 32 * lo : nullptr;
            a.child_pk = child_pk ? child_pk + kw * lo : nullptr; a.address = address ? address + aw * lo : nullptr; a.status = status + lo;
            a.k = ws + 32 * lo; a.chain = ws + 32 * n + 32 * lo; a.st = ws + 64 * n + lo;
            a.res = ctx->res.as<uint32_t>() + (size_t)PLUME_JAC_WORDS * lo; a.resinf = ctx->resinf.as<uint8_t>() + lo;
            a.gcomb = ctx->fixed->gcomb.as<uint32_t>(); a.gscan = ctx->fixed->gscan.as<uint32_t>();
            if (pub) {
                launch_hd_pub_load(a, st); t.stage("hd_pub_load", st);
                for (size_t j = 0; j < depth; j++) {
                    a.level = (uint32_t)j;
                    launch_hd_pub_step(a, st); t.stage("hd_pub_step", st);
                    launch_normalize(a.res, a.resinf, cnt, st); t.stage("to_affine", st);
                }
            } else {
                launch_hd_priv_load(a, st); t.stage("hd_priv_load", st);
                for (size_t j = 0; j <= depth; j++) {
                    launch_hd_gmul(a, st); t.stage("hd_gmul", st);
                    launch_normalize(a.res, a.resinf, cnt, st); t.stage("to_affine", st);
                    if (j == depth) break;
                    a.level = (uint32_t)j;
                    launch_hd_priv_step(a, st); t.stage("hd_priv_step", st);
                }
            }
            launch_hd_finish(a, st); t.stage("hd_finish", st);
        }
    }
    HIPCHK(hipGetLastError());
    return hold.release();
}
// pub = false: parent is sk, child_sk is required.  pub = true: parent is pk in pk_format, child_sk is NULL and child_pk required
static int hd_derive_batch_device(plume_ctx* ctx, bool pub, int flags, int pk_format, int addr_format, size_t n, const uint8_t* parent, const uint8_t* parent_chain,
                                  const uint32_t* path, size_t depth, uint8_t* child_sk, uint8_t* child_chain, uint8_t* child_pk, uint8_t* address, uint8_t* status,
                                  void* stream) {
    Route rt_(ctx, stream, n); ctx = rt_.lane; const hipStream_t st_ = rt_.st;
    if (int rc = bind(ctx)) return rc;
    if (int rc = hd_derive_args_ok(pub, flags, pk_format, addr_format, n, parent, parent_chain, path, depth, child_sk, child_pk, status)) return rc;
    return hd_derive_device(ctx, pub, flags, pk_format, addr_format, n, parent, parent_chain, (const uint8_t*)path, depth, pub ? nullptr : child_sk, child_chain, child_pk,
                            address, status, st_);
}
// the host-pointer form: a serial call; sk and the chain codes staged as secrets, going in and coming out; a shared parent or path is a whole-call input
static int hd_derive_batch(plume_ctx* ctx, bool pub, int flags, int pk_format, int addr_format, size_t n, const uint8_t* parent, const uint8_t* parent_chain,
                           const uint32_t* path, size_t depth, uint8_t* child_sk, uint8_t* child_chain, uint8_t* child_pk, uint8_t* address, uint8_t* status) {
    if (!ctx) return fail(PLUME_ERR_ARG, "null context");
    if (int rc = hd_derive_args_ok(pub, flags, pk_format, addr_format, n, parent, parent_chain, path, depth, child_sk, child_pk, status)) return rc;
    if (pub) child_sk = nullptr;
    const bool one_parent = (flags & PLUME_HDK_SHARED_PARENT) != 0, one_path = (flags & PLUME_HDK_SHARED_PATH) != 0;
    const size_t pw = pub ? eth_pk_width(pk_format) : 32;
    const HostCall call{nullptr, nullptr,
                        {{parent, pw, !pub, one_parent}, {parent_chain, 32, true, one_parent}, {path, 4 * depth, false, one_path}},
                        {{child_sk, 32, true}, {child_chain, 32, true}, {child_pk, eth_pk_width(pk_format)}, {address, eth_address_width(addr_format)}, {status, 1}}};
    return serial_host_call_any(ctx, n, call, [&](HostSlot& sl, size_t cnt, plume_ctx* on) -> int {
        return hd_derive_device(on, pub, flags, pk_format, addr_format, cnt, sl.in[0].as<uint8_t>(), sl.in[1].as<uint8_t>(), sl.in[2].as<uint8_t>(), depth,
                                child_sk ? sl.out[0].as<uint8_t>() : nullptr, child_chain ? sl.out[1].as<uint8_t>() : nullptr, child_pk ? sl.out[2].as<uint8_t>() : nullptr,
                                address ? sl.out[3].as<uint8_t>() : nullptr, sl.out[4].as<uint8_t>(), on->stream);
    });
}
extern "C" int plume_hd_derive_priv_batch(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* parent_sk, const uint8_t* parent_chain,
                                          const uint32_t* path, size_t depth, uint8_t* child_sk, uint8_t* child_chain, uint8_t* child_pk, uint8_t* address, uint8_t* status) {
    return hd_derive_batch(ctx, false, flags, pk_format, addr_format, n, parent_sk, parent_chain, path, depth, child_sk, child_chain, child_pk, address, status);
}
extern "C" int plume_hd_derive_priv_batch_device(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* parent_sk, const uint8_t* parent_chain,
                                                 const uint32_t* path, size_t depth, uint8_t* child_sk, uint8_t* child_chain, uint8_t* child_pk, uint8_t* address,
                                                 uint8_t* status, void* stream) {
    return hd_derive_batch_device(ctx, false, flags, pk_format, addr_format, n, parent_sk, parent_chain, path, depth, child_sk, child_chain, child_pk, address, status, stream);
}
extern "C" int plume_hd_derive_pub_batch(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* parent_pk, const uint8_t* parent_chain,
                                         const uint32_t* path, size_t depth, uint8_t* child_pk, uint8_t* child_chain, uint8_t* address, uint8_t* status) {
    return hd_derive_batch(ctx, true, flags, pk_format, addr_format, n, parent_pk, parent_chain, path, depth, nullptr, child_chain, child_pk, address, status);
}
extern "C" int plume_hd_derive_pub_batch_device(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* parent_pk, const uint8_t* parent_chain,
                                                const uint32_t* path, size_t depth, uint8_t* child_pk, uint8_t* child_chain, uint8_t* address, uint8_t* status, void* stream) {
    return hd_derive_batch_device(ctx, true, flags, pk_format, addr_format, n, parent_pk, parent_chain, path, depth, nullptr, child_chain, child_pk, address, status, stream);
}
