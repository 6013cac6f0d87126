// The ECDSA recovery (include/plume_hip.h, plume_ecdsa_recover_batch*): its C ABI and its host side -- prepare, the table stage, the multiplication and its redo launch, the
// conversion to affine, finalize; the table stage and the conversion are plume_capi.hip's.  The comb of G is the only fixed table (never the 1 GiB window table); the
// workspace is the verifier's own buffers, one table job per item, so the device form joins the ws_free chain.  plume_set_sub_batches cuts the call as it cuts a verify
// call (sub_batch_bounds); the slices follow one another on the caller's stream.  The device form does not synchronise; the host-pointer form goes through
// serial_host_call_any, as plume_eth_address_batch does.  ecdsa_args_ok and ecdsa_device are lent to the transaction sender and to the ECDSA signer's self-check
// (plume_capi_ctx.h).
#include <algorithm>
#include <cstring>
#include <memory>

#include "../../include/plume_hip.h"
#include "plume_capi_ctx.h"
#include "plume_ecdsa_launch.h"

using namespace plume;

int plume::ecdsa_args_ok(int flags, int pk_format, int addr_format, size_t n, const void* hash, const void* r, const void* s, const void* v, const void* pk, const void* address,
                         const void* status) {
    if (flags & ~PLUME_ECDSAK_LOW_S) return fail(PLUME_ERR_ARG, "unknown flag bits");
    if (pk_format != PLUME_ETHK_PK_AFFINE64 && pk_format != PLUME_ETHK_PK_SEC1) return fail(PLUME_ERR_ARG, "pk_format must be 0 or 1");
    if (addr_format != PLUME_ETHK_ADDR_RAW20 && addr_format != PLUME_ETHK_ADDR_RECORD64 && addr_format != PLUME_ETHK_ADDR_EIP55) return fail(PLUME_ERR_ARG, "addr_format must be 0, 1 or 2");
    if (n && (!hash || !r || !s || !v)) return fail(PLUME_ERR_ARG, "null array");
    if (n && !pk && !address && !status) return fail(PLUME_ERR_ARG, "no output array");
    if (n > 0xFFFFFFF0u) return fail(PLUME_ERR_ARG, "n too large");
    return 0;
}
int plume::ecdsa_device(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* hash, const uint8_t* r, const uint8_t* s, const uint8_t* v,
                        const uint8_t* expect, uint8_t* pk, uint8_t* address, uint8_t* status, hipStream_t st, bool continue_timer) {
    if (n == 0) return 0;
    if (n > ctx->chunk) return fail(PLUME_ERR_ARG, "n exceeds the chunk size (plume_set_chunk)");
    if (int rc = need_gcomb(ctx)) return rc;
    if (!continue_timer) { if (int rc = ws_acquire(ctx, st)) return rc; }     // continue_timer: the caller (the ECDSA signer's self-check) holds the workspace already
    std::unique_ptr<WsHold> hold(continue_timer ? nullptr : new WsHold(ctx, st));
    const std::vector<size_t> cut = sub_batch_bounds(ctx, n);
    const size_t nsub = cut.size() - 1;
    size_t scr_bytes = 0;
    for (size_t k = 0; k < nsub; k++) scr_bytes = std::max(scr_bytes, table_stage_scratch(ctx, cut[k + 1] - cut[k], 0));
    if (ctx->bases.ensure((size_t)PLUME_BASE_WORDS * 4 * n) || ctx->jobflags.ensure(n) || ctx->itemflags.ensure(n) || ctx->tab.ensure((size_t)PLUME_TAB_WORDS * 4 * n) ||
        ctx->tabscr.ensure(scr_bytes) || ctx->res.ensure((size_t)PLUME_JAC_WORDS * 4 * n) || ctx->resinf.ensure(n) || ctx->redo.ensure((n + nsub) * 4) ||
        ctx->digs.ensure((size_t)PLUME_NPOS * n) || ctx->eq1k.ensure(32 * n))
        return PLUME_ERR_HIP;
    ctx->redo_foreign = true;                                                 // the verifier's redo counters are no longer where plume_last_redo_tasks would read them
    const size_t P = eth_pk_width(pk_format), W = eth_address_width(addr_format);
    StageTimer& t = ctx->timer;
    if (!continue_timer) t.begin(st);
    for (size_t k = 0; k < nsub; k++) {
        const size_t lo = cut[k], cnt = cut[k + 1] - cut[k];
        EcdsaArgs a;                                                          // the slice [lo, lo + cnt) as a batch of its own: every array and every scratch region starts at the slice
        memset(&a, 0, sizeof a);
        a.flags = flags; a.pk_format = pk_format; a.addr_format = addr_format; a.n = (uint32_t)cnt;
        a.hash = hash + 32 * lo; a.r = r + 32 * lo; a.s = s + 32 * lo; a.v = v + lo; a.expect = expect ? expect + 20 * lo : nullptr;
        a.pk = pk ? pk + P * lo : nullptr; a.address = address ? address + W * lo : nullptr; a.status = status ? status + lo : nullptr;
        a.bases = ctx->bases.as<uint32_t>() + (size_t)PLUME_BASE_WORDS * lo; a.jobflags = ctx->jobflags.as<uint8_t>() + lo; a.itemflags = ctx->itemflags.as<uint8_t>() + lo;
        a.tab = ctx->tab.as<uint32_t>() + (size_t)PLUME_TAB_WORDS * lo; a.digs = ctx->digs.as<int8_t>() + (size_t)PLUME_NPOS * lo; a.u1 = ctx->eq1k.as<uint32_t>() + 8 * lo;
        a.res = ctx->res.as<uint32_t>() + (size_t)PLUME_JAC_WORDS * lo; a.resinf = ctx->resinf.as<uint8_t>() + lo;
        a.redo = ctx->redo.as<uint32_t>() + lo + k;                          // the slice's redo list: counter + up to cnt items
        a.gcomb = ctx->fixed->gcomb.as<uint32_t>();
        launch_ecdsa_prepare(a, st); t.stage("ecdsa_prepare", st);
        table_stage(ctx, a.tab, a.bases, a.jobflags, cnt, 0, st); t.stage("tables", st);
        launch_ecdsa_mul(a, st); t.stage("ecdsa_mul", st);
        launch_normalize(a.res, a.resinf, cnt, st); t.stage("to_affine", st);
        launch_ecdsa_finalize(a, st); t.stage("ecdsa_finalize", st);
    }
    HIPCHK(hipGetLastError());
    return hold ? hold->release() : 0;
}
extern "C" int plume_ecdsa_recover_batch_device(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* hash, const uint8_t* r, const uint8_t* s,
                                                const uint8_t* v, const uint8_t* expect, uint8_t* pk, uint8_t* address, uint8_t* status, void* stream) {
    Route rt_(ctx, stream, n); ctx = rt_.lane; const hipStream_t st_ = rt_.st;
    if (int rc = bind(ctx)) return rc;
    if (int rc = ecdsa_args_ok(flags, pk_format, addr_format, n, hash, r, s, v, pk, address, status)) return rc;
    return ecdsa_device(ctx, flags, pk_format, addr_format, n, hash, r, s, v, expect, pk, address, status, st_);
}
extern "C" int plume_ecdsa_recover_batch(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* hash, const uint8_t* r, const uint8_t* s,
                                         const uint8_t* v, const uint8_t* expect, uint8_t* pk, uint8_t* address, uint8_t* status) {
    if (!ctx) return fail(PLUME_ERR_ARG, "null context");
    if (int rc = ecdsa_args_ok(flags, pk_format, addr_format, n, hash, r, s, v, pk, address, status)) return rc;
    const HostCall call{nullptr, nullptr, {{hash, 32}, {r, 32}, {s, 32}, {v, 1}, {expect, 20}}, {{pk, eth_pk_width(pk_format)}, {address, eth_address_width(addr_format)}, {status, 1}}};
    return serial_host_call_any(ctx, n, call, [&](HostSlot& sl, size_t cnt, plume_ctx* on) -> int {
        return ecdsa_device(on, flags, pk_format, addr_format, cnt, sl.in[0].as<uint8_t>(), sl.in[1].as<uint8_t>(), sl.in[2].as<uint8_t>(), sl.in[3].as<uint8_t>(),
                            expect ? sl.in[4].as<uint8_t>() : nullptr, pk ? sl.out[0].as<uint8_t>() : nullptr, address ? sl.out[1].as<uint8_t>() : nullptr,
                            status ? sl.out[2].as<uint8_t>() : nullptr, on->stream);
    });
}
