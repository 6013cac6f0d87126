// The ECDSA signer (include/plume_hip.h, plume_ecdsa_sign_batch*): its C ABI and its host side -- nonce, the comb, the conversion to affine (plume_capi.hip's), finalize.
// The table of G is the signer's -- the comb, or at level 2 the scanned table, never the verifier's window table -- and the workspace is the signer's too: the nonce buffer,
// one Jacobian result per item (two with the self-check: sk G), the item flags; the call joins the ws_free chain.  plume_set_sub_batches cuts the call as it cuts an ECDSA
// recovery (sub_batch_bounds); there is no stage in front of a long multiplication to overlap, so the slices follow one another on the caller's stream.  With
// plume_set_sign_selfcheck on, finalize writes ctx->scstage, the recover stages (ecdsa_device of plume_ecdsa_capi.hip, on this workspace and this stream) recover a key from
// the staged (hash, r, s, v), the release kernel writes the caller's arrays and the staging is wiped.  The chunk limit, the in-flight lanes, the host pipeline (sk and aux
// staged and wiped) and sharding are those of plume_sign_batch_rfc6979*.  ecdsa_sign_args_ok and ecdsa_sign_device are lent to the transaction signer (plume_capi_ctx.h).
#include <cstring>
#include <memory>

#include "../../include/plume_hip.h"
#include "plume_capi_ctx.h"
#include "plume_ecdsa_sign_launch.h"

using namespace plume;

int plume::ecdsa_sign_args_ok(int flags, size_t n, const void* hash, const void* sk, const void* r, const void* s, const void* v, const void* status) {
    if (flags & ~PLUME_ECDSAK_SIGN_V27) return fail(PLUME_ERR_ARG, "unknown flag bits");
    if (n && (!hash || !sk || !r || !s || !v || !status)) return fail(PLUME_ERR_ARG, "null array");
    if (n > 0xFFFFFFF0u) return fail(PLUME_ERR_ARG, "n too large");
    return 0;
}
int plume::ecdsa_sign_device(plume_ctx* ctx, int flags, size_t n, const uint8_t* hash, const uint8_t* sk, const uint8_t* aux, uint8_t* r, uint8_t* s, uint8_t* v, uint8_t* status,
                             hipStream_t st, bool continue_timer) {
    if (n == 0) return 0;
    if (n > ctx->chunk) return fail(PLUME_ERR_ARG, "n exceeds the chunk size (plume_set_chunk)");
    if (int rc = need_sign_tables(ctx)) return rc;
    const bool selfcheck = ctx->sign_selfcheck != 0;
    if (selfcheck) { if (int rc = need_gcomb(ctx)) return rc; }                  // the recover stages' table, built before anything is queued
    if (!continue_timer) { if (int rc = ws_acquire(ctx, st)) return rc; }       // continue_timer: the caller (the transaction signer) holds the workspace already and has begun the timeline
    std::unique_ptr<WsHold> hold(continue_timer ? nullptr : new WsHold(ctx, st));
    const std::vector<size_t> cut = sub_batch_bounds(ctx, n);
    const size_t nsub = cut.size() - 1;
    const size_t T = selfcheck ? 2 : 1;                                         // points per item
    constexpr size_t kEcdsaStageBytes = 2 * 32 + 2 * 64 + 3;                         // per item: r, s | sk G, the recovered key | v, status, the recover stages' status -- in that order, the records 16-byte aligned
    if (ctx->nonce.ensure(32 * n) || ctx->itemflags.ensure(n) || ctx->res.ensure((size_t)PLUME_JAC_WORDS * 4 * T * n) || ctx->resinf.ensure(T * n) ||
        (selfcheck && ctx->scstage.ensure(kEcdsaStageBytes * n)))
        return PLUME_ERR_HIP;
    uint8_t* const stg = ctx->scstage.as<uint8_t>();
    uint8_t *const g_r = stg, *const g_s = stg + 32 * n, *const g_pk = stg + 64 * n, *const g_rec = stg + 128 * n, *const g_v = stg + 192 * n, *const g_status = stg + 193 * n,
            *const g_recst = stg + 194 * n;
    struct StageWipe {                                                          // failure paths only: a call that fails behind finalize still wipes what it staged, in front of ws_free (~WsHold)
        plume_ctx* ctx; size_t bytes; hipStream_t st;
        ~StageWipe() { if (bytes) (void)hipMemsetAsync(ctx->scstage.p, 0, bytes, st); }
    } stage_wipe{ctx, selfcheck ? kEcdsaStageBytes * n : 0, st};
    StageTimer& t = ctx->timer;
    if (!continue_timer) t.begin(st);
    for (size_t k = 0; k < nsub; k++) {
        const size_t lo = cut[k], cnt = cut[k + 1] - cut[k];
        EcdsaSignArgs a;                                                        // the slice [lo, lo + cnt) as a batch of its own
        memset(&a, 0, sizeof a);
        a.flags = flags; a.uniform = ctx->sign_uniform; a.n = (uint32_t)cnt; a.ntask = (uint32_t)T;
        a.hash = hash + 32 * lo; a.sk = sk + 32 * lo; a.aux = aux ? aux + 32 * lo : nullptr;
        a.r = (selfcheck ? g_r : r) + 32 * lo; a.s = (selfcheck ? g_s : s) + 32 * lo; a.v = (selfcheck ? g_v : v) + lo; a.status = (selfcheck ? g_status : status) + lo;
        a.pkstage = selfcheck ? g_pk + 64 * lo : nullptr;
        a.k = ctx->nonce.as<uint8_t>() + 32 * lo; a.itemflags = ctx->itemflags.as<uint8_t>() + lo;
        a.res = ctx->res.as<uint32_t>() + (size_t)PLUME_JAC_WORDS * T * lo; a.resinf = ctx->resinf.as<uint8_t>() + T * lo;
        a.gcomb = ctx->fixed->gcomb.as<uint32_t>(); a.gscan = ctx->fixed->gscan.as<uint32_t>();
        launch_ecdsa_sign_nonce(a, st); t.stage("ecdsa_sign_nonce", st);
        launch_ecdsa_sign_gmul(a, st); t.stage("ecdsa_sign_gmul", st);
        launch_normalize(a.res, a.resinf, T * cnt, st); t.stage("to_affine", st);
        launch_ecdsa_sign_finalize(a, st); t.stage("ecdsa_sign_finalize", st);
    }
    // the nonces never leave the device; wipe them and the images of k G behind the last kernel that reads them
    HIPCHK(hipMemsetAsync(ctx->nonce.p, 0, 32 * n, st));
    HIPCHK(hipMemsetAsync(ctx->res.p, 0, (size_t)PLUME_JAC_WORDS * 4 * T * n, st));
    HIPCHK(hipGetLastError());
    if (selfcheck) {
        if (int rc = ecdsa_device(ctx, PLUME_ECDSAK_LOW_S, PLUME_ETHK_PK_AFFINE64, PLUME_ETHK_ADDR_RAW20, n, hash, g_r, g_s, g_v, nullptr, g_rec, nullptr, g_recst, st, true))
            return rc;
        EcdsaSignReleaseArgs ra;
        ra.n = (uint32_t)n; ra.stage_r = g_r; ra.stage_s = g_s; ra.stage_v = g_v; ra.stage_status = g_status; ra.stage_pk = g_pk; ra.rec_pk = g_rec; ra.rec_status = g_recst;
        ra.r = r; ra.s = s; ra.v = v; ra.status = status;
        launch_ecdsa_sign_release(ra, st); t.stage("ecdsa_sign_release", st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemsetAsync(ctx->scstage.p, 0, kEcdsaStageBytes * n, st));        // a withheld s is precisely the value that must not linger
        stage_wipe.bytes = 0;
    }
    return hold ? hold->release() : 0;
}
extern "C" int plume_ecdsa_sign_batch_device(plume_ctx* ctx, int flags, size_t n, const uint8_t* hash, const uint8_t* sk, const uint8_t* aux, uint8_t* r, uint8_t* s,
                                             uint8_t* v, uint8_t* status, void* stream) {
    Route rt_(ctx, stream, n); ctx = rt_.lane; const hipStream_t st_ = rt_.st;
    if (int rc = bind(ctx)) return rc;
    if (int rc = ecdsa_sign_args_ok(flags, n, hash, sk, r, s, v, status)) return rc;
    return ecdsa_sign_device(ctx, flags, n, hash, sk, aux, r, s, v, status, st_);
}
// the host-pointer form: the signer's pipeline (host_call_any: pieces, two lanes, shards; sk and aux staged as secrets and wiped), with no messages to stage
extern "C" int plume_ecdsa_sign_batch(plume_ctx* ctx, int flags, size_t n, const uint8_t* hash, const uint8_t* sk, const uint8_t* aux, uint8_t* r, uint8_t* s, uint8_t* v,
                                      uint8_t* status) {
    if (!ctx) return fail(PLUME_ERR_ARG, "null context");
    if (int rc = ecdsa_sign_args_ok(flags, n, hash, sk, r, s, v, status)) return rc;
    if (n == 0) return 0;
    static const uint8_t no_msgs[16] = {0};
    const std::vector<uint64_t> no_off(n + 1, 0);                               // every item's message is empty
    const HostCall call{no_msgs, no_off.data(), {{hash, 32}, {sk, 32, true}, {aux, 32, true}}, {{r, 32}, {s, 32}, {v, 1}, {status, 1}}, false, ctx->host_sign_lanes > 1};
    return host_call_any(ctx, n, call, [&](HostSlot& sl, size_t cnt, plume_ctx* on) -> int {
        return ecdsa_sign_device(on, flags, cnt, sl.in[0].as<uint8_t>(), sl.in[1].as<uint8_t>(), aux ? sl.in[2].as<uint8_t>() : nullptr, sl.out[0].as<uint8_t>(),
                                 sl.out[1].as<uint8_t>(), sl.out[2].as<uint8_t>(), sl.out[3].as<uint8_t>(), on->stream);
    });
}
