// The transaction signer (include/plume_hip.h, plume_eth_tx_sign_batch*): its C ABI and its host side.  k_eth_tx_sign_frame stages the framing and the signing hash in
// ctx->txsign, the ECDSA signer's stages (ecdsa_sign_device of plume_ecdsa_sign_capi.hip, on this workspace and this stream, self-check included) sign the staged hash into
// the same staging -- tables, sub-batches, the uniform level and the chunk limit are theirs --, k_eth_tx_sign_assemble writes the caller's slots and records; the staged r, s,
// v and status are wiped behind it (an item the framing rejected was signed over the zero hash: that signature is never released).  The call holds the workspace from in
// front of the frame to behind the wipe.  The host-pointer form is a serial call (serial_host_call_any): the transactions staged as messages, sk and aux as secrets, `out` as
// the call's ragged output -- one contiguous download per piece.
#include <cstring>

#include "../../include/plume_hip.h"
#include "plume_capi_ctx.h"
#include "plume_eth_tx_sign_launch.h"

using namespace plume;

static_assert(PLUME_ETH_TX_SIGN_GROWTH == PLUME_ETHTXK_SIGN_GROWTH && PLUME_STATUS_BAD_TX == PLUME_ST_BAD_TX, "the header and the kernels state the same constants");

extern "C" size_t plume_eth_tx_sign_out_bytes(size_t n, uint64_t txs_bytes) { return (size_t)txs_bytes + (size_t)PLUME_ETH_TX_SIGN_GROWTH * n; }

static int eth_tx_sign_args_ok(int flags, size_t n, const void* off, const void* sk, const void* out, const void* out_len, const void* status) {
    if (flags) return fail(PLUME_ERR_ARG, "unknown flag bits");
    if (n && (!off || !sk || !out || !out_len || !status)) return fail(PLUME_ERR_ARG, "null array");
    if (n > 0xFFFFFFF0u) return fail(PLUME_ERR_ARG, "n too large");
    const uint8_t one = 0;                                                      // (hash, r, s, v are the staging's: any non-null pointer passes the signer's own check)
    return ecdsa_sign_args_ok(0, n, &one, sk ? sk : &one, &one, &one, &one, &one);
}
static int eth_tx_sign_device(plume_ctx* ctx, size_t n, const uint8_t* txs, const uint64_t* tx_off, size_t txs_bytes, const uint8_t* sk, const uint8_t* aux, uint8_t* out,
                              size_t out_bytes, uint32_t* out_len, uint8_t* hash, uint8_t* r, uint8_t* s, uint8_t* v, uint64_t* chain_id, uint8_t* tx_type, uint8_t* status,
                              hipStream_t st) {
    if (n == 0) return 0;
    if (n > ctx->chunk) return fail(PLUME_ERR_ARG, "n exceeds the chunk size (plume_set_chunk)");
    if (!txs && txs_bytes) return fail(PLUME_ERR_ARG, "null transaction buffer");
    if (int rc = need_sign_tables(ctx)) return rc;                              // the signer's tables, built before anything is queued
    if (ctx->sign_selfcheck) { if (int rc = need_gcomb(ctx)) return rc; }
    if (int rc = ws_acquire(ctx, st)) return rc;
    WsHold hold(ctx, st);
    if (ctx->txsign.ensure((size_t)PLUME_ETHTXK_SIGN_STAGE * n)) return PLUME_ERR_HIP;
    uint8_t* const stg = ctx->txsign.as<uint8_t>();
    uint8_t *const g_hash = stg + 16 * n, *const g_r = stg + 48 * n, *const g_s = stg + 80 * n, *const g_v = stg + 112 * n, *const g_status = stg + 113 * n;
    struct StageWipe {                                                          // failure paths only: whatever fails behind the sign stages, the staged signatures do not linger (queued in front of ws_free: ~WsHold runs later)
        uint8_t* p; size_t bytes; hipStream_t st;
        ~StageWipe() { if (bytes) (void)hipMemsetAsync(p, 0, bytes, st); }
    } stage_wipe{g_r, 66 * n, st};
    EthTxSignArgs a;
    memset(&a, 0, sizeof a);
    a.n = (uint32_t)n; a.txs = txs; a.tx_off = tx_off; a.txs_bytes = txs ? txs_bytes : 0;
    a.st_chain = (uint64_t*)stg; a.st_frame = (uint64_t*)(stg + 8 * n); a.st_hash = g_hash; a.st_r = g_r; a.st_s = g_s; a.st_v = g_v; a.st_status = g_status;
    a.out = out; a.out_bytes = out_bytes; a.out_len = out_len; a.hash = hash; a.r = r; a.s = s; a.v = v; a.chain_id = chain_id; a.tx_type = tx_type; a.status = status;
    ctx->timer.begin(st);
    launch_eth_tx_sign_frame(a, st); ctx->timer.stage("eth_tx_sign_frame", st);
    HIPCHK(hipGetLastError());
    if (int rc = ecdsa_sign_device(ctx, 0, n, g_hash, sk, aux, g_r, g_s, g_v, g_status, st, true)) return rc;
    launch_eth_tx_sign_assemble(a, st); ctx->timer.stage("eth_tx_sign_assemble", st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(g_r, 0, 66 * n, st));                                  // r, s, v, status: contiguous in the staging
    stage_wipe.bytes = 0;
    return hold.release();
}
extern "C" int plume_eth_tx_sign_batch_device(plume_ctx* ctx, int flags, size_t n, const uint8_t* txs, const uint64_t* tx_off, size_t txs_bytes, const uint8_t* sk,
                                              const uint8_t* aux, uint8_t* out, size_t out_bytes, uint32_t* out_len, uint8_t* hash32, uint8_t* r, uint8_t* s, uint8_t* v,
                                              uint64_t* chain_id, uint8_t* tx_type, uint8_t* status, void* stream) {
    Route rt_(ctx, stream, n); ctx = rt_.lane; const hipStream_t st_ = rt_.st;
    if (int rc = bind(ctx)) return rc;
    if (int rc = eth_tx_sign_args_ok(flags, n, tx_off, sk, out, out_len, status)) return rc;
    return eth_tx_sign_device(ctx, n, txs, tx_off, txs_bytes, sk, aux, out, out_bytes, out_len, hash32, r, s, v, chain_id, tx_type, status, st_);
}
// the host-pointer form: a serial call with the transactions as its messages, sk and aux staged as secrets, and `out` as the call's ragged output
extern "C" int plume_eth_tx_sign_batch(plume_ctx* ctx, int flags, size_t n, const uint8_t* txs, const uint64_t* tx_off, const uint8_t* sk, const uint8_t* aux, uint8_t* out,
                                       uint32_t* out_len, uint8_t* hash32, uint8_t* r, uint8_t* s, uint8_t* v, uint64_t* chain_id, uint8_t* tx_type, uint8_t* status) {
    if (!ctx) return fail(PLUME_ERR_ARG, "null context");
    if (int rc = eth_tx_sign_args_ok(flags, n, tx_off, sk, out, out_len, status)) return rc;
    HostCall call = eth_tx_call({txs, tx_off, {{sk, 32, true}, {aux, 32, true}},
                                 {{out_len, 4}, {status, 1}, {hash32, 32}, {r, 32}, {s, 32}, {v, 1}, {chain_id, 8}, {tx_type, 1}}});
    call.ragged = out; call.ragged_growth = PLUME_ETHTXK_SIGN_GROWTH;
    return serial_host_call_any(ctx, n, call, [&](HostSlot& sl, size_t cnt, plume_ctx* on) -> int {
        const size_t out_bytes = (size_t)sl.rel[cnt] + (size_t)PLUME_ETHTXK_SIGN_GROWTH * cnt;
        return eth_tx_sign_device(on, cnt, sl.msgs.as<uint8_t>(), sl.off.as<uint64_t>(), (size_t)sl.rel[cnt], sl.in[0].as<uint8_t>(), aux ? sl.in[1].as<uint8_t>() : nullptr,
                                  sl.ragged.as<uint8_t>(), out_bytes, sl.out[0].as<uint32_t>(), hash32 ? sl.out[2].as<uint8_t>() : nullptr,
                                  r ? sl.out[3].as<uint8_t>() : nullptr, s ? sl.out[4].as<uint8_t>() : nullptr, v ? sl.out[5].as<uint8_t>() : nullptr,
                                  chain_id ? sl.out[6].as<uint64_t>() : nullptr, tx_type ? sl.out[7].as<uint8_t>() : nullptr, sl.out[1].as<uint8_t>(), on->stream);
    });
}
