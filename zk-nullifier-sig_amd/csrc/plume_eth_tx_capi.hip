// The transaction calls (include/plume_hip.h, plume_eth_tx_parse_batch*, plume_eth_tx_sender_batch*): their C ABI and their host side.  parse is the message-hash call with
// more outputs: one kernel on the caller's arrays, no table, no workspace, through serial_host_call_any.  sender runs the same kernel into ctx->txstage (hash, r, s, v: 97 B /
// item) and the recover stages (ecdsa_device of plume_ecdsa_capi.hip, on this workspace and this stream) on what it staged, so it holds the workspace from in front of the
// parse to behind finalize; sub-batches, chunk limit and routing are those of plume_ecdsa_recover_batch*.
#include "../../include/plume_hip.h"
#include "plume_capi_ctx.h"
#include "plume_eth_tx_launch.h"

using namespace plume;

static int eth_tx_parse_args_ok(size_t n, const void* off, const void* hash, const void* r, const void* s, const void* v) {
    if (n && (!off || !hash || !r || !s || !v)) return fail(PLUME_ERR_ARG, "null array");
    if (n > 0xFFFFFFF0u) return fail(PLUME_ERR_ARG, "n too large");
    return 0;
}
static EthTxArgs eth_tx_args(size_t n, const uint8_t* txs, const uint64_t* tx_off, size_t txs_bytes, uint8_t* hash, uint8_t* r, uint8_t* s, uint8_t* v, uint64_t* chain_id,
                             uint8_t* tx_type, uint8_t* status) {
    EthTxArgs a; a.n = (uint32_t)n; a.txs = txs; a.tx_off = tx_off; a.txs_bytes = txs ? txs_bytes : 0; a.hash = hash; a.r = r; a.s = s; a.v = v; a.chain_id = chain_id;
    a.tx_type = tx_type; a.status = status;
    return a;
}
static int eth_tx_parse_device(plume_ctx* ctx, size_t n, const uint8_t* txs, const uint64_t* tx_off, size_t txs_bytes, uint8_t* hash, uint8_t* r, uint8_t* s, uint8_t* v,
                               uint64_t* chain_id, uint8_t* tx_type, uint8_t* status, hipStream_t st) {
    if (n == 0) return 0;
    if (!txs && txs_bytes) return fail(PLUME_ERR_ARG, "null transaction buffer");
    ctx->timer.begin(st);
    launch_eth_tx_parse(eth_tx_args(n, txs, tx_off, txs_bytes, hash, r, s, v, chain_id, tx_type, status), st); ctx->timer.stage("eth_tx_parse", st);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int plume_eth_tx_parse_batch_device(plume_ctx* ctx, size_t n, const uint8_t* txs, const uint64_t* tx_off, size_t txs_bytes, uint8_t* hash32, uint8_t* r,
                                               uint8_t* s, uint8_t* v, uint64_t* chain_id, uint8_t* tx_type, uint8_t* status, void* stream) {
    Route rt_(ctx, stream); ctx = rt_.lane; const hipStream_t st_ = rt_.st;
    if (int rc = bind(ctx)) return rc;
    if (int rc = eth_tx_parse_args_ok(n, tx_off, hash32, r, s, v)) return rc;
    return eth_tx_parse_device(ctx, n, txs, tx_off, txs_bytes, hash32, r, s, v, chain_id, tx_type, status, st_);
}
extern "C" int plume_eth_tx_parse_batch(plume_ctx* ctx, size_t n, const uint8_t* txs, const uint64_t* tx_off, uint8_t* hash32, uint8_t* r, uint8_t* s, uint8_t* v,
                                        uint64_t* chain_id, uint8_t* tx_type, uint8_t* status) {
    if (!ctx) return fail(PLUME_ERR_ARG, "null context");
    if (int rc = eth_tx_parse_args_ok(n, tx_off, hash32, r, s, v)) return rc;
    const HostCall call = eth_tx_call({txs, tx_off, {}, {{hash32, 32}, {r, 32}, {s, 32}, {v, 1}, {chain_id, 8}, {tx_type, 1}, {status, 1}}});
    return serial_host_call_any(ctx, n, call, [&](HostSlot& sl, size_t cnt, plume_ctx* on) -> int {
        return eth_tx_parse_device(on, cnt, sl.msgs.as<uint8_t>(), sl.off.as<uint64_t>(), (size_t)sl.rel[cnt], sl.out[0].as<uint8_t>(), sl.out[1].as<uint8_t>(), sl.out[2].as<uint8_t>(),
                                   sl.out[3].as<uint8_t>(), chain_id ? sl.out[4].as<uint64_t>() : nullptr, tx_type ? sl.out[5].as<uint8_t>() : nullptr,
                                   status ? sl.out[6].as<uint8_t>() : nullptr, on->stream);
    });
}
static int eth_tx_sender_args_ok(int flags, int pk_format, int addr_format, size_t n, const void* off, const void* pk, const void* address, const void* status) {
    if (n && !off) return fail(PLUME_ERR_ARG, "null array");
    const uint8_t one = 0;                                                      // (hash, r, s, v are the staging's: any non-null pointer passes the recovery's own check)
    return ecdsa_args_ok(flags, pk_format, addr_format, n, &one, &one, &one, &one, pk, address, status);
}
static int eth_tx_sender_device(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* txs, const uint64_t* tx_off, size_t txs_bytes,
                                const uint8_t* expect, uint8_t* pk, uint8_t* address, uint64_t* chain_id, uint8_t* tx_type, uint8_t* status, hipStream_t st) {
    if (n == 0) return 0;
    if (n > ctx->chunk) return fail(PLUME_ERR_ARG, "n exceeds the chunk size (plume_set_chunk)");
    if (!txs && txs_bytes) return fail(PLUME_ERR_ARG, "null transaction buffer");
    if (int rc = need_gcomb(ctx)) return rc;                                    // the recover stages' table, built before anything is queued
    if (int rc = ws_acquire(ctx, st)) return rc;
    WsHold hold(ctx, st);
    if (ctx->txstage.ensure(97 * n)) return PLUME_ERR_HIP;
    uint8_t* const stg = ctx->txstage.as<uint8_t>();
    uint8_t *const g_hash = stg, *const g_r = stg + 32 * n, *const g_s = stg + 64 * n, *const g_v = stg + 96 * n;
    ctx->timer.begin(st);
    launch_eth_tx_parse(eth_tx_args(n, txs, tx_off, txs_bytes, g_hash, g_r, g_s, g_v, chain_id, tx_type, nullptr), st); ctx->timer.stage("eth_tx_parse", st);
    HIPCHK(hipGetLastError());
    if (int rc = ecdsa_device(ctx, flags, pk_format, addr_format, n, g_hash, g_r, g_s, g_v, expect, pk, address, status, st, true)) return rc;
    return hold.release();
}
extern "C" int plume_eth_tx_sender_batch_device(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* txs, const uint64_t* tx_off,
                                                size_t txs_bytes, const uint8_t* expect, uint8_t* pk, uint8_t* address, uint64_t* chain_id, uint8_t* tx_type, uint8_t* status,
                                                void* stream) {
    Route rt_(ctx, stream, n); ctx = rt_.lane; const hipStream_t st_ = rt_.st;
    if (int rc = bind(ctx)) return rc;
    if (int rc = eth_tx_sender_args_ok(flags, pk_format, addr_format, n, tx_off, pk, address, status)) return rc;
    return eth_tx_sender_device(ctx, flags, pk_format, addr_format, n, txs, tx_off, txs_bytes, expect, pk, address, chain_id, tx_type, status, st_);
}
extern "C" int plume_eth_tx_sender_batch(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* txs, const uint64_t* tx_off,
                                         const uint8_t* expect, uint8_t* pk, uint8_t* address, uint64_t* chain_id, uint8_t* tx_type, uint8_t* status) {
    if (!ctx) return fail(PLUME_ERR_ARG, "null context");
    if (int rc = eth_tx_sender_args_ok(flags, pk_format, addr_format, n, tx_off, pk, address, status)) return rc;
    const HostCall call = eth_tx_call({txs, tx_off, {{expect, 20}},
                                       {{pk, eth_pk_width(pk_format)}, {address, eth_address_width(addr_format)}, {status, 1}, {chain_id, 8}, {tx_type, 1}}});
    return serial_host_call_any(ctx, n, call, [&](HostSlot& sl, size_t cnt, plume_ctx* on) -> int {
        return eth_tx_sender_device(on, flags, pk_format, addr_format, cnt, sl.msgs.as<uint8_t>(), sl.off.as<uint64_t>(), (size_t)sl.rel[cnt], expect ? sl.in[0].as<uint8_t>() : nullptr,
                                    pk ? sl.out[0].as<uint8_t>() : nullptr, address ? sl.out[1].as<uint8_t>() : nullptr, chain_id ? sl.out[3].as<uint64_t>() : nullptr,
                                    tx_type ? sl.out[4].as<uint8_t>() : nullptr, status ? sl.out[2].as<uint8_t>() : nullptr, on->stream);
    });
}
