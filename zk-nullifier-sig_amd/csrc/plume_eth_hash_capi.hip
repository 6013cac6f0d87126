// The message-hash call (include/plume_hip.h, plume_eth_message_hash_batch*): its C ABI and its host side; the launcher is declared beside the address kernel's.  Like the
// address call it needs no table and touches no workspace.  The host-pointer form goes through serial_host_call_any with the messages in its table (every chunk's bytes and
// its offsets, rebased to the chunk, are staged by stage_msgs; msgs may be null when it holds no bytes); the device form enqueues on the caller's stream and does not
// synchronise.  Kept apart from plume_eth_capi.hip so that the harness of the address call links with the one launcher it stands in for.
#include "../../include/plume_hip.h"
#include "plume_capi_ctx.h"
#include "plume_eth_launch.h"

using namespace plume;

static int eth_hash_args_ok(int mode, size_t n, const void* off, const void* hash) {
    if (mode != PLUME_ETHK_HASH_KECCAK256 && mode != PLUME_ETHK_HASH_EIP191) return fail(PLUME_ERR_ARG, "mode must be 0 or 1");
    if (n && (!off || !hash)) return fail(PLUME_ERR_ARG, "null array");
    if (n > 0xFFFFFFF0u) return fail(PLUME_ERR_ARG, "n too large");
    return 0;
}
static int eth_hash_device(plume_ctx* ctx, int mode, size_t n, const uint8_t* msgs, const uint64_t* msg_off, size_t msgs_bytes, uint8_t* hash, hipStream_t st) {
    if (n == 0) return 0;
    if (!msgs && msgs_bytes) return fail(PLUME_ERR_ARG, "null message buffer");
    EthHashArgs a; a.mode = mode; a.n = (uint32_t)n; a.msgs = msgs; a.msg_off = msg_off; a.msgs_bytes = msgs ? msgs_bytes : 0; a.hash = hash;
    ctx->timer.begin(st);
    launch_eth_message_hash(a, st); ctx->timer.stage("eth_message_hash", st);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int plume_eth_message_hash_batch_device(plume_ctx* ctx, int mode, size_t n, const uint8_t* msgs, const uint64_t* msg_off, size_t msgs_bytes, uint8_t* hash32,
                                                   void* stream) {
    Route rt_(ctx, stream); ctx = rt_.lane; const hipStream_t st_ = rt_.st;
    if (int rc = bind(ctx)) return rc;
    if (int rc = eth_hash_args_ok(mode, n, msg_off, hash32)) return rc;
    return eth_hash_device(ctx, mode, n, msgs, msg_off, msgs_bytes, hash32, st_);
}
extern "C" int plume_eth_message_hash_batch(plume_ctx* ctx, int mode, size_t n, const uint8_t* msgs, const uint64_t* msg_off, uint8_t* hash32) {
    if (!ctx) return fail(PLUME_ERR_ARG, "null context");
    if (int rc = eth_hash_args_ok(mode, n, msg_off, hash32)) return rc;
    const HostCall call{msgs, msg_off, {}, {{hash32, 32}}};
    return serial_host_call_any(ctx, n, call, [&](HostSlot& sl, size_t cnt, plume_ctx* on) -> int {
        return eth_hash_device(on, mode, cnt, sl.msgs.as<uint8_t>(), sl.off.as<uint64_t>(), (size_t)sl.rel[cnt], sl.out[0].as<uint8_t>(), on->stream);
    });
}
