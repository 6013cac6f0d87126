// The Ethereum-address call (include/plume_hip.h, plume_eth_address_batch*): its C ABI and its host side.  One kernel on the caller's arrays: no table is needed and no
// workspace is touched, so the call neither builds anything nor joins the ws_free chain.  The host-pointer form is a serial call (serial_host_call_any in plume_capi.hip:
// chunks of at most plume_set_chunk items through the context's first slot, one synchronise per chunk, the shards of a plume_init_multi context), as
// plume_scalars_to_sec1_der_batch is; the device form enqueues on the caller's stream and does not synchronise.
#include "../../include/plume_hip.h"
#include "plume_capi_ctx.h"
#include "plume_eth_launch.h"

using namespace plume;

static int eth_args_ok(int pk_format, int addr_format, size_t n, const void* pk, const void* address, const void* status) {
    if (pk_format != PLUME_ETHK_PK_AFFINE64 && pk_format != PLUME_ETHK_PK_SEC1) return fail(PLUME_ERR_ARG, "pk_format must be 0 or 1");
    if (addr_format != PLUME_ETHK_ADDR_RAW20 && addr_format != PLUME_ETHK_ADDR_RECORD64 && addr_format != PLUME_ETHK_ADDR_EIP55) return fail(PLUME_ERR_ARG, "addr_format must be 0, 1 or 2");
    if (n && !pk) return fail(PLUME_ERR_ARG, "null array");
    if (n && !address && !status) return fail(PLUME_ERR_ARG, "no output array");
    if (n > 0xFFFFFFF0u) return fail(PLUME_ERR_ARG, "n too large");
    return 0;
}
static int eth_device(plume_ctx* ctx, int pk_format, int addr_format, size_t n, const uint8_t* pk, const uint8_t* expect, uint8_t* address, uint8_t* status, hipStream_t st) {
    if (n == 0) return 0;
    EthArgs a; a.pk_format = pk_format; a.addr_format = addr_format; a.n = (uint32_t)n; a.pk = pk; a.expect = expect; a.address = address; a.status = status;
    ctx->timer.begin(st);
    launch_eth_address(a, st); ctx->timer.stage("eth_address", st);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int plume_eth_address_batch_device(plume_ctx* ctx, int pk_format, int addr_format, size_t n, const uint8_t* pk, const uint8_t* expect, uint8_t* address,
                                              uint8_t* status, void* stream) {
    Route rt_(ctx, stream); ctx = rt_.lane; const hipStream_t st_ = rt_.st;
    if (int rc = bind(ctx)) return rc;
    if (int rc = eth_args_ok(pk_format, addr_format, n, pk, address, status)) return rc;
    return eth_device(ctx, pk_format, addr_format, n, pk, expect, address, status, st_);
}
extern "C" int plume_eth_address_batch(plume_ctx* ctx, int pk_format, int addr_format, size_t n, const uint8_t* pk, const uint8_t* expect, uint8_t* address,
                                       uint8_t* status) {
    if (!ctx) return fail(PLUME_ERR_ARG, "null context");
    if (int rc = eth_args_ok(pk_format, addr_format, n, pk, address, status)) return rc;
    const HostCall call{nullptr, nullptr, {{pk, eth_pk_width(pk_format)}, {expect, 20}}, {{address, eth_address_width(addr_format)}, {status, 1}}};
    return serial_host_call_any(ctx, n, call, [&](HostSlot& sl, size_t cnt, plume_ctx* on) -> int {
        return eth_device(on, pk_format, addr_format, cnt, sl.in[0].as<uint8_t>(), expect ? sl.in[1].as<uint8_t>() : nullptr, address ? sl.out[0].as<uint8_t>() : nullptr,
                          status ? sl.out[1].as<uint8_t>() : nullptr, on->stream);
    });
}
