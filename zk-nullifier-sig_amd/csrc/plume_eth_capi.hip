// C ABI of the Ethereum-address call (include/plume_hip.h, plume_eth_address_batch*): hands k_eth_address's launcher to the host side of plume_capi.hip as a hook.
// Kept apart from plume_capi.hip so that the CPU build of that file (tests/hostsim) links without this kernel's launcher.
#include "../../include/plume_hip.h"
#include "plume_capi_internal.h"
#include "plume_eth_launch.h"

using namespace plume;

extern "C" int plume_eth_address_batch(plume_ctx* ctx, int pk_format, int addr_format, size_t n, const uint8_t* pk, const uint8_t* expect, uint8_t* address,
                                       uint8_t* status) {
    return capi_eth_address(ctx, pk_format, addr_format, n, pk, expect, address, status, launch_eth_address);
}
extern "C" int plume_eth_address_batch_device(plume_ctx* ctx, int pk_format, int addr_format, size_t n, const uint8_t* pk, const uint8_t* expect, uint8_t* address,
                                              uint8_t* status, void* stream) {
    return capi_eth_address_device(ctx, pk_format, addr_format, n, pk, expect, address, status, stream, launch_eth_address);
}
