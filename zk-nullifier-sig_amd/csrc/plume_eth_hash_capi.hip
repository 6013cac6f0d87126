// C ABI of the message-hash call (include/plume_hip.h, plume_eth_message_hash_batch*): hands k_eth_message_hash's launcher to the host side of plume_capi.hip as a hook.
// Kept apart from plume_capi.hip so that the CPU build of that file (tests/hostsim) links without this kernel's launcher, and apart from plume_eth_capi.hip so that the
// harness of the address call links with the one launcher it stands in for.
#include "../../include/plume_hip.h"
#include "plume_capi_internal.h"
#include "plume_eth_launch.h"

using namespace plume;

extern "C" int plume_eth_message_hash_batch(plume_ctx* ctx, int mode, size_t n, const uint8_t* msgs, const uint64_t* msg_off, uint8_t* hash32) {
    return capi_eth_message_hash(ctx, mode, n, msgs, msg_off, hash32, launch_eth_message_hash);
}
extern "C" int plume_eth_message_hash_batch_device(plume_ctx* ctx, int mode, size_t n, const uint8_t* msgs, const uint64_t* msg_off, size_t msgs_bytes, uint8_t* hash32,
                                                   void* stream) {
    return capi_eth_message_hash_device(ctx, mode, n, msgs, msg_off, msgs_bytes, hash32, stream, launch_eth_message_hash);
}
