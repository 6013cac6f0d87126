// C ABI of the ECDSA recovery (include/plume_hip.h, plume_ecdsa_recover_batch*): hands the launchers of its three kernels to the host side of plume_capi.hip as hooks.
// Kept apart from plume_capi.hip so that the CPU build of that file (tests/hostsim) links without these kernels' launchers.
#include "../../include/plume_hip.h"
#include "plume_capi_internal.h"
#include "plume_ecdsa_launch.h"

using namespace plume;

static const EcdsaLaunch kEcdsaLaunch = {launch_ecdsa_prepare, launch_ecdsa_mul, launch_ecdsa_finalize};

extern "C" int plume_ecdsa_recover_batch(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* hash, const uint8_t* r, const uint8_t* s,
                                         const uint8_t* v, const uint8_t* expect, uint8_t* pk, uint8_t* address, uint8_t* status) {
    return capi_ecdsa_recover(ctx, flags, pk_format, addr_format, n, hash, r, s, v, expect, pk, address, status, &kEcdsaLaunch);
}
extern "C" int plume_ecdsa_recover_batch_device(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* hash, const uint8_t* r, const uint8_t* s,
                                                const uint8_t* v, const uint8_t* expect, uint8_t* pk, uint8_t* address, uint8_t* status, void* stream) {
    return capi_ecdsa_recover_device(ctx, flags, pk_format, addr_format, n, hash, r, s, v, expect, pk, address, status, stream, &kEcdsaLaunch);
}
