// C ABI of the ECDSA signing call (include/plume_hip.h, plume_ecdsa_sign_batch*): hands the launchers of its kernels -- and, for the self-check, those of the recover
// stages -- to the host side of plume_capi.hip as hooks.
// Kept apart from plume_capi.hip so that the CPU build of that file (tests/hostsim) links without these kernels' launchers.
#include "../../include/plume_hip.h"
#include "plume_capi_internal.h"
#include "plume_ecdsa_launch.h"
#include "plume_ecdsa_sign_launch.h"

using namespace plume;

static const EcdsaLaunch kRecoverLaunch = {launch_ecdsa_prepare, launch_ecdsa_mul, launch_ecdsa_finalize};
static const EcdsaSignLaunch kSignLaunch = {launch_ecdsa_sign_nonce, launch_ecdsa_sign_gmul, launch_ecdsa_sign_finalize, launch_ecdsa_sign_release, &kRecoverLaunch};

extern "C" int plume_ecdsa_sign_batch(plume_ctx* ctx, int flags, size_t n, const uint8_t* hash, const uint8_t* sk, const uint8_t* aux, uint8_t* r, uint8_t* s, uint8_t* v,
                                      uint8_t* status) {
    return capi_ecdsa_sign(ctx, flags, n, hash, sk, aux, r, s, v, status, &kSignLaunch);
}
extern "C" int plume_ecdsa_sign_batch_device(plume_ctx* ctx, int flags, size_t n, const uint8_t* hash, const uint8_t* sk, const uint8_t* aux, uint8_t* r, uint8_t* s,
                                             uint8_t* v, uint8_t* status, void* stream) {
    return capi_ecdsa_sign_device(ctx, flags, n, hash, sk, aux, r, s, v, status, stream, &kSignLaunch);
}
