// C ABI of the derived-nonce signer (include/plume_hip.h, plume_sign_batch_rfc6979*): the sign pipeline of plume_capi.hip with k_sign_nonce as its nonce hook.
// Kept apart from plume_capi.hip so that the CPU build of that file (tests/hostsim) links without this kernel's launcher.
#include "../../include/plume_hip.h"
#include "plume_capi_internal.h"
#include "plume_nonce_launch.h"

using namespace plume;

extern "C" int plume_sign_batch_rfc6979(plume_ctx* ctx, int version, size_t n, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* sk, const uint8_t* aux,
                                        const uint8_t* pk_in, uint8_t* pk, uint8_t* nullifier, uint8_t* c, uint8_t* s, uint8_t* r_point, uint8_t* hashed_to_curve_r,
                                        uint8_t* status) {
    return capi_sign_derived(ctx, version, n, msgs, msg_off, sk, aux, pk_in, pk, nullifier, c, s, r_point, hashed_to_curve_r, status, launch_sign_nonce);
}

extern "C" int plume_sign_batch_rfc6979_device(plume_ctx* ctx, int version, size_t n, const uint8_t* msgs, const uint64_t* msg_off, size_t msgs_bytes, const uint8_t* sk,
                                               const uint8_t* aux, const uint8_t* pk_in, uint8_t* pk, uint8_t* nullifier, uint8_t* c, uint8_t* s, uint8_t* r_point,
                                               uint8_t* hashed_to_curve_r, uint8_t* status, void* stream) {
    return capi_sign_derived_device(ctx, version, n, msgs, msg_off, msgs_bytes, sk, aux, pk_in, pk, nullifier, c, s, r_point, hashed_to_curve_r, status, stream,
                                    launch_sign_nonce);
}
