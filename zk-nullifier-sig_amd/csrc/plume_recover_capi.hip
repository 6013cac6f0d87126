// C ABI of the point recovery (include/plume_hip.h, plume_recover_batch*): hands k_recover_finalize's launcher to the verify pipeline of plume_capi.hip as a hook.
// Kept apart from plume_capi.hip so that the CPU build of that file (tests/hostsim) links without this kernel's launcher.
#include "../../include/plume_hip.h"
#include "plume_capi_internal.h"
#include "plume_recover_launch.h"

using namespace plume;

extern "C" int plume_recover_batch(plume_ctx* ctx, int version, int format, size_t n, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* pk,
                                   const uint8_t* nullifier, const uint8_t* c, const uint8_t* s, uint8_t* r_point, uint8_t* hashed_to_curve_r, uint8_t* hashed_to_curve,
                                   uint8_t* status) {
    return capi_recover(ctx, version, format, n, msgs, msg_off, pk, nullifier, c, s, r_point, hashed_to_curve_r, hashed_to_curve, status, launch_recover_finalize);
}
extern "C" int plume_recover_batch_device(plume_ctx* ctx, int version, int format, size_t n, const uint8_t* msgs, const uint64_t* msg_off, size_t msgs_bytes,
                                          const uint8_t* pk, const uint8_t* nullifier, const uint8_t* c, const uint8_t* s, uint8_t* r_point, uint8_t* hashed_to_curve_r,
                                          uint8_t* hashed_to_curve, uint8_t* status, void* stream) {
    return capi_recover_device(ctx, version, format, n, msgs, msg_off, msgs_bytes, pk, nullifier, c, s, r_point, hashed_to_curve_r, hashed_to_curve, status, stream,
                               launch_recover_finalize);
}
