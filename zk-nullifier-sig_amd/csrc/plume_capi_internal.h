// The few services of plume_capi.hip that other translation units of the library use through launcher hooks or without knowing the context's layout (plume_nullset_capi.hip, plume_nonce_capi.hip, plume_selfcheck_capi.hip, plume_recover_capi.hip).  The three hooks here are called from inside sign_device / verify_device, which the CPU harness (tests/hostsim) links without those launchers; the call families that hold their own host side use plume_capi_ctx.h instead.  Internal: not part of the ABI, hidden in the shared object.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

struct plume_ctx;

namespace plume {

// sets this thread's plume_last_error() text; returns code
__attribute__((visibility("hidden"))) int capi_fail(int code, const char* msg);
// the device a context's single-device work runs on: its own, or its first shard's for a plume_init_multi context.  PLUME_ERR_ARG for a null context
__attribute__((visibility("hidden"))) int capi_ctx_device(const plume_ctx* ctx, int* device);
// len bytes of the OS generator (getrandom); false if it failed
__attribute__((visibility("hidden"))) bool capi_os_random(void* out, size_t len);

// The derived-nonce signer (plume_sign_batch_rfc6979*): the sign pipeline with r computed on the device.  The launcher of the nonce kernel comes in as a hook, so
// that plume_capi.hip never names it; it is called once per sub-batch, on the stream of the stages in front of the multiplications by G, and writes the
// workspace buffer that SignArgs::r then points at.  Arguments, routing, sharding and error codes are those of plume_sign_batch / plume_sign_batch_device.
struct NonceArgs;
typedef void (*SignNonceLaunch)(const NonceArgs& a, hipStream_t st);
__attribute__((visibility("hidden"))) int capi_sign_derived(plume_ctx* ctx, int version, size_t n, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* sk,
                                                            const uint8_t* aux, const uint8_t* pk_in, uint8_t* pk, uint8_t* nullifier, uint8_t* c, uint8_t* s,
                                                            uint8_t* r_point, uint8_t* hashed_to_curve_r, uint8_t* status, SignNonceLaunch nonce_fn);
__attribute__((visibility("hidden"))) int capi_sign_derived_device(plume_ctx* ctx, int version, size_t n, const uint8_t* msgs, const uint64_t* msg_off, size_t msgs_bytes,
                                                                   const uint8_t* sk, const uint8_t* aux, const uint8_t* pk_in, uint8_t* pk, uint8_t* nullifier, uint8_t* c,
                                                                   uint8_t* s, uint8_t* r_point, uint8_t* hashed_to_curve_r, uint8_t* status, void* stream,
                                                                   SignNonceLaunch nonce_fn);

// The signer's self-check (plume_set_sign_selfcheck): with mode 1 every sign entry point stages its outputs in the context, checks them with the verifier's stages and
// lets the release kernel write the caller's arrays.  That kernel's launcher comes in as a hook, like the nonce kernel's: plume_capi.hip never names it.
// capi_sign_release_hook files the launcher for contexts that take their mode from the environment (returns 0); capi_set_sign_selfcheck is the setter's body.
struct ReleaseArgs;
typedef void (*SignReleaseLaunch)(const ReleaseArgs& a, hipStream_t st);
__attribute__((visibility("hidden"))) int capi_sign_release_hook(SignReleaseLaunch release_fn);
__attribute__((visibility("hidden"))) int capi_set_sign_selfcheck(plume_ctx* ctx, int mode, SignReleaseLaunch release_fn);

// The point recovery (plume_recover_batch*): the V2 verify pipeline with k_recover_finalize in place of k_verify_finalize.  That kernel's launcher comes in as a hook, like
// the two above: plume_capi.hip never names it.  It is called once per sub-batch, on the caller's stream, behind the conversion of the two results to affine.
// Arguments, routing, sharding and error codes are those of plume_verify_batch / plume_verify_batch_device.
struct RecoverArgs;
typedef void (*RecoverLaunch)(const RecoverArgs& a, hipStream_t st);
__attribute__((visibility("hidden"))) int capi_recover(plume_ctx* ctx, int version, int format, size_t n, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* pk,
                                                       const uint8_t* nullifier, const uint8_t* c, const uint8_t* s, uint8_t* r_point, uint8_t* hashed_to_curve_r,
                                                       uint8_t* hashed_to_curve, uint8_t* status, RecoverLaunch recover_fn);
__attribute__((visibility("hidden"))) int capi_recover_device(plume_ctx* ctx, int version, int format, size_t n, const uint8_t* msgs, const uint64_t* msg_off, size_t msgs_bytes,
                                                              const uint8_t* pk, const uint8_t* nullifier, const uint8_t* c, const uint8_t* s, uint8_t* r_point,
                                                              uint8_t* hashed_to_curve_r, uint8_t* hashed_to_curve, uint8_t* status, void* stream, RecoverLaunch recover_fn);

}  // namespace plume
