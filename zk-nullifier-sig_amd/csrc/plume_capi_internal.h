// The few services of plume_capi.hip that other translation units of the library use (plume_nullset_capi.hip).  Internal: not part of the ABI, hidden in the shared object.
#pragma once
#include <stddef.h>

struct plume_ctx;

namespace plume {

// sets this thread's plume_last_error() text; returns code
__attribute__((visibility("hidden"))) int capi_fail(int code, const char* msg);
// the device a context's single-device work runs on: its own, or its first shard's for a plume_init_multi context.  PLUME_ERR_ARG for a null context
__attribute__((visibility("hidden"))) int capi_ctx_device(const plume_ctx* ctx, int* device);
// len bytes of the OS generator (getrandom); false if it failed
__attribute__((visibility("hidden"))) bool capi_os_random(void* out, size_t len);

}  // namespace plume
