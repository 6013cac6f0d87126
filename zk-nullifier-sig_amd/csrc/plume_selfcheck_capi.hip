// C ABI of the signer's self-check switch (include/plume_hip.h, plume_set_sign_selfcheck): hands k_sign_release's launcher to the sign pipeline of plume_capi.hip as a hook.
// Kept apart from plume_capi.hip so that the CPU build of that file (tests/hostsim) links without this kernel's launcher.
#include "../../include/plume_hip.h"
#include "plume_capi_internal.h"
#include "plume_selfcheck_launch.h"

using namespace plume;

// contexts whose default comes from the environment (PLUME_SIGN_SELFCHECK) find the launcher here, before any setter has run
static const int g_release_registered = capi_sign_release_hook(launch_sign_release);

extern "C" int plume_set_sign_selfcheck(plume_ctx* ctx, int mode) {
    (void)g_release_registered;
    return capi_set_sign_selfcheck(ctx, mode, launch_sign_release);
}
