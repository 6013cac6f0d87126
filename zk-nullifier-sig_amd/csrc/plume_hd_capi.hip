// C ABI of the key derivation (include/plume_hip.h, plume_hd_master_batch*, plume_hd_derive_priv_batch*, plume_hd_derive_pub_batch*): hands the launchers of its kernels to
// the host side of plume_capi.hip as hooks.  Kept apart from plume_capi.hip so that the CPU build of that file (tests/hostsim) links without these launchers.
#include "../../include/plume_hip.h"
#include "plume_capi_internal.h"
#include "plume_hd_launch.h"

using namespace plume;

static_assert(PLUME_HD_MAX_DEPTH == PLUME_HDK_MAX_DEPTH && PLUME_HD_SHARED_PARENT == PLUME_HDK_SHARED_PARENT && PLUME_HD_SHARED_PATH == PLUME_HDK_SHARED_PATH &&
                  PLUME_STATUS_HD_NO_KEY == PLUME_ST_HD_NO_KEY && PLUME_STATUS_HD_HARDENED == PLUME_ST_HD_HARDENED,
              "the header and the kernels state the same constants");

static const HdLaunch kHdLaunch = {launch_hd_master, launch_hd_priv_load, launch_hd_pub_load, launch_hd_gmul, launch_hd_priv_step, launch_hd_pub_step, launch_hd_finish};

extern "C" int plume_hd_master_batch(plume_ctx* ctx, size_t n, const uint8_t* seed, size_t seed_len, uint8_t* sk, uint8_t* chain, uint8_t* status) {
    return capi_hd_master(ctx, n, seed, seed_len, sk, chain, status, &kHdLaunch);
}
extern "C" int plume_hd_master_batch_device(plume_ctx* ctx, size_t n, const uint8_t* seed, size_t seed_len, uint8_t* sk, uint8_t* chain, uint8_t* status, void* stream) {
    return capi_hd_master_device(ctx, n, seed, seed_len, sk, chain, status, stream, &kHdLaunch);
}
extern "C" int plume_hd_derive_priv_batch(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* parent_sk, const uint8_t* parent_chain,
                                          const uint32_t* path, size_t depth, uint8_t* child_sk, uint8_t* child_chain, uint8_t* child_pk, uint8_t* address, uint8_t* status) {
    return capi_hd_derive(ctx, false, flags, pk_format, addr_format, n, parent_sk, parent_chain, path, depth, child_sk, child_chain, child_pk, address, status, &kHdLaunch);
}
extern "C" int plume_hd_derive_priv_batch_device(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* parent_sk, const uint8_t* parent_chain,
                                                 const uint32_t* path, size_t depth, uint8_t* child_sk, uint8_t* child_chain, uint8_t* child_pk, uint8_t* address,
                                                 uint8_t* status, void* stream) {
    return capi_hd_derive_device(ctx, false, flags, pk_format, addr_format, n, parent_sk, parent_chain, path, depth, child_sk, child_chain, child_pk, address, status, stream,
                                 &kHdLaunch);
}
extern "C" int plume_hd_derive_pub_batch(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* parent_pk, const uint8_t* parent_chain,
                                         const uint32_t* path, size_t depth, uint8_t* child_pk, uint8_t* child_chain, uint8_t* address, uint8_t* status) {
    return capi_hd_derive(ctx, true, flags, pk_format, addr_format, n, parent_pk, parent_chain, path, depth, nullptr, child_chain, child_pk, address, status, &kHdLaunch);
}
extern "C" int plume_hd_derive_pub_batch_device(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* parent_pk, const uint8_t* parent_chain,
                                                const uint32_t* path, size_t depth, uint8_t* child_pk, uint8_t* child_chain, uint8_t* address, uint8_t* status, void* stream) {
    return capi_hd_derive_device(ctx, true, flags, pk_format, addr_format, n, parent_pk, parent_chain, path, depth, nullptr, child_chain, child_pk, address, status, stream,
                                 &kHdLaunch);
}
