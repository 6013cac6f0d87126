// C ABI of the transaction signer (include/plume_hip.h, plume_eth_tx_sign_batch*): hands the launchers of its two kernels, of the ECDSA signer's stages and -- for the
// self-check -- of the recover stages to the host side of plume_capi.hip as hooks.  Kept apart from plume_capi.hip so that the CPU build of that file (tests/hostsim) links
// without these launchers.
#include "../../include/plume_hip.h"
#include "plume_capi_internal.h"
#include "plume_ecdsa_launch.h"
#include "plume_ecdsa_sign_launch.h"
#include "plume_eth_tx_sign_launch.h"

using namespace plume;

static_assert(PLUME_ETH_TX_SIGN_GROWTH == PLUME_ETHTXK_SIGN_GROWTH && PLUME_STATUS_BAD_TX == PLUME_ST_BAD_TX, "the header and the kernels state the same constants");

static const EcdsaLaunch kRecoverLaunch = {launch_ecdsa_prepare, launch_ecdsa_mul, launch_ecdsa_finalize};
static const EcdsaSignLaunch kSignLaunch = {launch_ecdsa_sign_nonce, launch_ecdsa_sign_gmul, launch_ecdsa_sign_finalize, launch_ecdsa_sign_release, &kRecoverLaunch};
static const EthTxSignLaunch kTxSignLaunch = {launch_eth_tx_sign_frame, launch_eth_tx_sign_assemble, &kSignLaunch};

extern "C" size_t plume_eth_tx_sign_out_bytes(size_t n, uint64_t txs_bytes) { return (size_t)txs_bytes + (size_t)PLUME_ETH_TX_SIGN_GROWTH * n; }

extern "C" int plume_eth_tx_sign_batch(plume_ctx* ctx, int flags, size_t n, const uint8_t* txs, const uint64_t* tx_off, const uint8_t* sk, const uint8_t* aux, uint8_t* out,
                                       uint32_t* out_len, uint8_t* hash32, uint8_t* r, uint8_t* s, uint8_t* v, uint64_t* chain_id, uint8_t* tx_type, uint8_t* status) {
    return capi_eth_tx_sign(ctx, flags, n, txs, tx_off, sk, aux, out, out_len, hash32, r, s, v, chain_id, tx_type, status, &kTxSignLaunch);
}
extern "C" int plume_eth_tx_sign_batch_device(plume_ctx* ctx, int flags, size_t n, const uint8_t* txs, const uint64_t* tx_off, size_t txs_bytes, const uint8_t* sk,
                                              const uint8_t* aux, uint8_t* out, size_t out_bytes, uint32_t* out_len, uint8_t* hash32, uint8_t* r, uint8_t* s, uint8_t* v,
                                              uint64_t* chain_id, uint8_t* tx_type, uint8_t* status, void* stream) {
    return capi_eth_tx_sign_device(ctx, flags, n, txs, tx_off, txs_bytes, sk, aux, out, out_bytes, out_len, hash32, r, s, v, chain_id, tx_type, status, stream,
                                   &kTxSignLaunch);
}
