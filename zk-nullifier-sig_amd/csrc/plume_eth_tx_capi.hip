// C ABI of the transaction calls (include/plume_hip.h, plume_eth_tx_parse_batch*, plume_eth_tx_sender_batch*): hands k_eth_tx_parse's launcher, and for the sender the
// launchers of the recover stages, to the host side of plume_capi.hip as hooks.  Kept apart from plume_capi.hip so that the CPU build of that file (tests/hostsim) links
// without these launchers.
#include "../../include/plume_hip.h"
#include "plume_capi_internal.h"
#include "plume_ecdsa_launch.h"
#include "plume_eth_tx_launch.h"

using namespace plume;

static const EcdsaLaunch kRecoverLaunch = {launch_ecdsa_prepare, launch_ecdsa_mul, launch_ecdsa_finalize};

extern "C" int plume_eth_tx_parse_batch(plume_ctx* ctx, size_t n, const uint8_t* txs, const uint64_t* tx_off, uint8_t* hash32, uint8_t* r, uint8_t* s, uint8_t* v,
                                        uint64_t* chain_id, uint8_t* tx_type, uint8_t* status) {
    return capi_eth_tx_parse(ctx, n, txs, tx_off, hash32, r, s, v, chain_id, tx_type, status, launch_eth_tx_parse);
}
extern "C" int plume_eth_tx_parse_batch_device(plume_ctx* ctx, size_t n, const uint8_t* txs, const uint64_t* tx_off, size_t txs_bytes, uint8_t* hash32, uint8_t* r,
                                               uint8_t* s, uint8_t* v, uint64_t* chain_id, uint8_t* tx_type, uint8_t* status, void* stream) {
    return capi_eth_tx_parse_device(ctx, n, txs, tx_off, txs_bytes, hash32, r, s, v, chain_id, tx_type, status, stream, launch_eth_tx_parse);
}
extern "C" int plume_eth_tx_sender_batch(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* txs, const uint64_t* tx_off,
                                         const uint8_t* expect, uint8_t* pk, uint8_t* address, uint64_t* chain_id, uint8_t* tx_type, uint8_t* status) {
    return capi_eth_tx_sender(ctx, flags, pk_format, addr_format, n, txs, tx_off, expect, pk, address, chain_id, tx_type, status, launch_eth_tx_parse, &kRecoverLaunch);
}
extern "C" int plume_eth_tx_sender_batch_device(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* txs, const uint64_t* tx_off,
                                                size_t txs_bytes, const uint8_t* expect, uint8_t* pk, uint8_t* address, uint64_t* chain_id, uint8_t* tx_type, uint8_t* status,
                                                void* stream) {
    return capi_eth_tx_sender_device(ctx, flags, pk_format, addr_format, n, txs, tx_off, txs_bytes, expect, pk, address, chain_id, tx_type, status, stream,
                                     launch_eth_tx_parse, &kRecoverLaunch);
}
