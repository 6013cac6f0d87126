// The few services of plume_capi.hip that other translation units of the library use (plume_nullset_capi.hip, plume_nonce_capi.hip, plume_selfcheck_capi.hip, plume_recover_capi.hip, plume_eth_capi.hip, plume_eth_hash_capi.hip, plume_ecdsa_capi.hip, plume_ecdsa_sign_capi.hip, plume_eth_tx_capi.hip, plume_eth_tx_sign_capi.hip, plume_merkle_capi.hip, plume_hd_capi.hip).  Internal: not part of the ABI, hidden in the shared object.
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

// The Ethereum-address call (plume_eth_address_batch*): one kernel on the caller's arrays, no tables and no workspace.  Its launcher comes in as a hook, like the three
// above.  The host-pointer form is a serial call (serial_host_call_any in plume_capi.hip: chunks of at most plume_set_chunk items through the context's first slot,
// one synchronise per chunk, the shards of a plume_init_multi context), as plume_scalars_to_sec1_der_batch is; the device form enqueues on the caller's stream and does
// not synchronise.
struct EthArgs;
typedef void (*EthLaunch)(const EthArgs& a, hipStream_t st);
__attribute__((visibility("hidden"))) int capi_eth_address(plume_ctx* ctx, int pk_format, int addr_format, size_t n, const uint8_t* pk, const uint8_t* expect,
                                                           uint8_t* address, uint8_t* status, EthLaunch eth_fn);
__attribute__((visibility("hidden"))) int capi_eth_address_device(plume_ctx* ctx, int pk_format, int addr_format, size_t n, const uint8_t* pk, const uint8_t* expect,
                                                                  uint8_t* address, uint8_t* status, void* stream, EthLaunch eth_fn);

// The ECDSA recovery (plume_ecdsa_recover_batch*): prepare, the table stage, the multiplication and its redo launch, the conversion to affine, finalize.  The three launchers
// of its own kernels come in as a hook struct, like the four above; the table stage and the conversion are plume_capi.hip's own.  The device form takes its workspace from the
// context (it joins the ws_free chain), honours plume_set_sub_batches and does not synchronise; the host-pointer form goes through serial_host_call_any, as
// plume_eth_address_batch does.
struct EcdsaArgs;
struct EcdsaLaunch {
    void (*prepare)(const EcdsaArgs& a, hipStream_t st);
    void (*mul)(const EcdsaArgs& a, hipStream_t st);
    void (*finalize)(const EcdsaArgs& a, hipStream_t st);
};
__attribute__((visibility("hidden"))) int capi_ecdsa_recover(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* hash, const uint8_t* r,
                                                             const uint8_t* s, const uint8_t* v, const uint8_t* expect, uint8_t* pk, uint8_t* address, uint8_t* status,
                                                             const EcdsaLaunch* fn);
__attribute__((visibility("hidden"))) int capi_ecdsa_recover_device(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* hash, const uint8_t* r,
                                                                    const uint8_t* s, const uint8_t* v, const uint8_t* expect, uint8_t* pk, uint8_t* address, uint8_t* status,
                                                                    void* stream, const EcdsaLaunch* fn);

// The message-hash call (plume_eth_message_hash_batch*): one kernel on the caller's arrays, no tables and no workspace, like the address call.  The host-pointer form goes
// through serial_host_call_any with the messages in its table (every chunk's bytes and its offsets, rebased to the chunk, are staged by stage_msgs; msgs may be null when
// it holds no bytes); the device form enqueues on the caller's stream and does not synchronise.
struct EthHashArgs;
typedef void (*EthHashLaunch)(const EthHashArgs& a, hipStream_t st);
__attribute__((visibility("hidden"))) int capi_eth_message_hash(plume_ctx* ctx, int mode, size_t n, const uint8_t* msgs, const uint64_t* msg_off, uint8_t* hash32,
                                                                EthHashLaunch hash_fn);
__attribute__((visibility("hidden"))) int capi_eth_message_hash_device(plume_ctx* ctx, int mode, size_t n, const uint8_t* msgs, const uint64_t* msg_off, size_t msgs_bytes,
                                                                       uint8_t* hash32, void* stream, EthHashLaunch hash_fn);

// The transaction calls (plume_eth_tx_parse_batch*, plume_eth_tx_sender_batch*).  parse: one kernel on the caller's arrays, through serial_host_call_any like the message-hash call.  sender: the
// same kernel into the context's staging (hash, r, s, v: 97 B / item), then the recover stages on it -- workspace, sub-batches, chunk limit and routing are those of
// capi_ecdsa_recover*.  The kernel's launcher comes in as a hook, the recover stages' as theirs.
struct EthTxArgs;
typedef void (*EthTxLaunch)(const EthTxArgs& a, hipStream_t st);
__attribute__((visibility("hidden"))) int capi_eth_tx_parse(plume_ctx* ctx, size_t n, const uint8_t* txs, const uint64_t* tx_off, uint8_t* hash32, uint8_t* r, uint8_t* s,
                                                            uint8_t* v, uint64_t* chain_id, uint8_t* tx_type, uint8_t* status, EthTxLaunch tx_fn);
__attribute__((visibility("hidden"))) int capi_eth_tx_parse_device(plume_ctx* ctx, size_t n, const uint8_t* txs, const uint64_t* tx_off, size_t txs_bytes, uint8_t* hash32,
                                                                   uint8_t* r, uint8_t* s, uint8_t* v, uint64_t* chain_id, uint8_t* tx_type, uint8_t* status, void* stream,
                                                                   EthTxLaunch tx_fn);
__attribute__((visibility("hidden"))) int capi_eth_tx_sender(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* txs, const uint64_t* tx_off,
                                                             const uint8_t* expect, uint8_t* pk, uint8_t* address, uint64_t* chain_id, uint8_t* tx_type, uint8_t* status,
                                                             EthTxLaunch tx_fn, const EcdsaLaunch* fn);
__attribute__((visibility("hidden"))) int capi_eth_tx_sender_device(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* txs,
                                                                    const uint64_t* tx_off, size_t txs_bytes, const uint8_t* expect, uint8_t* pk, uint8_t* address,
                                                                    uint64_t* chain_id, uint8_t* tx_type, uint8_t* status, void* stream, EthTxLaunch tx_fn,
                                                                    const EcdsaLaunch* fn);

// The Merkle calls (plume_merkle_leaf_batch*, plume_merkle_tree_build*, plume_merkle_proof_batch*, plume_merkle_verify_batch*).  leaf and verify are per-item calls on the
// caller's arrays, through serial_host_call_any like the address call (verify's root is a whole-call input; the device forms one kernel, no workspace).
// build and proof work on ONE tree: the host-pointer forms run on the context itself or on its first shard, the whole tree staged in the first slot (proof:
// serial_host_call with the tree as a whole-call input; build: one piece, serial_host_piece); build's sort
// takes its workspace (36 B per padded leaf) from the context, so its device form joins the ws_free chain.  fused_top = 0 (env PLUME_MERKLE_FUSED_TOP=0, the A/B
// knob of tests/gpu_debug/merkle_timing.py) runs one k_merkle_level launch per depth instead of k_merkle_top.  The launchers come in as a hook struct.
struct MerkleLeafArgs;
struct MerkleSortArgs;
struct MerkleTreeArgs;
struct MerkleProofArgs;
struct MerkleVerifyArgs;
struct MerkleLaunch {
    void (*leaf)(const MerkleLeafArgs& a, hipStream_t st);
    void (*sort)(const MerkleSortArgs& a, hipStream_t st);
    void (*place)(const MerkleTreeArgs& a, hipStream_t st);
    void (*level)(uint8_t* tree, uint32_t n, uint32_t d, hipStream_t st);
    void (*top)(uint8_t* tree, uint32_t n, uint32_t dtop, hipStream_t st);
    void (*proof)(const MerkleProofArgs& a, hipStream_t st);
    void (*verify)(const MerkleVerifyArgs& a, hipStream_t st);
};
__attribute__((visibility("hidden"))) int capi_merkle_leaf(plume_ctx* ctx, int leaf_format, int addr_format, size_t n, const uint8_t* address, const uint8_t* amount,
                                                           uint8_t* leaf32, uint8_t* status, const MerkleLaunch* fn);
__attribute__((visibility("hidden"))) int capi_merkle_leaf_device(plume_ctx* ctx, int leaf_format, int addr_format, size_t n, const uint8_t* address, const uint8_t* amount,
                                                                  uint8_t* leaf32, uint8_t* status, void* stream, const MerkleLaunch* fn);
__attribute__((visibility("hidden"))) int capi_merkle_tree_build(plume_ctx* ctx, int flags, size_t n, const uint8_t* leaf32, uint8_t* tree, uint32_t* leaf_pos,
                                                                 const MerkleLaunch* fn);
__attribute__((visibility("hidden"))) int capi_merkle_tree_build_device(plume_ctx* ctx, int flags, size_t n, const uint8_t* leaf32, uint8_t* tree, uint32_t* leaf_pos,
                                                                        void* stream, const MerkleLaunch* fn);
__attribute__((visibility("hidden"))) int capi_merkle_proof(plume_ctx* ctx, size_t n, const uint8_t* tree, size_t m, const uint32_t* pos, size_t depth, uint8_t* proof,
                                                            uint8_t* proof_len, const MerkleLaunch* fn);
__attribute__((visibility("hidden"))) int capi_merkle_proof_device(plume_ctx* ctx, size_t n, const uint8_t* tree, size_t m, const uint32_t* pos, size_t depth,
                                                                   uint8_t* proof, uint8_t* proof_len, void* stream, const MerkleLaunch* fn);
__attribute__((visibility("hidden"))) int capi_merkle_verify(plume_ctx* ctx, int leaf_format, int addr_format, size_t m, const uint8_t* address_or_leaf,
                                                             const uint8_t* amount, size_t depth, const uint8_t* proof, const uint8_t* proof_len, const uint8_t* root32,
                                                             uint8_t* status, const MerkleLaunch* fn);
__attribute__((visibility("hidden"))) int capi_merkle_verify_device(plume_ctx* ctx, int leaf_format, int addr_format, size_t m, const uint8_t* address_or_leaf,
                                                                    const uint8_t* amount, size_t depth, const uint8_t* proof, const uint8_t* proof_len,
                                                                    const uint8_t* root32, uint8_t* status, void* stream, const MerkleLaunch* fn);

// The ECDSA signer (plume_ecdsa_sign_batch*): nonce, the comb, the conversion to affine, finalize; with plume_set_sign_selfcheck on, the recover stages over the staged
// signatures and the release kernel behind them.  The launchers of its own kernels come in as a hook struct, with the recover stages' hooks beside them; the conversion and
// the table stage are plume_capi.hip's own.  Workspace waits, plume_set_sub_batches, the chunk limit, the in-flight lanes, the host pipeline (sk and aux staged and wiped)
// and sharding are those of plume_sign_batch_rfc6979*.  The comb (or, at level 2, the scanned table) is the only fixed table: never the verifier's window table.
struct EcdsaSignArgs;
struct EcdsaSignReleaseArgs;
struct EcdsaSignLaunch {
    void (*nonce)(const EcdsaSignArgs& a, hipStream_t st);
    void (*gmul)(const EcdsaSignArgs& a, hipStream_t st);
    void (*finalize)(const EcdsaSignArgs& a, hipStream_t st);
    void (*release)(const EcdsaSignReleaseArgs& a, hipStream_t st);
    const EcdsaLaunch* recover;
};
__attribute__((visibility("hidden"))) int capi_ecdsa_sign(plume_ctx* ctx, int flags, size_t n, const uint8_t* hash, const uint8_t* sk, const uint8_t* aux, uint8_t* r,
                                                          uint8_t* s, uint8_t* v, uint8_t* status, const EcdsaSignLaunch* fn);
__attribute__((visibility("hidden"))) int capi_ecdsa_sign_device(plume_ctx* ctx, int flags, size_t n, const uint8_t* hash, const uint8_t* sk, const uint8_t* aux,
                                                                 uint8_t* r, uint8_t* s, uint8_t* v, uint8_t* status, void* stream, const EcdsaSignLaunch* fn);

// The transaction signer (plume_eth_tx_sign_batch*): k_eth_tx_sign_frame into staging the context owns (the framing, the signing hash), the ECDSA signer's stages above on the
// staged hash -- tables, workspace, sub-batches, the uniform level, the self-check and the chunk limit are theirs --, k_eth_tx_sign_assemble into the caller's slots.  The two
// launchers come in as hooks, the signer's as its own hook struct.  The host-pointer form is a serial call (serial_host_call_any): the transactions staged as messages, sk and
// aux as secrets, `out` as the call's ragged output -- one contiguous download per piece.
struct EthTxSignArgs;
struct EthTxSignLaunch {
    void (*frame)(const EthTxSignArgs& a, hipStream_t st);
    void (*assemble)(const EthTxSignArgs& a, hipStream_t st);
    const EcdsaSignLaunch* sign;
};
__attribute__((visibility("hidden"))) int capi_eth_tx_sign(plume_ctx* ctx, int flags, size_t n, const uint8_t* txs, const uint64_t* tx_off, const uint8_t* sk, const uint8_t* aux,
                                                           uint8_t* out, uint32_t* out_len, uint8_t* hash32, uint8_t* r, uint8_t* s, uint8_t* v, uint64_t* chain_id,
                                                           uint8_t* tx_type, uint8_t* status, const EthTxSignLaunch* fn);
__attribute__((visibility("hidden"))) int capi_eth_tx_sign_device(plume_ctx* ctx, int flags, size_t n, const uint8_t* txs, const uint64_t* tx_off, size_t txs_bytes,
                                                                  const uint8_t* sk, const uint8_t* aux, uint8_t* out, size_t out_bytes, uint32_t* out_len, uint8_t* hash32,
                                                                  uint8_t* r, uint8_t* s, uint8_t* v, uint64_t* chain_id, uint8_t* tx_type, uint8_t* status, void* stream,
                                                                  const EthTxSignLaunch* fn);

// The key derivation (plume_hd_master_batch*, plume_hd_derive_priv_batch*, plume_hd_derive_pub_batch*).  master is one kernel on the caller's arrays.  The two derive calls
// keep k, the chain code and the status of every item in staging the context owns (65 B / item) and the points in the signer's result array: load, then per level the comb
// (private form: at the context's uniform level), the conversion to affine and the step kernel, then finish into the caller's arrays.  The staging and the Jacobian images
// are wiped on the call's stream behind finish, and on failure paths too.  Tables, the workspace chain, the chunk limit and routing are the ECDSA signer's; the launchers come
// in as a hook struct.  The host-pointer forms are serial calls (serial_host_call_any): sk, chain codes and seeds staged as secrets -- inputs and outputs --, a shared
// parent or path as whole-call inputs.
struct HdArgs;
struct HdLaunch {
    void (*master)(const HdArgs& a, hipStream_t st);
    void (*priv_load)(const HdArgs& a, hipStream_t st);
    void (*pub_load)(const HdArgs& a, hipStream_t st);
    void (*gmul)(const HdArgs& a, hipStream_t st);
    void (*priv_step)(const HdArgs& a, hipStream_t st);
    void (*pub_step)(const HdArgs& a, hipStream_t st);
    void (*finish)(const HdArgs& a, hipStream_t st);
};
__attribute__((visibility("hidden"))) int capi_hd_master(plume_ctx* ctx, size_t n, const uint8_t* seed, size_t seed_len, uint8_t* sk, uint8_t* chain, uint8_t* status,
                                                         const HdLaunch* fn);
__attribute__((visibility("hidden"))) int capi_hd_master_device(plume_ctx* ctx, size_t n, const uint8_t* seed, size_t seed_len, uint8_t* sk, uint8_t* chain, uint8_t* status,
                                                                void* stream, const HdLaunch* fn);
// pub = false: parent is sk, child_sk is required.  pub = true: parent is pk in pk_format, child_sk is NULL and child_pk required
__attribute__((visibility("hidden"))) int capi_hd_derive(plume_ctx* ctx, bool pub, int flags, int pk_format, int addr_format, size_t n, const uint8_t* parent,
                                                         const uint8_t* parent_chain, const uint32_t* path, size_t depth, uint8_t* child_sk, uint8_t* child_chain,
                                                         uint8_t* child_pk, uint8_t* address, uint8_t* status, const HdLaunch* fn);
__attribute__((visibility("hidden"))) int capi_hd_derive_device(plume_ctx* ctx, bool pub, int flags, int pk_format, int addr_format, size_t n, const uint8_t* parent,
                                                                const uint8_t* parent_chain, const uint32_t* path, size_t depth, uint8_t* child_sk, uint8_t* child_chain,
                                                                uint8_t* child_pk, uint8_t* address, uint8_t* status, void* stream, const HdLaunch* fn);

}  // namespace plume
