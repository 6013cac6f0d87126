//! Batch PLUME on AMD MI355X through `libplume_hip.so` (C ABI: `include/plume_hip.h`) behind the `plume_rustcrypto` surface.
//!
//! NOT COMPILED in the build image (it has no Rust toolchain): this crate is the binding `INTEGRATION.md` describes, kept complete so that a
//! maintainer with `cargo` only has to build it.  The same FFI surface IS exercised from a non-Python caller by `tests/abi_c/abi_smoke.c`
//! (plain C, same symbols, same argument order), and from Python by `zk_nullifier_sig_amd` (ctypes).
//!
//! Shape: the reference's own types and method names (`rust-k256/src/lib.rs:67-156`, `rust-k256/src/randomizedsigner.rs:25-47`) with a batch
//! twin for every entry point.  Inside `rust-k256` the record would be `crate::PlumeSignature`; as a standalone crate it is mirrored here.
//!
//! ```ignore
//! let engine = HipEngine::new(0)?;                                  // or HipEngine::new_multi(&[0, 1, 2, 3, 4, 5, 6, 7])?
//! let oks: Vec<bool> = engine.verify_batch(&sigs)?;                 // sigs[i].verify()
//! let sigs = engine.sign_batch(&keys, &msgs, true, &mut OsRng)?;    // PlumeSigner::new(&keys[i], true).sign_with_rng(rng, msgs[i])
//! ```
use k256::elliptic_curve::sec1::{FromEncodedPoint, ToEncodedPoint};
use k256::elliptic_curve::rand_core::CryptoRngCore;
use k256::{AffinePoint, EncodedPoint, FieldBytes, NonZeroScalar, SecretKey};
use std::os::raw::{c_char, c_int, c_void};

/// `plume_rustcrypto::PlumeSignatureV1Fields` (rust-k256/src/lib.rs:84-89)
#[derive(Clone, Debug, PartialEq)]
pub struct PlumeSignatureV1Fields {
    pub r_point: AffinePoint,
    pub hashed_to_curve_r: AffinePoint,
}
/// `plume_rustcrypto::PlumeSignature` (rust-k256/src/lib.rs:67-80)
#[derive(Clone, Debug, PartialEq)]
pub struct PlumeSignature {
    pub message: Vec<u8>,
    pub pk: AffinePoint,
    pub nullifier: AffinePoint,
    pub c: NonZeroScalar,
    pub s: NonZeroScalar,
    pub v1specific: Option<PlumeSignatureV1Fields>,
}

/// What the reference signals by `panic!` / `Err` inside `try_sign_with_rng` (randomizedsigner.rs:59-61,90-95), per item of a batch.
#[derive(Clone, Debug, PartialEq, Eq)]
pub enum SignError {
    /// "something is drammatically wrong if the input hashed to the identity" (randomizedsigner.rs:61)
    HashedToIdentity,
    /// "it should be impossible to get the hash equal to zero" — the digest is 0 or >= n (randomizedsigner.rs:90-91)
    ChallengeNotCanonical,
    /// "the nonce is equal to negated product of the secret and the hash" — s == 0 (randomizedsigner.rs:95)
    ZeroResponse,
    /// a scalar outside [1, n-1] reached the library (cannot happen through `SecretKey` / `NonZeroScalar`)
    BadScalar,
    /// the signer's self-check (`Engine::set_sign_selfcheck(1)`) withheld the item: the signer called it good but its records do not verify.  Not one of the
    /// reference's panics: the reference releases such a signature
    SelfCheckFailed,
}

#[derive(Debug)]
pub struct HipError(pub String);
impl std::fmt::Display for HipError {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result { write!(f, "plume_hip: {}", self.0) }
}
impl std::error::Error for HipError {}
impl HipError {
    /// What `PlumeSigner::try_sign_with_rng` / `sign_deterministic` return when the signer's self-check (`HipEngine::set_sign_selfcheck(1)`) withheld the signature:
    /// not a failed library call and not one of the reference's panics -- the signature was computed, did not verify and was not released.
    pub const SELF_CHECK_FAILED: &'static str = "the signature does not verify and was withheld by the signer's self-check";
    pub fn self_check_failed() -> Self { HipError(Self::SELF_CHECK_FAILED.to_string()) }
    pub fn is_self_check_failed(&self) -> bool { self.0 == Self::SELF_CHECK_FAILED }
}

// ------------------------------------------------------------------------------------------------------ FFI (include/plume_hip.h)
#[repr(C)]
pub struct plume_ctx { _private: [u8; 0] }

pub const PLUME_STATUS_C_NOT_CANONICAL: u8 = 1;
pub const PLUME_STATUS_BAD_SCALAR: u8 = 2;
pub const PLUME_STATUS_IDENTITY: u8 = 4;
pub const PLUME_STATUS_SELFCHECK_FAILED: u8 = 8;
pub const PLUME_STATUS_BAD_TX: u8 = 16;
pub const PLUME_STATUS_HD_NO_KEY: u8 = 32;
pub const PLUME_STATUS_HD_HARDENED: u8 = 64;
pub const PLUME_HD_MAX_DEPTH: usize = 8;
pub const PLUME_STATUS_KDF_BAD_INPUT: u8 = 128;
pub const PLUME_KDF_BIP39: c_int = 1;
pub const PLUME_KDF_SHARED_SALT: c_int = 2;
pub const PLUME_KDF_MAX_SALT: usize = 256;
pub const PLUME_KDF_MAX_ITERATIONS: u32 = 1 << 24;
pub const PLUME_RECOVER_MISMATCH: u8 = 0;
pub const PLUME_RECOVER_MATCH: u8 = 1;
pub const PLUME_RECOVER_INVALID: u8 = 3;
pub const PLUME_RECOVER_FMT_AFFINE64: c_int = 0;
pub const PLUME_RECOVER_FMT_SEC1: c_int = 1;
pub const PLUME_RECOVER_FMT_REGISTERS: c_int = 2;
pub const PLUME_ETH_MISMATCH: u8 = 0;
pub const PLUME_ETH_MATCH: u8 = 1;
pub const PLUME_ETH_INVALID: u8 = 3;
pub const PLUME_ETH_PK_AFFINE64: c_int = 0;
pub const PLUME_ETH_PK_SEC1: c_int = 1;
pub const PLUME_ETH_ADDR_RAW20: c_int = 0;
pub const PLUME_ETH_ADDR_RECORD64: c_int = 1;
pub const PLUME_ETH_ADDR_EIP55: c_int = 2;
pub const PLUME_ECDSA_MISMATCH: u8 = 0;
pub const PLUME_ECDSA_MATCH: u8 = 1;
pub const PLUME_ECDSA_INVALID: u8 = 3;
/// `plume_ecdsa_sign_batch`: flag bit 0, `v` is 27 or 28; `plume_eth_message_hash_batch`: what is hashed
pub const PLUME_ECDSA_SIGN_V27: c_int = 1;
pub const PLUME_ETH_HASH_KECCAK256: c_int = 0;
pub const PLUME_ETH_HASH_EIP191: c_int = 1;
pub const PLUME_ECDSA_LOW_S: c_int = 1;
/// `plume_eth_tx_parse_batch`: the status of an item
pub const PLUME_ETH_TX_OK: u8 = 1;
pub const PLUME_ETH_TX_INVALID: u8 = 3;
/// `plume_merkle_*`: leaf formats, the sort flag, the status of an item, the proof length of a refused index
pub const PLUME_MERKLE_LEAF_HASH32: c_int = 0;
pub const PLUME_MERKLE_LEAF_ADDRESS: c_int = 1;
pub const PLUME_MERKLE_LEAF_ADDRESS_UINT256: c_int = 2;
pub const PLUME_MERKLE_SORT_LEAVES: c_int = 1;
pub const PLUME_MERKLE_MISMATCH: u8 = 0;
pub const PLUME_MERKLE_MATCH: u8 = 1;
pub const PLUME_MERKLE_INVALID: u8 = 3;
pub const PLUME_MERKLE_BAD_PROOF: u8 = 255;

#[link(name = "plume_hip")]
extern "C" {
    fn plume_init(out: *mut *mut plume_ctx, device_id: c_int) -> c_int;
    fn plume_init_multi(out: *mut *mut plume_ctx, device_ids: *const c_int, n_devices: c_int) -> c_int;
    fn plume_num_shards(ctx: *const plume_ctx) -> c_int;
    fn plume_destroy(ctx: *mut plume_ctx);
    fn plume_last_error() -> *const c_char;
    fn plume_host_register(p: *mut c_void, bytes: usize) -> c_int;
    fn plume_host_unregister(p: *mut c_void) -> c_int;
    fn plume_verify_batch(ctx: *mut plume_ctx, version: c_int, n: usize, msgs: *const u8, msg_off: *const u64,
        pk: *const u8, nullifier: *const u8, c: *const u8, s: *const u8, r_point: *const u8, hashed_to_curve_r: *const u8, ok: *mut u8) -> c_int;
    fn plume_verify_batch_sec1(ctx: *mut plume_ctx, version: c_int, n: usize, msgs: *const u8, msg_off: *const u64,
        pk33: *const u8, nullifier33: *const u8, c: *const u8, s: *const u8, r_point33: *const u8, hashed_to_curve_r33: *const u8, ok: *mut u8) -> c_int;
    fn plume_sign_batch(ctx: *mut plume_ctx, version: c_int, n: usize, msgs: *const u8, msg_off: *const u64, sk: *const u8, r: *const u8, pk_in: *const u8,
        pk: *mut u8, nullifier: *mut u8, c: *mut u8, s: *mut u8, r_point: *mut u8, hashed_to_curve_r: *mut u8, status: *mut u8) -> c_int;
    fn plume_scalars_to_sec1_der_batch(ctx: *mut plume_ctx, n: usize, scalars: *const u8, der109: *mut u8, status: *mut u8) -> c_int;
    fn plume_sec1_der_to_scalars_checked(ctx: *mut plume_ctx, n: usize, der109: *const u8, scalars: *mut u8, ok: *mut u8) -> c_int;
    fn plume_h2c_hints_batch(ctx: *mut plume_ctx, n: usize, msgs: *const u8, msg_off: *const u64, pk: *const u8, registers: c_int, hints: *mut u8) -> c_int;
    fn plume_set_sub_batches(ctx: *mut plume_ctx, sub_batches: c_int) -> c_int;
    fn plume_set_in_flight(ctx: *mut plume_ctx, batches: c_int) -> c_int;
    fn plume_set_sign_uniform(ctx: *mut plume_ctx, level: c_int) -> c_int;
    fn plume_get_sign_uniform(ctx: *const plume_ctx) -> c_int;
    fn plume_set_sign_selfcheck(ctx: *mut plume_ctx, mode: c_int) -> c_int;
    fn plume_get_sign_selfcheck(ctx: *const plume_ctx) -> c_int;
    fn plume_set_host_lanes(ctx: *mut plume_ctx, lanes: c_int) -> c_int;
    fn plume_set_stage_timing(ctx: *mut plume_ctx, on: c_int) -> c_int;
    fn plume_set_eq1_short(ctx: *mut plume_ctx, mode: c_int) -> c_int;
    fn plume_get_eq1_short(ctx: *const plume_ctx, min_items: *mut usize) -> c_int;
    fn plume_last_msm_kernel(ctx: *const plume_ctx) -> *const c_char;
    fn plume_shard_numa_node(ctx: *const plume_ctx, shard: c_int) -> c_int;
    fn plume_aggregate_check(ctx: *mut plume_ctx, version: c_int, mode: c_int, n: usize, msgs: *const u8, msg_off: *const u64, pk: *const u8, nullifier: *const u8, c: *const u8,
                             s: *const u8, r_point: *const u8, hashed_to_curve_r: *const u8, seed: *const u8, hash_ok: *mut u8, result: *mut u8) -> c_int;
    fn plume_nullset_create(ctx: *mut plume_ctx, reserve_items: usize, set: *mut *mut c_void) -> c_int;
    fn plume_nullset_destroy(set: *mut c_void);
    fn plume_nullset_reserve(set: *mut c_void, items: usize) -> c_int;
    fn plume_nullset_clear(set: *mut c_void) -> c_int;
    fn plume_nullset_size(set: *mut c_void, size: *mut u64, capacity: *mut u64) -> c_int;
    fn plume_nullset_insert(set: *mut c_void, n: usize, nullifier: *const u8, live: *const u8, ids: *const u64, fresh: *mut u8, n_fresh: *mut u64) -> c_int;
    fn plume_nullset_contains(set: *mut c_void, n: usize, nullifier: *const u8, found: *mut u8) -> c_int;
    fn plume_nullset_export(set: *mut c_void, cap: usize, records: *mut u8, count: *mut u64) -> c_int;
    fn plume_nullset_insert_device(set: *mut c_void, n: usize, nullifier: *const u8, live: *const u8, ids: *const u64, fresh: *mut u8, n_fresh: *mut u64,
                                   stream: *mut c_void) -> c_int;
    fn plume_nullset_contains_device(set: *mut c_void, n: usize, nullifier: *const u8, found: *mut u8, stream: *mut c_void) -> c_int;
    fn plume_sign_batch_rfc6979(ctx: *mut plume_ctx, version: c_int, n: usize, msgs: *const u8, msg_off: *const u64, sk: *const u8, aux: *const u8, pk_in: *const u8,
        pk: *mut u8, nullifier: *mut u8, c: *mut u8, s: *mut u8, r_point: *mut u8, hashed_to_curve_r: *mut u8, status: *mut u8) -> c_int;
    fn plume_sign_batch_rfc6979_device(ctx: *mut plume_ctx, version: c_int, n: usize, msgs: *const u8, msg_off: *const u64, msgs_bytes: usize, sk: *const u8, aux: *const u8,
        pk_in: *const u8, pk: *mut u8, nullifier: *mut u8, c: *mut u8, s: *mut u8, r_point: *mut u8, hashed_to_curve_r: *mut u8, status: *mut u8, stream: *mut c_void) -> c_int;
    fn plume_recover_batch(ctx: *mut plume_ctx, version: c_int, format: c_int, n: usize, msgs: *const u8, msg_off: *const u64, pk: *const u8, nullifier: *const u8,
        c: *const u8, s: *const u8, r_point: *mut u8, hashed_to_curve_r: *mut u8, hashed_to_curve: *mut u8, status: *mut u8) -> c_int;
    fn plume_recover_batch_device(ctx: *mut plume_ctx, version: c_int, format: c_int, n: usize, msgs: *const u8, msg_off: *const u64, msgs_bytes: usize, pk: *const u8,
        nullifier: *const u8, c: *const u8, s: *const u8, r_point: *mut u8, hashed_to_curve_r: *mut u8, hashed_to_curve: *mut u8, status: *mut u8,
        stream: *mut c_void) -> c_int;
    fn plume_eth_address_batch(ctx: *mut plume_ctx, pk_format: c_int, addr_format: c_int, n: usize, pk: *const u8, expect: *const u8, address: *mut u8,
        status: *mut u8) -> c_int;
    fn plume_eth_address_batch_device(ctx: *mut plume_ctx, pk_format: c_int, addr_format: c_int, n: usize, pk: *const u8, expect: *const u8, address: *mut u8,
        status: *mut u8, stream: *mut c_void) -> c_int;
    fn plume_ecdsa_recover_batch(ctx: *mut plume_ctx, flags: c_int, pk_format: c_int, addr_format: c_int, n: usize, hash: *const u8, r: *const u8, s: *const u8, v: *const u8,
        expect: *const u8, pk: *mut u8, address: *mut u8, status: *mut u8) -> c_int;
    fn plume_ecdsa_recover_batch_device(ctx: *mut plume_ctx, flags: c_int, pk_format: c_int, addr_format: c_int, n: usize, hash: *const u8, r: *const u8, s: *const u8,
        v: *const u8, expect: *const u8, pk: *mut u8, address: *mut u8, status: *mut u8, stream: *mut c_void) -> c_int;
    fn plume_eth_message_hash_batch(ctx: *mut plume_ctx, mode: c_int, n: usize, msgs: *const u8, msg_off: *const u64, hash32: *mut u8) -> c_int;
    fn plume_eth_message_hash_batch_device(ctx: *mut plume_ctx, mode: c_int, n: usize, msgs: *const u8, msg_off: *const u64, msgs_bytes: usize, hash32: *mut u8,
        stream: *mut c_void) -> c_int;
    fn plume_ecdsa_sign_batch(ctx: *mut plume_ctx, flags: c_int, n: usize, hash: *const u8, sk: *const u8, aux: *const u8, r: *mut u8, s: *mut u8, v: *mut u8,
        status: *mut u8) -> c_int;
    fn plume_ecdsa_sign_batch_device(ctx: *mut plume_ctx, flags: c_int, n: usize, hash: *const u8, sk: *const u8, aux: *const u8, r: *mut u8, s: *mut u8, v: *mut u8,
        status: *mut u8, stream: *mut c_void) -> c_int;
    fn plume_eth_tx_parse_batch(ctx: *mut plume_ctx, n: usize, txs: *const u8, tx_off: *const u64, hash32: *mut u8, r: *mut u8, s: *mut u8, v: *mut u8, chain_id: *mut u64,
        tx_type: *mut u8, status: *mut u8) -> c_int;
    fn plume_eth_tx_parse_batch_device(ctx: *mut plume_ctx, n: usize, txs: *const u8, tx_off: *const u64, txs_bytes: usize, hash32: *mut u8, r: *mut u8, s: *mut u8, v: *mut u8,
        chain_id: *mut u64, tx_type: *mut u8, status: *mut u8, stream: *mut c_void) -> c_int;
    fn plume_eth_tx_sender_batch(ctx: *mut plume_ctx, flags: c_int, pk_format: c_int, addr_format: c_int, n: usize, txs: *const u8, tx_off: *const u64, expect: *const u8,
        pk: *mut u8, address: *mut u8, chain_id: *mut u64, tx_type: *mut u8, status: *mut u8) -> c_int;
    fn plume_eth_tx_sender_batch_device(ctx: *mut plume_ctx, flags: c_int, pk_format: c_int, addr_format: c_int, n: usize, txs: *const u8, tx_off: *const u64, txs_bytes: usize,
        expect: *const u8, pk: *mut u8, address: *mut u8, chain_id: *mut u64, tx_type: *mut u8, status: *mut u8, stream: *mut c_void) -> c_int;
    fn plume_merkle_max_proof_len(n: usize) -> usize;
    fn plume_merkle_leaf_batch(ctx: *mut plume_ctx, leaf_format: c_int, addr_format: c_int, n: usize, address: *const u8, amount: *const u8, leaf32: *mut u8,
        status: *mut u8) -> c_int;
    fn plume_merkle_leaf_batch_device(ctx: *mut plume_ctx, leaf_format: c_int, addr_format: c_int, n: usize, address: *const u8, amount: *const u8, leaf32: *mut u8,
        status: *mut u8, stream: *mut c_void) -> c_int;
    fn plume_merkle_tree_build(ctx: *mut plume_ctx, flags: c_int, n: usize, leaf32: *const u8, tree: *mut u8, leaf_pos: *mut u32) -> c_int;
    fn plume_merkle_tree_build_device(ctx: *mut plume_ctx, flags: c_int, n: usize, leaf32: *const u8, tree: *mut u8, leaf_pos: *mut u32, stream: *mut c_void) -> c_int;
    fn plume_merkle_proof_batch(ctx: *mut plume_ctx, n: usize, tree: *const u8, m: usize, pos: *const u32, depth: usize, proof: *mut u8, proof_len: *mut u8) -> c_int;
    fn plume_merkle_proof_batch_device(ctx: *mut plume_ctx, n: usize, tree: *const u8, m: usize, pos: *const u32, depth: usize, proof: *mut u8, proof_len: *mut u8,
        stream: *mut c_void) -> c_int;
    fn plume_merkle_verify_batch(ctx: *mut plume_ctx, leaf_format: c_int, addr_format: c_int, m: usize, address_or_leaf: *const u8, amount: *const u8, depth: usize,
        proof: *const u8, proof_len: *const u8, root32: *const u8, status: *mut u8) -> c_int;
    fn plume_merkle_verify_batch_device(ctx: *mut plume_ctx, leaf_format: c_int, addr_format: c_int, m: usize, address_or_leaf: *const u8, amount: *const u8, depth: usize,
        proof: *const u8, proof_len: *const u8, root32: *const u8, status: *mut u8, stream: *mut c_void) -> c_int;
    fn plume_eth_tx_sign_out_bytes(n: usize, txs_bytes: u64) -> usize;
    fn plume_eth_tx_sign_batch(ctx: *mut plume_ctx, flags: c_int, n: usize, txs: *const u8, tx_off: *const u64, sk: *const u8, aux: *const u8, out: *mut u8,
        out_len: *mut u32, hash32: *mut u8, r: *mut u8, s: *mut u8, v: *mut u8, chain_id: *mut u64, tx_type: *mut u8, status: *mut u8) -> c_int;
    fn plume_eth_tx_sign_batch_device(ctx: *mut plume_ctx, flags: c_int, n: usize, txs: *const u8, tx_off: *const u64, txs_bytes: usize, sk: *const u8, aux: *const u8,
        out: *mut u8, out_bytes: usize, out_len: *mut u32, hash32: *mut u8, r: *mut u8, s: *mut u8, v: *mut u8, chain_id: *mut u64, tx_type: *mut u8, status: *mut u8,
        stream: *mut c_void) -> c_int;
    fn plume_hd_master_batch(ctx: *mut plume_ctx, n: usize, seed: *const u8, seed_len: usize, sk32: *mut u8, chain32: *mut u8, status: *mut u8) -> c_int;
    fn plume_hd_master_batch_device(ctx: *mut plume_ctx, n: usize, seed: *const u8, seed_len: usize, sk32: *mut u8, chain32: *mut u8, status: *mut u8, stream: *mut c_void) -> c_int;
    fn plume_hd_derive_priv_batch(ctx: *mut plume_ctx, flags: c_int, pk_format: c_int, addr_format: c_int, n: usize, parent_sk32: *const u8, parent_chain32: *const u8,
        path: *const u32, depth: usize, child_sk32: *mut u8, child_chain32: *mut u8, child_pk: *mut u8, address: *mut u8, status: *mut u8) -> c_int;
    fn plume_hd_derive_priv_batch_device(ctx: *mut plume_ctx, flags: c_int, pk_format: c_int, addr_format: c_int, n: usize, parent_sk32: *const u8, parent_chain32: *const u8,
        path: *const u32, depth: usize, child_sk32: *mut u8, child_chain32: *mut u8, child_pk: *mut u8, address: *mut u8, status: *mut u8, stream: *mut c_void) -> c_int;
    fn plume_hd_derive_pub_batch(ctx: *mut plume_ctx, flags: c_int, pk_format: c_int, addr_format: c_int, n: usize, parent_pk: *const u8, parent_chain32: *const u8,
        path: *const u32, depth: usize, child_pk: *mut u8, child_chain32: *mut u8, address: *mut u8, status: *mut u8) -> c_int;
    fn plume_hd_derive_pub_batch_device(ctx: *mut plume_ctx, flags: c_int, pk_format: c_int, addr_format: c_int, n: usize, parent_pk: *const u8, parent_chain32: *const u8,
        path: *const u32, depth: usize, child_pk: *mut u8, child_chain32: *mut u8, address: *mut u8, status: *mut u8, stream: *mut c_void) -> c_int;
    fn plume_pbkdf2_sha512_batch(ctx: *mut plume_ctx, flags: c_int, n: usize, pw: *const u8, pw_off: *const u64, salt: *const u8, salt_len: usize, iterations: u32,
        dklen: usize, out: *mut u8, status: *mut u8) -> c_int;
    fn plume_pbkdf2_sha512_batch_device(ctx: *mut plume_ctx, flags: c_int, n: usize, pw: *const u8, pw_off: *const u64, pw_bytes: usize, salt: *const u8, salt_len: usize,
        iterations: u32, dklen: usize, out: *mut u8, status: *mut u8, stream: *mut c_void) -> c_int;
}

fn last_error() -> HipError { HipError(unsafe { std::ffi::CStr::from_ptr(plume_last_error()) }.to_string_lossy().into_owned()) }

/// One context (`plume_ctx`): a GPU, or several with the batch sharded by the library.  One caller thread at a time (plume_hip.h "Threading").
pub struct HipEngine(*mut plume_ctx);
unsafe impl Send for HipEngine {}
impl Drop for HipEngine { fn drop(&mut self) { unsafe { plume_destroy(self.0) } } }

/// SoA staging of a slice of signatures in the ABI's formats (64-byte affine points, all-zero = identity; 32-byte big-endian scalars)
struct Packed { msgs: Vec<u8>, off: Vec<u64>, pk: Vec<u8>, nul: Vec<u8>, c: Vec<u8>, s: Vec<u8>, rp: Vec<u8>, hr: Vec<u8>, v1: bool }

fn put_point(dst: &mut [u8], p: &AffinePoint) {
    let e = p.to_encoded_point(false);               // 04 || x || y, or 00 for the identity
    if let (Some(x), Some(y)) = (e.x(), e.y()) { dst[..32].copy_from_slice(x); dst[32..64].copy_from_slice(y); }
    // identity: the 64 bytes stay zero
}
fn hd_status(what: &str, st: u8) -> Result<(), HipError> {
    if st == PLUME_STATUS_HD_HARDENED { return Err(HipError(format!("{what}: a public key has no hardened children"))); }
    if st == PLUME_STATUS_HD_NO_KEY { return Err(HipError(format!("{what}: the path has no key"))); }
    if st != 0 { return Err(HipError(format!("{what}: the parent key is not valid (status {st})"))); }
    Ok(())
}
/// The indices of a BIP-32 path, "m/44'/60'/0'/0/3" or, relative to a node, "0/3": decimal components below 2^31, a trailing `'` or `h` adds 2^31 (hardened);
/// 1 .. `PLUME_HD_MAX_DEPTH` of them.  An error for "m", "m/", an empty component, anything that is no index, too many components.
pub fn parse_path(path: &str) -> Result<Vec<u32>, HipError> {
    let bad = || HipError(format!("parse_path: {path:?} is not a path of 1 .. {PLUME_HD_MAX_DEPTH} indices below 2^31"));
    let rest = if path == "m" { return Err(bad()); } else { path.strip_prefix("m/").unwrap_or(path) };
    let mut out = Vec::new();
    for c in rest.split('/') {
        let (num, hard) = match c.strip_suffix('\'').or_else(|| c.strip_suffix('h')) { Some(n) => (n, true), None => (c, false) };
        if num.is_empty() || num.len() > 10 || !num.bytes().all(|b| b.is_ascii_digit()) { return Err(bad()); }
        let v: u64 = num.parse().map_err(|_| bad())?;
        if v >= 1 << 31 || out.len() == PLUME_HD_MAX_DEPTH { return Err(bad()); }
        out.push(v as u32 + if hard { 1 << 31 } else { 0 });
    }
    Ok(out)
}
/// What an extended key string holds: `key` is `00 || sk` for an xprv, the 33 SEC1 bytes of `pk` for an xpub.
pub struct ExtendedKey { pub depth: u8, pub child_number: u32, pub chain: [u8; 32], pub key: [u8; 33] }
fn xkey_sha256(msg: &[u8]) -> [u8; 32] {          // host-side, for the four checksum bytes only
    const K: [u32; 64] = [
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74,
        0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d,
        0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e,
        0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5,
        0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2];
    let mut h: [u32; 8] = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19];
    let mut m = msg.to_vec();
    m.push(0x80);
    while m.len() % 64 != 56 { m.push(0); }
    m.extend_from_slice(&((msg.len() as u64) * 8).to_be_bytes());
    for blk in m.chunks(64) {
        let mut w = [0u32; 64];
        for i in 0..16 { w[i] = u32::from_be_bytes([blk[4 * i], blk[4 * i + 1], blk[4 * i + 2], blk[4 * i + 3]]); }
        for i in 16..64 {
            let (a, b) = (w[i - 15], w[i - 2]);
            w[i] = w[i - 16].wrapping_add(a.rotate_right(7) ^ a.rotate_right(18) ^ (a >> 3)).wrapping_add(w[i - 7]).wrapping_add(b.rotate_right(17) ^ b.rotate_right(19) ^ (b >> 10));
        }
        let mut v = h;
        for i in 0..64 {
            let t1 = v[7].wrapping_add(v[4].rotate_right(6) ^ v[4].rotate_right(11) ^ v[4].rotate_right(25)).wrapping_add((v[4] & v[5]) ^ (!v[4] & v[6])).wrapping_add(K[i]).wrapping_add(w[i]);
            let t2 = (v[0].rotate_right(2) ^ v[0].rotate_right(13) ^ v[0].rotate_right(22)).wrapping_add((v[0] & v[1]) ^ (v[0] & v[2]) ^ (v[1] & v[2]));
            v = [t1.wrapping_add(t2), v[0], v[1], v[2], v[3].wrapping_add(t1), v[4], v[5], v[6]];
        }
        for i in 0..8 { h[i] = h[i].wrapping_add(v[i]); }
    }
    let mut out = [0u8; 32];
    for i in 0..8 { out[4 * i..4 * i + 4].copy_from_slice(&h[i].to_be_bytes()); }
    out
}
fn parse_xkey(s: &str, version: [u8; 4]) -> Result<ExtendedKey, HipError> {
    const DIGITS: &[u8] = b"123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz";
    let bad = |why: &str| HipError(format!("extended key: {why}"));
    let mut raw = [0u8; 82];
    for ch in s.bytes() {
        let mut carry = DIGITS.iter().position(|d| *d == ch).ok_or_else(|| bad("not a base58 digit"))? as u32;
        for b in raw.iter_mut().rev() { carry += 58 * *b as u32; *b = carry as u8; carry >>= 8; }
        if carry != 0 { return Err(bad("longer than 82 bytes")); }
    }
    if xkey_sha256(&xkey_sha256(&raw[..78]))[..4] != raw[78..] { return Err(bad("checksum")); }
    if raw[..4] != version { return Err(bad("version bytes")); }
    let (mut chain, mut key) = ([0u8; 32], [0u8; 33]);
    chain.copy_from_slice(&raw[13..45]);
    key.copy_from_slice(&raw[45..78]);
    Ok(ExtendedKey { depth: raw[4], child_number: u32::from_be_bytes([raw[9], raw[10], raw[11], raw[12]]), chain, key })
}
/// A mainnet "xprv..." string, base58check DECODE only: `hd_derive(&key[1..], &chain, path)` takes it from there.
pub fn parse_xprv(s: &str) -> Result<ExtendedKey, HipError> {
    let k = parse_xkey(s, [0x04, 0x88, 0xAD, 0xE4])?;
    if k.key[0] != 0 { return Err(HipError("parse_xprv: the key is not 00 || 32 bytes".to_string())); }
    Ok(k)
}
/// A mainnet "xpub..." string, base58check DECODE only.
pub fn parse_xpub(s: &str) -> Result<ExtendedKey, HipError> {
    let k = parse_xkey(s, [0x04, 0x88, 0xB2, 0x1E])?;
    if k.key[0] != 2 && k.key[0] != 3 { return Err(HipError("parse_xpub: the key is not a compressed point".to_string())); }
    Ok(k)
}
fn get_point(src: &[u8]) -> AffinePoint {
    if src[..64].iter().all(|b| *b == 0) { return AffinePoint::IDENTITY; }
    let e = EncodedPoint::from_affine_coordinates(FieldBytes::from_slice(&src[..32]), FieldBytes::from_slice(&src[32..64]), false);
    Option::from(AffinePoint::from_encoded_point(&e)).expect("the library only emits curve points")
}
fn get_scalar(src: &[u8]) -> Option<NonZeroScalar> { Option::from(NonZeroScalar::from_repr(*FieldBytes::from_slice(&src[..32]))) }

fn pack(sigs: &[PlumeSignature]) -> Packed {
    let n = sigs.len();
    let v1 = sigs.first().map_or(false, |s| s.v1specific.is_some());
    let mut p = Packed { msgs: Vec::new(), off: Vec::with_capacity(n + 1), pk: vec![0; 64 * n], nul: vec![0; 64 * n], c: vec![0; 32 * n], s: vec![0; 32 * n],
                         rp: vec![0; if v1 { 64 * n } else { 0 }], hr: vec![0; if v1 { 64 * n } else { 0 }], v1 };
    p.off.push(0);
    for (i, sig) in sigs.iter().enumerate() {
        assert_eq!(sig.v1specific.is_some(), v1, "a batch is all V1 or all V2");
        p.msgs.extend_from_slice(&sig.message);
        p.off.push(p.msgs.len() as u64);
        put_point(&mut p.pk[64 * i..], &sig.pk);
        put_point(&mut p.nul[64 * i..], &sig.nullifier);
        p.c[32 * i..32 * i + 32].copy_from_slice(&sig.c.to_bytes());
        p.s[32 * i..32 * i + 32].copy_from_slice(&sig.s.to_bytes());
        if let Some(v) = &sig.v1specific { put_point(&mut p.rp[64 * i..], &v.r_point); put_point(&mut p.hr[64 * i..], &v.hashed_to_curve_r); }
    }
    p.msgs.push(0); // keeps the pointer non-null for n = 0 / empty messages
    p
}

impl HipEngine {
    /// `plume_init`: one GPU
    pub fn new(device: i32) -> Result<Self, HipError> {
        let mut p = std::ptr::null_mut();
        match unsafe { plume_init(&mut p, device) } { 0 => Ok(Self(p)), _ => Err(last_error()) }
    }
    /// `plume_init_multi`: the host-pointer calls split every batch evenly and contiguously over `devices` (one worker thread, streams and staging
    /// buffers per device inside the library; results land in disjoint slices; no collective)
    pub fn new_multi(devices: &[i32]) -> Result<Self, HipError> {
        let mut p = std::ptr::null_mut();
        match unsafe { plume_init_multi(&mut p, devices.as_ptr(), devices.len() as c_int) } { 0 => Ok(Self(p)), _ => Err(last_error()) }
    }
    pub fn num_shards(&self) -> usize { unsafe { plume_num_shards(self.0) as usize } }

    /// Batch twin of `PlumeSignature::verify` (rust-k256/src/lib.rs:93-145): `result[i] == sigs[i].verify()`.  All V1 or all V2.
    pub fn verify_batch(&self, sigs: &[PlumeSignature]) -> Result<Vec<bool>, HipError> {
        let p = pack(sigs);
        let mut ok = vec![0u8; sigs.len()];
        let null = std::ptr::null();
        let rc = unsafe { plume_verify_batch(self.0, if p.v1 { 1 } else { 2 }, sigs.len(), p.msgs.as_ptr(), p.off.as_ptr(), p.pk.as_ptr(), p.nul.as_ptr(), p.c.as_ptr(),
                                             p.s.as_ptr(), if p.v1 { p.rp.as_ptr() } else { null }, if p.v1 { p.hr.as_ptr() } else { null }, ok.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        Ok(ok.into_iter().map(|b| b == 1).collect())
    }

    /// What a V2 signature leaves out (`plume_recover_batch`): `r_point = s G - c pk` and `hashed_to_curve_r = s H - c nullifier`, recomputed on the GPU as
    /// `check_ec_equations` recomputes them (circuits/circom/verify_nullifier.circom:140-222), with `H = hash_to_curve(msg, pk)` and whether `c` is the hash
    /// of them that `v1` asks for (the six-encoding hash, or V2's three).  `result[i]` is `None` where the library rejects the item's inputs -- which the
    /// types here cannot express, so only for an identity nullifier the library accepts and `Some` carries.  The signatures' own `v1specific` is ignored.
    pub fn recover_batch(&self, sigs: &[PlumeSignature], v1: bool) -> Result<Vec<Option<(PlumeSignatureV1Fields, AffinePoint, bool)>>, HipError> {
        let n = sigs.len();
        let stripped: Vec<PlumeSignature> = sigs.iter().map(|s| PlumeSignature { v1specific: None, ..s.clone() }).collect();
        let p = pack(&stripped);
        let (mut rp, mut hr, mut h, mut status) = (vec![0u8; 64 * n], vec![0u8; 64 * n], vec![0u8; 64 * n], vec![0u8; n]);
        let rc = unsafe { plume_recover_batch(self.0, if v1 { 1 } else { 2 }, PLUME_RECOVER_FMT_AFFINE64, n, p.msgs.as_ptr(), p.off.as_ptr(), p.pk.as_ptr(), p.nul.as_ptr(),
                                              p.c.as_ptr(), p.s.as_ptr(), rp.as_mut_ptr(), hr.as_mut_ptr(), h.as_mut_ptr(), status.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        Ok((0..n).map(|i| if status[i] == PLUME_RECOVER_INVALID { None } else {
            Some((PlumeSignatureV1Fields { r_point: get_point(&rp[64 * i..]), hashed_to_curve_r: get_point(&hr[64 * i..]) }, get_point(&h[64 * i..]), status[i] == PLUME_RECOVER_MATCH))
        }).collect())
    }

    /// The Ethereum address of every public key, `Keccak-256(x || y)[12..32)` (`plume_eth_address_batch`): `result[i]` is `None` for a key that is no non-identity curve
    /// point -- the identity, which `verify` accepts, has no address -- and otherwise the 20 bytes and, when `expect` is given, whether they equal `expect[i]`
    /// (`true` without `expect`).
    pub fn eth_address_batch(&self, pks: &[AffinePoint], expect: Option<&[[u8; 20]]>) -> Result<Vec<Option<([u8; 20], bool)>>, HipError> {
        let n = pks.len();
        if let Some(e) = expect { if e.len() != n { return Err(HipError("eth_address_batch: expect must hold one address per key".to_string())); } }
        let mut pk = vec![0u8; 64 * n];
        for (i, p) in pks.iter().enumerate() { put_point(&mut pk[64 * i..64 * i + 64], p); }
        let want: Vec<u8> = expect.map(|e| e.concat()).unwrap_or_default();
        let (mut addr, mut status) = (vec![0u8; 20 * n], vec![0u8; n]);
        let rc = unsafe { plume_eth_address_batch(self.0, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, n, pk.as_ptr(), if expect.is_some() { want.as_ptr() } else { std::ptr::null() },
                                                  addr.as_mut_ptr(), status.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        Ok((0..n).map(|i| if status[i] == PLUME_ETH_INVALID { None } else {
            let mut a = [0u8; 20];
            a.copy_from_slice(&addr[20 * i..20 * i + 20]);
            Some((a, status[i] == PLUME_ETH_MATCH))
        }).collect())
    }

    /// The addresses as `"0x"` + 40 hex digits with the EIP-55 mixed-case checksum, computed on the GPU as well; `None` as in `eth_address_batch`.
    pub fn eth_address_eip55_batch(&self, pks: &[AffinePoint]) -> Result<Vec<Option<String>>, HipError> {
        let n = pks.len();
        let mut pk = vec![0u8; 64 * n];
        for (i, p) in pks.iter().enumerate() { put_point(&mut pk[64 * i..64 * i + 64], p); }
        let (mut addr, mut status) = (vec![0u8; 42 * n], vec![0u8; n]);
        let rc = unsafe { plume_eth_address_batch(self.0, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_EIP55, n, pk.as_ptr(), std::ptr::null(), addr.as_mut_ptr(), status.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        Ok((0..n).map(|i| if status[i] == PLUME_ETH_INVALID { None } else { Some(String::from_utf8_lossy(&addr[42 * i..42 * i + 42]).into_owned()) }).collect())
    }

    /// The public key and the Ethereum address behind one ECDSA signature over a 32-byte digest (`plume_ecdsa_recover_batch`, Ethereum's `ecrecover`): `v` is 0, 1, 27 or
    /// 28.  An error when the library rejects the item: `v`, `r` or `s` out of range, no curve point with x = `r`, or a key that comes out as the identity.
    pub fn ecdsa_recover(&self, hash32: &[u8; 32], r: &[u8; 32], s: &[u8; 32], v: u8) -> Result<(AffinePoint, [u8; 20]), HipError> {
        let (mut pk, mut addr, mut status) = ([0u8; 64], [0u8; 20], [0u8; 1]);
        let vs = [v];
        let rc = unsafe { plume_ecdsa_recover_batch(self.0, 0, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, 1, hash32.as_ptr(), r.as_ptr(), s.as_ptr(), vs.as_ptr(), std::ptr::null(),
                                                    pk.as_mut_ptr(), addr.as_mut_ptr(), status.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        if status[0] == PLUME_ECDSA_INVALID { return Err(HipError("ecdsa_recover: the signature recovers no public key".to_string())); }
        Ok((get_point(&pk), addr))
    }
    /// `ecdsa_recover` for callers that want the 20 address bytes only.
    pub fn ecdsa_recover_address(&self, hash32: &[u8; 32], r: &[u8; 32], s: &[u8; 32], v: u8) -> Result<[u8; 20], HipError> {
        let (mut addr, mut status) = ([0u8; 20], [0u8; 1]);
        let vs = [v];
        let rc = unsafe { plume_ecdsa_recover_batch(self.0, 0, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, 1, hash32.as_ptr(), r.as_ptr(), s.as_ptr(), vs.as_ptr(), std::ptr::null(),
                                                    std::ptr::null_mut(), addr.as_mut_ptr(), status.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        if status[0] == PLUME_ECDSA_INVALID { return Err(HipError("ecdsa_recover_address: the signature recovers no public key".to_string())); }
        Ok(addr)
    }

    /// A deterministic ECDSA signature `(r, s, v)` by `sk` (32 big-endian bytes) over a 32-byte digest (`plume_ecdsa_sign_batch`): the RFC 6979 nonce over the digest
    /// itself, byte-identical to geth, ethers and libsecp256k1, hedged with `aux` when given; always low `s`; `v` is 0 / 1, or 27 / 28 with `v27`.  An error when `sk` is
    /// outside [1, n - 1], the outcome is degenerate, or the self-check withheld the signature.
    pub fn ecdsa_sign(&self, sk: &[u8; 32], hash32: &[u8; 32], aux: Option<&[u8; 32]>, v27: bool) -> Result<([u8; 32], [u8; 32], u8), HipError> {
        let (mut r, mut s, mut v, mut status) = ([0u8; 32], [0u8; 32], [0u8; 1], [0u8; 1]);
        let rc = unsafe { plume_ecdsa_sign_batch(self.0, if v27 { PLUME_ECDSA_SIGN_V27 } else { 0 }, 1, hash32.as_ptr(), sk.as_ptr(), aux.map_or(std::ptr::null(), |a| a.as_ptr()),
                                                 r.as_mut_ptr(), s.as_mut_ptr(), v.as_mut_ptr(), status.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        if status[0] != 0 { return Err(HipError(format!("ecdsa_sign: no signature (status {})", status[0]))); }
        Ok((r, s, v[0]))
    }
    /// The EIP-191 digest of `msg`, Keccak-256("\x19Ethereum Signed Message:\n" || decimal(len) || msg) (`plume_eth_message_hash_batch`).
    pub fn eth_message_hash(&self, msg: &[u8]) -> Result<[u8; 32], HipError> {
        let off = [0u64, msg.len() as u64];
        let mut h = [0u8; 32];
        let rc = unsafe { plume_eth_message_hash_batch(self.0, PLUME_ETH_HASH_EIP191, 1, msg.as_ptr(), off.as_ptr(), h.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        Ok(h)
    }
    /// A wallet's `personal_sign`: the 65 bytes `r || s || v` (`v` = 27 / 28) of `ecdsa_sign` over the EIP-191 digest of `msg`.
    pub fn personal_sign(&self, sk: &[u8; 32], msg: &[u8], aux: Option<&[u8; 32]>) -> Result<[u8; 65], HipError> {
        let (r, s, v) = self.ecdsa_sign(sk, &self.eth_message_hash(msg)?, aux, true)?;
        let mut out = [0u8; 65];
        out[..32].copy_from_slice(&r); out[32..64].copy_from_slice(&s); out[64] = v;
        Ok(out)
    }
    /// The public key and the address that `personal_sign`ed `msg`: the EIP-191 digest, then `ecdsa_recover`.
    pub fn personal_recover(&self, msg: &[u8], sig65: &[u8; 65]) -> Result<(AffinePoint, [u8; 20]), HipError> {
        let (mut r, mut s) = ([0u8; 32], [0u8; 32]);
        r.copy_from_slice(&sig65[..32]); s.copy_from_slice(&sig65[32..64]);
        self.ecdsa_recover(&self.eth_message_hash(msg)?, &r, &s, sig65[64])
    }

    /// The 32 bytes the sender of one raw signed transaction signed (`plume_eth_tx_parse_batch`): legacy (unprotected or EIP-155) and the typed envelopes 01 - 04.  An
    /// error for an item that is no such transaction.  A sender recovery, not a consensus decoder: inner fields are not validated.
    pub fn tx_signing_hash(&self, raw: &[u8]) -> Result<[u8; 32], HipError> {
        let off = [0u64, raw.len() as u64];
        let (mut h, mut r, mut s, mut v, mut status) = ([0u8; 32], [0u8; 32], [0u8; 32], [0u8; 1], [0u8; 1]);
        let rc = unsafe { plume_eth_tx_parse_batch(self.0, 1, raw.as_ptr(), off.as_ptr(), h.as_mut_ptr(), r.as_mut_ptr(), s.as_mut_ptr(), v.as_mut_ptr(), std::ptr::null_mut(),
                                                   std::ptr::null_mut(), status.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        if status[0] != PLUME_ETH_TX_OK { return Err(HipError("tx_signing_hash: not a signed transaction of a known kind".to_string())); }
        Ok(h)
    }
    /// The signed raw transaction of one UNSIGNED serialization (`plume_eth_tx_sign_batch`): legacy with 6 items (unprotected) or 9 (EIP-155: chainId, then two empty
    /// strings), or a typed envelope 01 - 04 without its last three fields.  The signature is `ecdsa_sign`'s over Keccak-256 of `unsigned`, hedged with `aux` when
    /// given.  An error for an item that is no such payload (the error `tx_signing_hash` gives for a bad item), for a key outside [1, n - 1] or a degenerate outcome, and
    /// `HipError::self_check_failed()` when the self-check withheld the signature.
    pub fn sign_tx(&self, sk: &[u8; 32], unsigned: &[u8], aux: Option<&[u8; 32]>) -> Result<Vec<u8>, HipError> {
        let off = [0u64, unsigned.len() as u64];
        let mut out = vec![0u8; unsafe { plume_eth_tx_sign_out_bytes(1, unsigned.len() as u64) }];
        let (mut out_len, mut status) = ([0u32; 1], [0u8; 1]);
        let null = std::ptr::null_mut::<u8>();
        let rc = unsafe { plume_eth_tx_sign_batch(self.0, 0, 1, unsigned.as_ptr(), off.as_ptr(), sk.as_ptr(), aux.map_or(std::ptr::null(), |a| a.as_ptr()), out.as_mut_ptr(),
                                                  out_len.as_mut_ptr(), null, null, null, null, std::ptr::null_mut(), null, status.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        if status[0] & PLUME_STATUS_BAD_TX != 0 { return Err(HipError("sign_tx: not an unsigned transaction of a known kind".to_string())); }
        if status[0] & PLUME_STATUS_SELFCHECK_FAILED != 0 { return Err(HipError::self_check_failed()); }
        if status[0] != 0 { return Err(HipError(format!("sign_tx: no signature (status {})", status[0]))); }
        out.truncate(out_len[0] as usize);
        Ok(out)
    }
    /// PBKDF2-HMAC-SHA512(password, salt, iterations), the first `dklen` bytes (1 ..= 64), on the GPU (`plume_pbkdf2_sha512_batch`); a salt of at most
    /// `PLUME_KDF_MAX_SALT` bytes.  Over bytes: a caller with non-ASCII text normalises it (NFKD) first.
    pub fn pbkdf2_sha512(&self, password: &[u8], salt: &[u8], iterations: u32, dklen: usize) -> Result<Vec<u8>, HipError> {
        let off = [0u64, password.len() as u64];
        let (mut out, mut status) = (vec![0u8; dklen.max(1)], [0u8; 1]);
        let rc = unsafe { plume_pbkdf2_sha512_batch(self.0, PLUME_KDF_SHARED_SALT, 1, password.as_ptr(), off.as_ptr(), salt.as_ptr(), salt.len(), iterations, dklen,
                                                    out.as_mut_ptr(), status.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        if status[0] != 0 { return Err(HipError(format!("pbkdf2_sha512: not derived (status {})", status[0]))); }
        Ok(out)
    }
    /// The 64-byte BIP-39 seed of a mnemonic sentence, on the GPU: PBKDF2-HMAC-SHA512(sentence, "mnemonic" || passphrase, 2048).  Over bytes: a caller with non-ASCII
    /// text normalises it (NFKD) first.  The word list is out of scope: the sentence is not checked against it.
    pub fn mnemonic_to_seed(&self, mnemonic: &[u8], passphrase: &[u8]) -> Result<[u8; 64], HipError> {
        let off = [0u64, mnemonic.len() as u64];
        let (mut seed, mut status) = ([0u8; 64], [0u8; 1]);
        let rc = unsafe { plume_pbkdf2_sha512_batch(self.0, PLUME_KDF_BIP39 | PLUME_KDF_SHARED_SALT, 1, mnemonic.as_ptr(), off.as_ptr(), passphrase.as_ptr(), passphrase.len(), 2048,
                                                    64, seed.as_mut_ptr(), status.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        if status[0] != 0 { return Err(HipError(format!("mnemonic_to_seed: not derived (status {})", status[0]))); }
        Ok(seed)
    }
    /// The BIP-32 master node `(sk, chain)` of a seed of 16 .. 64 bytes (`plume_hd_master_batch`): HMAC-SHA512("Bitcoin seed", seed), on the GPU.
    pub fn hd_master(&self, seed: &[u8]) -> Result<([u8; 32], [u8; 32]), HipError> {
        let (mut sk, mut chain, mut status) = ([0u8; 32], [0u8; 32], [0u8; 1]);
        let rc = unsafe { plume_hd_master_batch(self.0, 1, seed.as_ptr(), seed.len(), sk.as_mut_ptr(), chain.as_mut_ptr(), status.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        hd_status("hd_master", status[0])?;
        Ok((sk, chain))
    }
    /// The node `(sk, chain)` at `path` ("m/44'/60'/0'/0/3") below the node `(sk, chain)`: BIP-32's CKDpriv on the GPU (`plume_hd_derive_priv_batch`).
    pub fn hd_derive(&self, sk: &[u8; 32], chain: &[u8; 32], path: &str) -> Result<([u8; 32], [u8; 32]), HipError> {
        let idx = parse_path(path)?;
        let (mut csk, mut cchain, mut status) = ([0u8; 32], [0u8; 32], [0u8; 1]);
        let null = std::ptr::null_mut::<u8>();
        let rc = unsafe { plume_hd_derive_priv_batch(self.0, 0, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, 1, sk.as_ptr(), chain.as_ptr(), idx.as_ptr(), idx.len(), csk.as_mut_ptr(),
                                                     cchain.as_mut_ptr(), null, null, status.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        hd_status("hd_derive", status[0])?;
        Ok((csk, cchain))
    }
    /// The public node `(pk, chain)` at the non-hardened `path` ("0/3") below the public node `(pk, chain)`: BIP-32's CKDpub on the GPU (`plume_hd_derive_pub_batch`).
    pub fn hd_derive_pub(&self, pk: &AffinePoint, chain: &[u8; 32], path: &str) -> Result<(AffinePoint, [u8; 32]), HipError> {
        let idx = parse_path(path)?;
        let (mut par, mut cpk, mut cchain, mut status) = ([0u8; 64], [0u8; 64], [0u8; 32], [0u8; 1]);
        put_point(&mut par, pk);
        let rc = unsafe { plume_hd_derive_pub_batch(self.0, 0, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, 1, par.as_ptr(), chain.as_ptr(), idx.as_ptr(), idx.len(), cpk.as_mut_ptr(),
                                                    cchain.as_mut_ptr(), std::ptr::null_mut(), status.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        hd_status("hd_derive_pub", status[0])?;
        Ok((get_point(&cpk), cchain))
    }
    /// The 20-byte Ethereum address of the key at `path` below a private node.
    pub fn hd_address(&self, sk: &[u8; 32], chain: &[u8; 32], path: &str) -> Result<[u8; 20], HipError> {
        let idx = parse_path(path)?;
        let (mut csk, mut addr, mut status) = ([0u8; 32], [0u8; 20], [0u8; 1]);
        let null = std::ptr::null_mut::<u8>();
        let rc = unsafe { plume_hd_derive_priv_batch(self.0, 0, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, 1, sk.as_ptr(), chain.as_ptr(), idx.as_ptr(), idx.len(), csk.as_mut_ptr(),
                                                     null, null, addr.as_mut_ptr(), status.as_mut_ptr()) };
        csk.iter_mut().for_each(|b| *b = 0);
        if rc != 0 { return Err(last_error()); }
        hd_status("hd_address", status[0])?;
        Ok(addr)
    }
    /// The 20-byte Ethereum address of the key at the non-hardened `path` below a public node: what a watcher holding an xpub derives.
    pub fn hd_address_pub(&self, pk: &AffinePoint, chain: &[u8; 32], path: &str) -> Result<[u8; 20], HipError> {
        let idx = parse_path(path)?;
        let (mut par, mut cpk, mut addr, mut status) = ([0u8; 64], [0u8; 64], [0u8; 20], [0u8; 1]);
        put_point(&mut par, pk);
        let rc = unsafe { plume_hd_derive_pub_batch(self.0, 0, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, 1, par.as_ptr(), chain.as_ptr(), idx.as_ptr(), idx.len(), cpk.as_mut_ptr(),
                                                    std::ptr::null_mut(), addr.as_mut_ptr(), status.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        hd_status("hd_address_pub", status[0])?;
        Ok(addr)
    }
    /// The public key and the address of the sender of one raw signed transaction (`plume_eth_tx_sender_batch`), with the EIP-2 low-`s` rule.  An error when there is no
    /// sender: the framing is broken or the signature recovers no key.
    pub fn tx_sender(&self, raw: &[u8]) -> Result<(AffinePoint, [u8; 20]), HipError> {
        let off = [0u64, raw.len() as u64];
        let (mut pk, mut addr, mut status) = ([0u8; 64], [0u8; 20], [0u8; 1]);
        let rc = unsafe { plume_eth_tx_sender_batch(self.0, PLUME_ECDSA_LOW_S, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, 1, raw.as_ptr(), off.as_ptr(), std::ptr::null(),
                                                    pk.as_mut_ptr(), addr.as_mut_ptr(), std::ptr::null_mut(), std::ptr::null_mut(), status.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        if status[0] == PLUME_ECDSA_INVALID { return Err(HipError("tx_sender: no sender".to_string())); }
        Ok((get_point(&pk), addr))
    }
    /// `tx_sender` for callers that want the 20 address bytes only.
    pub fn tx_sender_address(&self, raw: &[u8]) -> Result<[u8; 20], HipError> {
        let off = [0u64, raw.len() as u64];
        let (mut addr, mut status) = ([0u8; 20], [0u8; 1]);
        let rc = unsafe { plume_eth_tx_sender_batch(self.0, PLUME_ECDSA_LOW_S, PLUME_ETH_PK_AFFINE64, PLUME_ETH_ADDR_RAW20, 1, raw.as_ptr(), off.as_ptr(), std::ptr::null(),
                                                    std::ptr::null_mut(), addr.as_mut_ptr(), std::ptr::null_mut(), std::ptr::null_mut(), status.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        if status[0] == PLUME_ECDSA_INVALID { return Err(HipError("tx_sender_address: no sender".to_string())); }
        Ok(addr)
    }

    /// The leaf of one account in OpenZeppelin's `StandardMerkleTree` (`plume_merkle_leaf_batch`): `Keccak(Keccak(abi.encode(address)))`, or with an `amount` (32
    /// big-endian bytes) `Keccak(Keccak(abi.encode(address, amount)))`, the tree of `["address", "uint256"]`.
    pub fn merkle_leaf(&self, addr20: &[u8; 20], amount: Option<&[u8; 32]>) -> Result<[u8; 32], HipError> {
        let mut leaf = [0u8; 32];
        let fmt = if amount.is_some() { PLUME_MERKLE_LEAF_ADDRESS_UINT256 } else { PLUME_MERKLE_LEAF_ADDRESS };
        let rc = unsafe { plume_merkle_leaf_batch(self.0, fmt, PLUME_ETH_ADDR_RAW20, 1, addr20.as_ptr(), amount.map_or(std::ptr::null(), |a| a.as_ptr()), leaf.as_mut_ptr(),
                                                  std::ptr::null_mut()) };
        if rc != 0 { return Err(last_error()); }
        Ok(leaf)
    }
    /// The whole tree over 32-byte leaves (`plume_merkle_tree_build`): `(2n - 1) * 32` bytes, the root first, and the tree index of every input leaf.  `sort`: order
    /// the leaves by (hash, input index) first, as `StandardMerkleTree` does.
    pub fn merkle_tree(&self, leaves: &[[u8; 32]], sort: bool) -> Result<(Vec<u8>, Vec<u32>), HipError> {
        let n = leaves.len();
        let flat: Vec<u8> = leaves.iter().flatten().copied().collect();
        let (mut tree, mut pos) = (vec![0u8; if n == 0 { 0 } else { 32 * (2 * n - 1) }], vec![0u32; n]);
        let rc = unsafe { plume_merkle_tree_build(self.0, if sort { PLUME_MERKLE_SORT_LEAVES } else { 0 }, n, flat.as_ptr(), tree.as_mut_ptr(), pos.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        Ok((tree, pos))
    }
    /// The root of `merkle_tree`.
    pub fn merkle_root(&self, leaves: &[[u8; 32]], sort: bool) -> Result<[u8; 32], HipError> {
        let (tree, _) = self.merkle_tree(leaves, sort)?;
        let mut root = [0u8; 32];
        root.copy_from_slice(&tree[..32]);
        Ok(root)
    }
    /// The proof of input leaf `index`: the siblings on the way to the root, leaf side first (`plume_merkle_proof_batch`).
    pub fn merkle_proof(&self, leaves: &[[u8; 32]], index: usize, sort: bool) -> Result<Vec<[u8; 32]>, HipError> {
        if index >= leaves.len() { return Err(HipError("merkle_proof: index out of range".to_string())); }
        let (tree, pos) = self.merkle_tree(leaves, sort)?;
        let depth = unsafe { plume_merkle_max_proof_len(leaves.len()) };
        let (mut slots, mut len) = (vec![0u8; 32 * depth + 1], [0u8; 1]);
        let rc = unsafe { plume_merkle_proof_batch(self.0, leaves.len(), tree.as_ptr(), 1, pos[index..].as_ptr(), depth, slots.as_mut_ptr(), len.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        if len[0] == PLUME_MERKLE_BAD_PROOF { return Err(HipError("merkle_proof: no proof".to_string())); }
        Ok((0..len[0] as usize).map(|k| { let mut e = [0u8; 32]; e.copy_from_slice(&slots[32 * k..32 * k + 32]); e }).collect())
    }
    fn merkle_verify_item(&self, fmt: c_int, item: &[u8], amount: Option<&[u8; 32]>, proof: &[[u8; 32]], root32: &[u8; 32]) -> Result<bool, HipError> {
        if proof.len() > 64 { return Ok(false); }
        let mut slots: Vec<u8> = proof.iter().flatten().copied().collect();
        slots.push(0);                                   // keeps the pointer non-null for an empty proof
        let (len, mut status) = ([proof.len() as u8], [0u8; 1]);
        let rc = unsafe { plume_merkle_verify_batch(self.0, fmt, PLUME_ETH_ADDR_RAW20, 1, item.as_ptr(), amount.map_or(std::ptr::null(), |a| a.as_ptr()), proof.len(),
                                                    slots.as_ptr(), len.as_ptr(), root32.as_ptr(), status.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        Ok(status[0] == PLUME_MERKLE_MATCH)
    }
    /// `MerkleProof.verify` of a 32-byte leaf (`plume_merkle_verify_batch`).
    pub fn merkle_verify(&self, leaf: &[u8; 32], proof: &[[u8; 32]], root32: &[u8; 32]) -> Result<bool, HipError> {
        self.merkle_verify_item(PLUME_MERKLE_LEAF_HASH32, leaf, None, proof, root32)
    }
    /// `merkle_verify` of an address: its leaf (with `amount`, the leaf of `["address", "uint256"]`) is computed in the same kernel.
    pub fn merkle_verify_address(&self, addr20: &[u8; 20], amount: Option<&[u8; 32]>, proof: &[[u8; 32]], root32: &[u8; 32]) -> Result<bool, HipError> {
        self.merkle_verify_item(if amount.is_some() { PLUME_MERKLE_LEAF_ADDRESS_UINT256 } else { PLUME_MERKLE_LEAF_ADDRESS }, addr20, amount, proof, root32)
    }

    /// Aggregate pre-filter (no reference counterpart; include/plume_hip.h `plume_aggregate_check`): `Ok(true)` iff every V1 signature of the batch would
    /// `verify()` — up to a false-accept probability of 2^-126 over `seed`, which must be 32 fresh random bytes the signers could not predict.  All-or-nothing:
    /// on `Ok(false)` call `verify_batch` to find the culprits.  Per item the challenge hash is checked exactly; the two group equations (lib.rs:101,109,117,122)
    /// only in one random linear combination (a single 5n-point multi-scalar multiplication on the GPU).
    /// `seed = None` lets the library draw the 32 bytes from the OS generator (prefer it over anything constant, reused or known to the signers).
    pub fn aggregate_check_v1(&self, sigs: &[PlumeSignature], seed: Option<&[u8; 32]>) -> Result<bool, HipError> {
        let p = pack(sigs);
        assert!(p.v1 || sigs.is_empty(), "the aggregate check needs the V1 fields r_point / hashed_to_curve_r");
        let mut rec = [0u8; 72];
        let rc = unsafe { plume_aggregate_check(self.0, 1, 0, sigs.len(), p.msgs.as_ptr(), p.off.as_ptr(), p.pk.as_ptr(), p.nul.as_ptr(), p.c.as_ptr(), p.s.as_ptr(),
                                                p.rp.as_ptr(), p.hr.as_ptr(), seed.map_or(std::ptr::null(), |s| s.as_ptr()), std::ptr::null_mut(), rec.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        Ok(rec[0] == 1)
    }

    /// The wire format of the serde / wasm layer (javascript/src/lib.rs:95-118,147-184): points as 33-byte SEC1-compressed records, decompressed and
    /// validated on the GPU; a record that would fail `AffinePoint::from_encoded_point` gives `false`.  Arrays are `n` records each.
    #[allow(clippy::too_many_arguments)]
    pub fn verify_batch_sec1(&self, v1: bool, msgs: &[&[u8]], pk33: &[u8], nullifier33: &[u8], c: &[u8], s: &[u8], r_point33: &[u8], hashed_to_curve_r33: &[u8])
        -> Result<Vec<bool>, HipError> {
        let n = msgs.len();
        // the library reads 33 n / 32 n bytes through these pointers: a short slice must never reach it (this is a safe fn)
        let lens_ok = pk33.len() == 33 * n && nullifier33.len() == 33 * n && c.len() == 32 * n && s.len() == 32 * n
            && (!v1 || (r_point33.len() == 33 * n && hashed_to_curve_r33.len() == 33 * n));
        if !lens_ok { return Err(HipError(format!("verify_batch_sec1: array lengths do not match {n} items (33 n bytes per point array, 32 n per scalar array)"))); }
        let (mut buf, mut off) = (Vec::new(), vec![0u64]);
        for m in msgs { buf.extend_from_slice(m); off.push(buf.len() as u64); }
        buf.push(0);
        let mut ok = vec![0u8; n];
        let null = std::ptr::null();
        let rc = unsafe { plume_verify_batch_sec1(self.0, if v1 { 1 } else { 2 }, n, buf.as_ptr(), off.as_ptr(), pk33.as_ptr(), nullifier33.as_ptr(), c.as_ptr(), s.as_ptr(),
                                                  if v1 { r_point33.as_ptr() } else { null }, if v1 { hashed_to_curve_r33.as_ptr() } else { null }, ok.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        Ok(ok.into_iter().map(|b| b == 1).collect())
    }

    /// Batch twin of `PlumeSigner::new(&keys[i], v1).try_sign_with_rng(rng, msgs[i])` (randomizedsigner.rs:43-112).  The nonces are drawn on the host
    /// exactly as the reference draws them — `SecretKey::random(rng)`, one per item, in item order (randomizedsigner.rs:49) — and wiped after the call;
    /// an item on which the reference would panic comes back as `Err(SignError)` instead of unwinding.
    pub fn sign_batch(&self, keys: &[SecretKey], msgs: &[&[u8]], v1: bool, rng: &mut impl CryptoRngCore)
        -> Result<Vec<Result<PlumeSignature, SignError>>, HipError> {
        let nonces: Vec<SecretKey> = keys.iter().map(|_| SecretKey::random(rng)).collect();
        self.sign_batch_with_nonces(keys, msgs, v1, &nonces)
    }

    /// Same with the nonces supplied (the mock RNG of rust-k256/tests/signing.rs:23-44; `plume_arkworks::sign_with_r`).
    pub fn sign_batch_with_nonces(&self, keys: &[SecretKey], msgs: &[&[u8]], v1: bool, nonces: &[SecretKey])
        -> Result<Vec<Result<PlumeSignature, SignError>>, HipError> {
        let n = keys.len();
        assert!(msgs.len() == n && nonces.len() == n);
        let (mut buf, mut off) = (Vec::new(), vec![0u64]);
        for m in msgs { buf.extend_from_slice(m); off.push(buf.len() as u64); }
        buf.push(0);
        let (mut sk, mut r) = (vec![0u8; 32 * n], vec![0u8; 32 * n]);
        for i in 0..n { sk[32 * i..32 * i + 32].copy_from_slice(&keys[i].to_bytes()); r[32 * i..32 * i + 32].copy_from_slice(&nonces[i].to_bytes()); }
        let (mut pk, mut nul, mut rp, mut hr) = (vec![0u8; 64 * n], vec![0u8; 64 * n], vec![0u8; 64 * n], vec![0u8; 64 * n]);
        let (mut c, mut s, mut status) = (vec![0u8; 32 * n], vec![0u8; 32 * n], vec![0u8; n]);
        let rc = unsafe { plume_sign_batch(self.0, if v1 { 1 } else { 2 }, n, buf.as_ptr(), off.as_ptr(), sk.as_ptr(), r.as_ptr(), std::ptr::null(), pk.as_mut_ptr(),
                                           nul.as_mut_ptr(), c.as_mut_ptr(), s.as_mut_ptr(), rp.as_mut_ptr(), hr.as_mut_ptr(), status.as_mut_ptr()) };
        sk.iter_mut().for_each(|b| *b = 0);   // the reference zeroizes its secrets (SecretKey: ZeroizeOnDrop); so does the library on the device
        r.iter_mut().for_each(|b| *b = 0);
        if rc != 0 { return Err(last_error()); }
        Ok(signatures(msgs, v1, &pk, &nul, &c, &s, &rp, &hr, &status))
    }

    /// Same with each nonce derived on the GPU by RFC 6979 from (key, variant, message), hedged with `aux[i]` when given (`plume_sign_batch_rfc6979`):
    /// no nonce exists in host memory, and the same inputs give the same signatures.
    pub fn sign_batch_deterministic(&self, keys: &[SecretKey], msgs: &[&[u8]], v1: bool, aux: Option<&[[u8; 32]]>)
        -> Result<Vec<Result<PlumeSignature, SignError>>, HipError> {
        let n = keys.len();
        assert!(msgs.len() == n && aux.map_or(true, |a| a.len() == n));
        let (mut buf, mut off) = (Vec::new(), vec![0u64]);
        for m in msgs { buf.extend_from_slice(m); off.push(buf.len() as u64); }
        buf.push(0);
        let (mut sk, mut ax) = (vec![0u8; 32 * n], vec![0u8; if aux.is_some() { 32 * n } else { 0 }]);
        for i in 0..n { sk[32 * i..32 * i + 32].copy_from_slice(&keys[i].to_bytes()); }
        if let Some(a) = aux { for i in 0..n { ax[32 * i..32 * i + 32].copy_from_slice(&a[i]); } }
        let (mut pk, mut nul, mut rp, mut hr) = (vec![0u8; 64 * n], vec![0u8; 64 * n], vec![0u8; 64 * n], vec![0u8; 64 * n]);
        let (mut c, mut s, mut status) = (vec![0u8; 32 * n], vec![0u8; 32 * n], vec![0u8; n]);
        let rc = unsafe { plume_sign_batch_rfc6979(self.0, if v1 { 1 } else { 2 }, n, buf.as_ptr(), off.as_ptr(), sk.as_ptr(), if aux.is_some() { ax.as_ptr() } else { std::ptr::null() },
                                                   std::ptr::null(), pk.as_mut_ptr(), nul.as_mut_ptr(), c.as_mut_ptr(), s.as_mut_ptr(), rp.as_mut_ptr(), hr.as_mut_ptr(),
                                                   status.as_mut_ptr()) };
        sk.iter_mut().for_each(|b| *b = 0);
        ax.iter_mut().for_each(|b| *b = 0);
        if rc != 0 { return Err(last_error()); }
        Ok(signatures(msgs, v1, &pk, &nul, &c, &s, &rp, &hr, &status))
    }

    /// `SecretKey::from(scalar).to_sec1_der()` for a batch — the encoding the wasm wrapper uses for `s` and `digest_private`
    /// (javascript/src/lib.rs:98-110): SEC1 `ECPrivateKey { version 1, privateKey, publicKey = scalar * G (uncompressed) }`, 109 bytes.  The public-key
    /// field costs one generator multiplication per scalar: the GPU's doubling-free comb does them.
    pub fn scalars_to_sec1_der(&self, scalars: &[NonZeroScalar]) -> Result<Vec<[u8; 109]>, HipError> {
        let n = scalars.len();
        let mut flat = vec![0u8; 32 * n];
        for (i, k) in scalars.iter().enumerate() { flat[32 * i..32 * i + 32].copy_from_slice(&k.to_bytes()); }
        let (mut der, mut status) = (vec![0u8; 109 * n], vec![0u8; n]);
        let rc = unsafe { plume_scalars_to_sec1_der_batch(self.0, n, flat.as_ptr(), der.as_mut_ptr(), status.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        Ok(der.chunks_exact(109).map(|ch| { let mut a = [0u8; 109]; a.copy_from_slice(ch); a }).collect())
    }

    /// `SecretKey::from_sec1_der` for the 109-byte records of `scalars_to_sec1_der`, with the reference's semantics: `None` for a record of another shape, a scalar outside
    /// [1, n-1], or an embedded public key that is not scalar * G (elliptic-curve's `TryFrom<EcPrivateKey>` validates it; here the GPU recomputes it).
    pub fn scalars_from_sec1_der(&self, der: &[[u8; 109]]) -> Result<Vec<Option<NonZeroScalar>>, HipError> {
        let n = der.len();
        let flat: Vec<u8> = der.iter().flat_map(|d| d.iter().copied()).collect();
        let (mut sc, mut ok) = (vec![0u8; 32 * n], vec![0u8; n]);
        let rc = unsafe { plume_sec1_der_to_scalars_checked(self.0, n, flat.as_ptr(), sc.as_mut_ptr(), ok.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        Ok((0..n).map(|i| if ok[i] == 1 { get_scalar(&sc[32 * i..]) } else { None }).collect())
    }

    /// The circuit's square-root hints for `h2c(msg || SEC1c(pk))` (circuits/circom/verify_nullifier.circom:21-23,27-29) as 4 x 64-bit little-endian registers each:
    /// `[q0_gx1_sqrt, q0_gx2_sqrt, q0_y_pos, q1_gx1_sqrt, q1_gx2_sqrt, q1_y_pos]` per item.  UNPINNED: include/plume_hip.h defines them (the reference's generator
    /// of these inputs is not in its tree).
    pub fn h2c_hints(&self, msgs: &[&[u8]], pks: &[AffinePoint]) -> Result<Vec<[[u64; 4]; 6]>, HipError> {
        let n = msgs.len();
        assert!(pks.len() == n);
        let (mut buf, mut off) = (Vec::new(), vec![0u64]);
        for m in msgs { buf.extend_from_slice(m); off.push(buf.len() as u64); }
        buf.push(0);
        let mut pk = vec![0u8; 64 * n];
        for (i, p) in pks.iter().enumerate() { put_point(&mut pk[64 * i..], p); }
        let mut out = vec![0u8; 192 * n];
        let rc = unsafe { plume_h2c_hints_batch(self.0, n, buf.as_ptr(), off.as_ptr(), pk.as_ptr(), 1, out.as_mut_ptr()) };
        if rc != 0 { return Err(last_error()); }
        Ok(out.chunks_exact(192).map(|it| {
            let mut r = [[0u64; 4]; 6];
            for k in 0..6 { for j in 0..4 { r[k][j] = u64::from_le_bytes(it[32 * k + 8 * j..32 * k + 8 * j + 8].try_into().unwrap()); } }
            r
        }).collect())
    }

    /// Device-resident calls only (`plume_set_sub_batches`): 1 = strictly serial launch order (the default and, on the MI355X, the fastest: DESIGN.md section 6)
    pub fn set_sub_batches(&self, k: i32) -> Result<(), HipError> { if unsafe { plume_set_sub_batches(self.0, k) } == 0 { Ok(()) } else { Err(last_error()) } }
    /// Batches in flight (`plume_set_in_flight`): with 2, device-resident calls issued on different streams run side by side (two lanes of the context); default 1
    pub fn set_in_flight(&self, k: i32) -> Result<(), HipError> { if unsafe { plume_set_in_flight(self.0, k) } == 0 { Ok(()) } else { Err(last_error()) } }
    /// The verifier's first equation where `r_point` is given (`plume_set_eq1_short`): 1 = the short form for calls of at least `eq1_short()?.1` items (default), 3 = the short
    /// form whatever the size, 0 = the long form always, 2 = test mode (every item through the fallback).  Verdicts do not depend on it.
    pub fn set_eq1_short(&self, mode: i32) -> Result<(), HipError> { if unsafe { plume_set_eq1_short(self.0, mode as c_int) } == 0 { Ok(()) } else { Err(last_error()) } }
    /// `(mode, min_items)` in force (`plume_get_eq1_short`).
    pub fn eq1_short(&self) -> Result<(i32, usize), HipError> { let mut m: usize = 0; let r = unsafe { plume_get_eq1_short(self.0, &mut m) }; if r >= 0 { Ok((r as i32, m)) } else { Err(last_error()) } }
    /// Measurement hook (`plume_last_msm_kernel`): the multi-scalar kernel the last verify call on this context launched.
    pub fn last_msm_kernel(&self) -> Option<String> { let p = unsafe { plume_last_msm_kernel(self.0) }; if p.is_null() { None } else { Some(unsafe { std::ffi::CStr::from_ptr(p) }.to_string_lossy().into_owned()) } }
    /// The signer's self-check (`plume_set_sign_selfcheck`): mode 1 = every sign call verifies its own records on the GPU before anything reaches the caller's arrays;
    /// an item that does not verify comes back as `Err(SignError::SelfCheckFailed)`.  0 (the default) = off.
    pub fn set_sign_selfcheck(&self, mode: i32) -> Result<(), HipError> { if unsafe { plume_set_sign_selfcheck(self.0, mode as c_int) } == 0 { Ok(()) } else { Err(last_error()) } }
    /// The mode this context signs with (`plume_get_sign_selfcheck`).
    pub fn sign_selfcheck(&self) -> Result<i32, HipError> { let m = unsafe { plume_get_sign_selfcheck(self.0) }; if m >= 0 { Ok(m as i32) } else { Err(last_error()) } }
    /// The level this context signs at (`plume_get_sign_uniform`).
    pub fn sign_uniform(&self) -> Result<i32, HipError> { let l = unsafe { plume_get_sign_uniform(self.0) }; if l >= 0 { Ok(l as i32) } else { Err(last_error()) } }
    /// per-stage timing events inside the device pipelines: off by default (library 0.5); turn on before a call whose `last_stage_times` are wanted
    pub fn set_stage_timing(&self, on: bool) -> Result<(), HipError> { if unsafe { plume_set_stage_timing(self.0, on as c_int) } == 0 { Ok(()) } else { Err(last_error()) } }
    /// Host-pointer calls: 1 = every piece on the context itself, 2 (default) = pieces alternate between the context and a second lane.
    pub fn set_host_lanes(&self, lanes: i32) -> Result<(), HipError> { if unsafe { plume_set_host_lanes(self.0, lanes as c_int) } == 0 { Ok(()) } else { Err(last_error()) } }
    /// The signer's schedule (`plume_set_sign_uniform`).  k256's multiplication is constant-time, so the library's default is level 1 (no branch on a digit of `sk` or `r` in
    /// the kernels that walk them; table rows still gathered at digit-dependent addresses).  0 = fastest, not uniform; 2 = no secret-dependent address either (every row of a
    /// window's table is read and one kept by masked selects, as k256 does).  Outputs are unchanged at every level.
    pub fn set_sign_uniform(&self, level: i32) -> Result<(), HipError> { if unsafe { plume_set_sign_uniform(self.0, level as c_int) } == 0 { Ok(()) } else { Err(last_error()) } }
    /// The NUMA node shard `d`'s worker thread bound itself to (`None`: not bound) — allocate / pin the caller arrays of that shard's slice there
    pub fn shard_numa_node(&self, d: usize) -> Option<i32> { let v = unsafe { plume_shard_numa_node(self.0, d as c_int) }; if v >= 0 { Some(v) } else { None } }

    /// Page-lock a long-lived buffer once (`plume_host_register`): the copy engines then read / write it directly and the library's
    /// upload / compute / download pipeline overlaps fully.  Pair with `unpin`.
    pub fn pin(buf: &mut [u8]) -> Result<(), HipError> { if unsafe { plume_host_register(buf.as_mut_ptr() as *mut c_void, buf.len()) } == 0 { Ok(()) } else { Err(last_error()) } }
    pub fn unpin(buf: &mut [u8]) -> Result<(), HipError> { if unsafe { plume_host_unregister(buf.as_mut_ptr() as *mut c_void) } == 0 { Ok(()) } else { Err(last_error()) } }
}

// ------------------------------------------------------------------------------------------------ persistent nullifier set
/// The signatures of one sign call's outputs; an item on which the reference would panic comes back as `Err(SignError)`.
fn signatures(msgs: &[&[u8]], v1: bool, pk: &[u8], nul: &[u8], c: &[u8], s: &[u8], rp: &[u8], hr: &[u8], status: &[u8]) -> Vec<Result<PlumeSignature, SignError>> {
    (0..msgs.len()).map(|i| {
        let st = status[i];
        let nullifier = get_point(&nul[64 * i..]);
        if st & PLUME_STATUS_SELFCHECK_FAILED != 0 { return Err(SignError::SelfCheckFailed); }
        if st & PLUME_STATUS_BAD_SCALAR != 0 { return Err(SignError::BadScalar); }
        if st & PLUME_STATUS_IDENTITY != 0 && nullifier == AffinePoint::IDENTITY { return Err(SignError::HashedToIdentity); }     // :61
        if st & PLUME_STATUS_C_NOT_CANONICAL != 0 { return Err(SignError::ChallengeNotCanonical); }                           // :91
        if st & PLUME_STATUS_IDENTITY != 0 { return Err(SignError::ZeroResponse); }                                             // :95
        Ok(PlumeSignature {
            message: msgs[i].to_vec(), pk: get_point(&pk[64 * i..]), nullifier,
            c: get_scalar(&c[32 * i..]).ok_or(SignError::ChallengeNotCanonical)?, s: get_scalar(&s[32 * i..]).ok_or(SignError::ZeroResponse)?,
            v1specific: if v1 { Some(PlumeSignatureV1Fields { r_point: get_point(&rp[64 * i..]), hashed_to_curve_r: get_point(&hr[64 * i..]) }) } else { None },
        })
    }).collect()
}

/// A GPU-resident set of nullifiers that persists across batches (`plume_nullset_*`): `insert` tells which signatures carry a nullifier for the first
/// time EVER, across every earlier insert into the set — the check an application makes before it accepts a verified signature.  Lives on the engine's
/// (first) GPU and may outlive the engine.  One caller thread at a time.
pub struct NullifierSet(*mut c_void);
unsafe impl Send for NullifierSet {}
impl Drop for NullifierSet { fn drop(&mut self) { unsafe { plume_nullset_destroy(self.0) } } }

impl NullifierSet {
    /// An empty set with room for `reserve` records before its first growth.
    pub fn new(engine: &HipEngine, reserve: usize) -> Result<Self, HipError> {
        let mut h: *mut c_void = std::ptr::null_mut();
        if unsafe { plume_nullset_create(engine.0, reserve, &mut h) } == 0 { Ok(NullifierSet(h)) } else { Err(last_error()) }
    }
    /// `fresh[i]`: `live[i]` (None = all), the nullifier was not in the set, and no earlier live item of this call carries it.  Returns the flags and their count;
    /// every live nullifier is in the set afterwards.
    pub fn insert(&self, nullifiers: &[AffinePoint], live: Option<&[bool]>) -> Result<(Vec<bool>, u64), HipError> {
        let n = nullifiers.len();
        if let Some(l) = live { assert_eq!(l.len(), n, "one live flag per nullifier"); }
        let mut nul = vec![0u8; 64 * n];
        for (i, p) in nullifiers.iter().enumerate() { put_point(&mut nul[64 * i..], p); }
        let lv: Vec<u8> = live.map_or(Vec::new(), |l| l.iter().map(|b| *b as u8).collect());
        let mut fresh = vec![0u8; n];
        let mut cnt: u64 = 0;
        let rc = unsafe { plume_nullset_insert(self.0, n, nul.as_ptr(), if live.is_some() { lv.as_ptr() } else { std::ptr::null() }, std::ptr::null(), fresh.as_mut_ptr(), &mut cnt) };
        if rc == 0 { Ok((fresh.into_iter().map(|f| f != 0).collect(), cnt)) } else { Err(last_error()) }
    }
    /// Membership, read-only.
    pub fn contains(&self, nullifiers: &[AffinePoint]) -> Result<Vec<bool>, HipError> {
        let n = nullifiers.len();
        let mut nul = vec![0u8; 64 * n];
        for (i, p) in nullifiers.iter().enumerate() { put_point(&mut nul[64 * i..], p); }
        let mut found = vec![0u8; n];
        if unsafe { plume_nullset_contains(self.0, n, nul.as_ptr(), found.as_mut_ptr()) } == 0 { Ok(found.into_iter().map(|f| f != 0).collect()) } else { Err(last_error()) }
    }
    /// Number of nullifiers in the set.
    pub fn len(&self) -> Result<u64, HipError> {
        let (mut size, mut cap) = (0u64, 0u64);
        if unsafe { plume_nullset_size(self.0, &mut size, &mut cap) } == 0 { Ok(size) } else { Err(last_error()) }
    }
    pub fn reserve(&self, items: usize) -> Result<(), HipError> { if unsafe { plume_nullset_reserve(self.0, items) } == 0 { Ok(()) } else { Err(last_error()) } }
    pub fn clear(&self) -> Result<(), HipError> { if unsafe { plume_nullset_clear(self.0) } == 0 { Ok(()) } else { Err(last_error()) } }
    /// Every nullifier of the set, in no particular order.
    pub fn export(&self) -> Result<Vec<AffinePoint>, HipError> {
        let mut cnt: u64 = 0;
        if unsafe { plume_nullset_export(self.0, 0, std::ptr::null_mut(), &mut cnt) } != 0 { return Err(last_error()); }
        let mut rec = vec![0u8; 64 * cnt as usize];
        if cnt > 0 && unsafe { plume_nullset_export(self.0, cnt as usize, rec.as_mut_ptr(), &mut cnt) } != 0 { return Err(last_error()); }
        Ok(rec.chunks(64).take(cnt as usize).map(get_point).collect())
    }
    /// Device form: every pointer on the set's GPU, enqueued on `stream` (null = the set's own); `n_fresh` may be null.  Does not synchronise.
    ///
    /// # Safety
    /// The pointers must be valid device allocations of the sizes `plume_hip.h` states, alive until the work has run.
    pub unsafe fn insert_device(&self, n: usize, nullifier: *const u8, live: *const u8, ids: *const u64, fresh: *mut u8, n_fresh: *mut u64, stream: *mut c_void) -> Result<(), HipError> {
        if plume_nullset_insert_device(self.0, n, nullifier, live, ids, fresh, n_fresh, stream) == 0 { Ok(()) } else { Err(last_error()) }
    }
    /// Device form of `contains`.
    ///
    /// # Safety
    /// As for `insert_device`.
    pub unsafe fn contains_device(&self, n: usize, nullifier: *const u8, found: *mut u8, stream: *mut c_void) -> Result<(), HipError> {
        if plume_nullset_contains_device(self.0, n, nullifier, found, stream) == 0 { Ok(()) } else { Err(last_error()) }
    }
}

// ------------------------------------------------------------------------------------------------ the reference's single-item surface
impl PlumeSignature {
    /// `PlumeSignature::verify` (rust-k256/src/lib.rs:93-145) on the GPU — a batch of one; use `HipEngine::verify_batch` for throughput.
    pub fn verify(&self, engine: &HipEngine) -> bool { engine.verify_batch(std::slice::from_ref(self)).map(|v| v[0]).unwrap_or(false) }
    /// The 20-byte Ethereum address of `pk` (`HipEngine::eth_address_batch`); an error when `pk` is no Ethereum key (off the curve, or the identity).
    pub fn eth_address(&self, engine: &HipEngine) -> Result<[u8; 20], HipError> {
        engine.eth_address_batch(std::slice::from_ref(&self.pk), None)?.pop().flatten().map(|(a, _)| a).ok_or_else(|| HipError("eth_address: pk is not a non-identity curve point".to_string()))
    }
    /// `eth_address` as `"0x"` + 40 hex digits with the EIP-55 checksum.
    pub fn eth_address_eip55(&self, engine: &HipEngine) -> Result<String, HipError> {
        engine.eth_address_eip55_batch(std::slice::from_ref(&self.pk))?.pop().flatten().ok_or_else(|| HipError("eth_address_eip55: pk is not a non-identity curve point".to_string()))
    }
    /// `verify()` AND "`pk` is the key of `addr20`": the gate of a consumer that holds addresses, not public keys.  `false` for a `pk` that has no address.
    pub fn verify_for_address(&self, engine: &HipEngine, addr20: &[u8; 20]) -> bool {
        let matches = engine.eth_address_batch(std::slice::from_ref(&self.pk), Some(std::slice::from_ref(addr20))).ok().and_then(|mut v| v.pop().flatten()).map(|(_, m)| m).unwrap_or(false);
        matches && self.verify(engine)
    }
    /// `verify()` AND "`pk`'s address is on the allow-list whose Merkle root is `root32`": pk -> address -> leaf -> proof, for a consumer that holds one 32-byte root
    /// of a `StandardMerkleTree` of `["address"]` (or of `["address", "uint256"]` with `amount`).  `false` for a `pk` that has no address.
    pub fn verify_for_root(&self, engine: &HipEngine, root32: &[u8; 32], proof: &[[u8; 32]], amount: Option<&[u8; 32]>) -> bool {
        let on_list = self.eth_address(engine).ok().map_or(false, |a| engine.merkle_verify_address(&a, amount, proof, root32).unwrap_or(false));
        on_list && self.verify(engine)
    }
    /// The V1-specific fields this signature's `pk, nullifier, c, s` imply (`HipEngine::recover_batch`), for a `c` that is the V1 hash of them: upgrades a compact
    /// four-field record to a V1 record.  An error when the library rejects the inputs or `c` is not that hash -- never a silent pair of points that do not verify.
    pub fn recover_v1specific(&self, engine: &HipEngine) -> Result<PlumeSignatureV1Fields, HipError> {
        match engine.recover_batch(std::slice::from_ref(self), true)?.pop().flatten() {
            Some((fields, _h, true)) => Ok(fields),
            Some(_) => Err(HipError("recover_v1specific: c is not the V1 hash of the recovered points".to_string())),
            None => Err(HipError("recover_v1specific: an input is no value of the reference's types".to_string())),
        }
    }
    /// `PlumeSignature::sign_v1` (rust-k256/src/lib.rs:149-151; the doc comments of sign_v1 / sign_v2 are swapped there, the behaviour is this)
    pub fn sign_v1(engine: &HipEngine, secret_key: &SecretKey, msg: &[u8], rng: &mut impl CryptoRngCore) -> Self { PlumeSigner::new(secret_key, true).sign_with_rng(engine, rng, msg) }
    /// `PlumeSignature::sign_v2` (rust-k256/src/lib.rs:154-156)
    pub fn sign_v2(engine: &HipEngine, secret_key: &SecretKey, msg: &[u8], rng: &mut impl CryptoRngCore) -> Self { PlumeSigner::new(secret_key, false).sign_with_rng(engine, rng, msg) }
}

/// `plume_rustcrypto::randomizedsigner::PlumeSigner` (randomizedsigner.rs:25-41)
pub struct PlumeSigner<'signing> {
    secret_key: &'signing SecretKey,
    pub v1: bool,
}
impl<'signing> PlumeSigner<'signing> {
    pub fn new(secret_key: &'signing SecretKey, v1: bool) -> Self { PlumeSigner { secret_key, v1 } }
    /// `RandomizedSigner::try_sign_with_rng` (randomizedsigner.rs:43-112).  `Err` only where the reference returns `signature::Error` (h2c failure,
    /// unreachable with this DST), where the library call fails, or where the signer's self-check withheld the signature (`HipError::is_self_check_failed`);
    /// the reference's `expect`s panic here too, with its messages.
    pub fn try_sign_with_rng(&self, engine: &HipEngine, rng: &mut impl CryptoRngCore, msg: &[u8]) -> Result<PlumeSignature, HipError> {
        let mut out = engine.sign_batch(std::slice::from_ref(self.secret_key), &[msg], self.v1, rng)?;
        match out.remove(0) {
            Ok(sig) => Ok(sig),
            Err(SignError::HashedToIdentity) => panic!("something is drammatically wrong if the input hashed to the identity"),
            Err(SignError::ChallengeNotCanonical) => panic!("it should be impossible to get the hash equal to zero"),
            Err(SignError::ZeroResponse) => panic!("something is terribly wrong if the nonce is equal to negated product of the secret and the hash"),
            Err(SignError::BadScalar) => unreachable!("SecretKey is in [1, n-1] by construction"),
            Err(SignError::SelfCheckFailed) => Err(HipError::self_check_failed()),
        }
    }
    pub fn sign_with_rng(&self, engine: &HipEngine, rng: &mut impl CryptoRngCore, msg: &[u8]) -> PlumeSignature {
        self.try_sign_with_rng(engine, rng, msg).expect("libplume_hip call failed")
    }
    /// The nonce derived on the GPU by RFC 6979 from (secret key, variant, message), hedged with `aux` when given (`plume_sign_batch_rfc6979`); no RNG.
    pub fn sign_deterministic(&self, engine: &HipEngine, msg: &[u8], aux: Option<&[u8; 32]>) -> Result<PlumeSignature, HipError> {
        let a = aux.map(|a| [*a]);
        let mut out = engine.sign_batch_deterministic(std::slice::from_ref(self.secret_key), &[msg], self.v1, a.as_ref().map(|a| &a[..]))?;
        match out.remove(0) {
            Ok(sig) => Ok(sig),
            Err(SignError::HashedToIdentity) => panic!("something is drammatically wrong if the input hashed to the identity"),
            Err(SignError::ChallengeNotCanonical) => panic!("it should be impossible to get the hash equal to zero"),
            Err(SignError::ZeroResponse) => panic!("something is terribly wrong if the nonce is equal to negated product of the secret and the hash"),
            Err(SignError::BadScalar) => unreachable!("SecretKey is in [1, n-1] by construction; a derived nonce outside it has probability below 2^-2000"),
            Err(SignError::SelfCheckFailed) => Err(HipError::self_check_failed()),
        }
    }
}

#[cfg(test)]
mod tests {
    //! rust-k256/tests/signing.rs:9-64 against the GPU path (needs a gfx950 device and PLUME_HIP_LIB_DIR at build time)
    use super::*;
    use k256::elliptic_curve::rand_core::{CryptoRng, Error, RngCore};
    const R: [u8; 32] = hex_literal::hex!("93b9323b629f251b8f3fc2dd11f4672c5544e8230d493eceea98a90bda789808");
    const SK: [u8; 32] = hex_literal::hex!("519b423d715f8b581f4fa8ee59f4771a5b44c8130b4e3eacca54a56dda72b464");
    struct Mock;
    impl CryptoRng for Mock {}
    impl RngCore for Mock {
        fn next_u32(&mut self) -> u32 { unimplemented!() }
        fn next_u64(&mut self) -> u64 { unimplemented!() }
        fn fill_bytes(&mut self, dest: &mut [u8]) { dest.copy_from_slice(&R) }
        fn try_fill_bytes(&mut self, dest: &mut [u8]) -> Result<(), Error> { self.fill_bytes(dest); Ok(()) }
    }
    #[test]
    fn fixed_vector() {
        let engine = HipEngine::new(0).unwrap();
        let sk = SecretKey::from_slice(&SK).unwrap();
        let v1 = PlumeSignature::sign_v1(&engine, &sk, b"An example app message string", &mut Mock);
        assert_eq!(v1.c.to_bytes().as_slice(), hex_literal::hex!("c6a7fc2c926ddbaf20731a479fb6566f2daa5514baae5223fe3b32edbce83254"));
        assert_eq!(v1.s.to_bytes().as_slice(), hex_literal::hex!("e69f027d84cb6fe5f761e333d12e975fb190d163e8ea132d7de0bd6079ba28ca"));
        let v2 = PlumeSignature::sign_v2(&engine, &sk, b"An example app message string", &mut Mock);
        assert_eq!(v2.c.to_bytes().as_slice(), hex_literal::hex!("3dbfb717705010d4f44a70720c95e74b475bd3a783ab0b9e8a6b3b363434eb96"));
        assert_eq!(v2.s.to_bytes().as_slice(), hex_literal::hex!("528e8fbb6452f82200797b1a73b2947a92524bd611085a920f1177cb8098136b"));
        assert!(v1.verify(&engine) && v2.verify(&engine));
    }
}
