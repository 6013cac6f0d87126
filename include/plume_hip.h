/* plume_hip.h — C ABI of the MI355X batch PLUME sign/verify engine (libplume_hip.so).
 *
 * This is the drop-in boundary for the hot path of plume-sig/zk-nullifier-sig.  The reference has no FFI of
 * its own: its public Rust API is the boundary.  Each entry point below replaces, for a whole
 * batch at once, the Rust item named beside it; a `plume_rustcrypto`-compatible façade binds these with
 * `extern "C"` (INTEGRATION.md shows the stub).
 *
 * Data formats (all arrays are structure-of-arrays, caller-owned, never retained after return):
 *   point   64 bytes  affine x || y, big-endian; all-zero = the identity (k256 AffinePoint::IDENTITY)
 *   scalar  32 bytes  big-endian
 *   msgs    packed message bytes + (n+1) u64 offsets: message i = msgs[msg_off[i] .. msg_off[i+1])
 *   arrays of 32/64-byte records must be 4-byte aligned (16 recommended); msgs may have any alignment
 *
 * Return codes: 0 ok, -1 bad argument, -2 HIP runtime error (text via plume_last_error), -3 no usable GPU.
 * Nothing throws or unwinds across this boundary.  There is NO CPU fallback: without a gfx950 device
 * plume_init fails with -3.
 *
 * Threading: one plume_ctx is used by one host thread at a time; distinct contexts are independent and may be used
 * concurrently from different threads, also on the same GPU.  Multi-GPU, two ways: (a) one process holding all the
 * devices creates ONE context with plume_init_multi and passes whole batches to the host-pointer entry points, the
 * library shards them; (b) one process per GPU (torch.distributed / MPI ranks) each creates a plume_init context for
 * its device and passes its own contiguous shard.  The path has no cross-device exchange, so neither way involves a
 * collective.
 */
#ifndef PLUME_HIP_H
#define PLUME_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct plume_ctx plume_ctx;

#define PLUME_OK 0
#define PLUME_ERR_ARG (-1)
#define PLUME_ERR_HIP (-2)
#define PLUME_ERR_NODEV (-3)

/* sign status bits (per item) */
#define PLUME_STATUS_C_NOT_CANONICAL 1 /* SHA-256 digest was 0 or >= n: k256's sign panics here (rust-k256/src/randomizedsigner.rs:90-91), \
                                          arkworks' reduces (rust-arkworks/src/lib.rs:257); c is emitted reduced mod n */
#define PLUME_STATUS_BAD_SCALAR 2      /* sk or r outside [1, n-1] (NonZeroScalar / SecretKey invariant), a supplied pk not on the curve, or \
                                          (device-resident calls) message offsets that decrease or reach past msgs_bytes */
#define PLUME_STATUS_IDENTITY 4        /* H == identity (randomizedsigner.rs:61) or s == 0 (randomizedsigner.rs:95) */
#define PLUME_STATUS_SELFCHECK_FAILED 8 /* plume_set_sign_selfcheck(ctx, 1) only: the signer called the item good (no other bit) but its records do not verify; \
                                           every output record of the item is all zero */
#define PLUME_STATUS_BAD_TX 16         /* plume_eth_tx_sign_batch* only: the unsigned transaction breaks a framing rule, its offsets are rejected or its slot reaches past \
                                          out_bytes; reported alone, whatever the key is */
#define PLUME_STATUS_HD_NO_KEY 32      /* plume_hd_*_batch* only: BIP-32's outcomes that "have no key": IL >= n, child scalar 0 or child point = identity at some level \
                                          (master: IL = 0 or IL >= n) */
#define PLUME_STATUS_HD_HARDENED 64    /* plume_hd_derive_pub_batch* only: public derivation asked for an index >= 2^31 */

/* Create a context bound to HIP device `device_id` (>= 0): streams, events and a small scratch area; about 1.5 ms.  The generator's fixed tables are built by the first call
 * that needs them, ONCE per device and process -- (1..2^23)*G for the verifier's 24-bit windows (1 GiB, first verify / verify_non_zk call) and the signer's doubling-free
 * comb, 15 windows of 2^17 rows (252 MiB, first sign / SEC1-DER export / aggregate check) -- about 18 ms for both, synchronously inside that call.  They are read-only and
 * shared by every context of the process on that device; the last context to go frees them.  A verify-only process never holds the comb, a sign-only one never the 1 GiB table
 * -- unless it signs with the self-check on (plume_set_sign_selfcheck): the check is a verify_non_zk call, so such a signer holds the 1 GiB window table as well (equation 2
 * and the fallback of equation 1's short form walk it), next to the comb (level 0 / 1, and the check's short first equation for calls of at least 2^16 items) or the scanned table (level 2).
 * plume_destroy (and plume_set_in_flight when it takes lanes away) waits for the context's OWN work before it releases anything -- the last device-resident call it was
 * given, on whatever stream (every such call leaves an event behind its last kernel and waits for its predecessor's), and its private streams -- and does not call
 * hipDeviceSynchronize.  It then frees its workspace with hipFree, which the HIP runtime may itself implement with a device-wide wait: a caller that must not stall
 * other streams should destroy contexts at a quiet point.  A caller-provided stream must stay alive until the context's last call on it has finished. */
int plume_init(plume_ctx** out, int device_id);
/* Create a multi-device context: one shard (a complete single-device context with its own streams and workspace, driven by its own
 * worker thread) per entry of device_ids (SURVEY.md §8b sketch, §8e).  Every HOST-POINTER entry point below then splits its batch
 * evenly and contiguously -- shard d of g gets items [floor(d*n/g), floor((d+1)*n/g)) of every array -- runs the shards concurrently
 * and writes each shard's results into its slice of the caller's output arrays; there is no cross-device exchange and no collective.
 * A device id may repeat (two shards on one GPU overlap one's copies with the other's kernels).  The *_device entry points need
 * a single-device context (device pointers belong to one GPU) and return PLUME_ERR_ARG on a multi-device one;
 * plume_nullifier_first_occurrence runs on the first shard (every record has to meet every other). */
int plume_init_multi(plume_ctx** out, const int* device_ids, int n_devices);
/* 1 for plume_init contexts, n_devices for plume_init_multi contexts */
int plume_num_shards(const plume_ctx* ctx);
/* Each shard's worker thread (it issues all copies between the caller's arrays and its GPU) is bound to the CPUs of the NUMA node its GPU hangs off, found through the
 * device's PCI address in sysfs and cut to the CPUs the process may use; where that cannot be determined the thread is left alone (PLUME_NO_AFFINITY=1 switches the
 * binding off).  Returns the node shard `shard` was bound to, or -1.  Callers should allocate / page-lock their arrays on the same nodes. */
int plume_shard_numa_node(const plume_ctx* ctx, int shard);
void plume_destroy(plume_ctx* ctx);
/* Last error text of this thread (valid until the next failing call on the thread). */
const char* plume_last_error(void);
/* Library / build information: "plume_hip <major.minor> gfx950 build=<hash of the device sources>".  The number in the string stays 0.12 for library 0.13: callers
 * that need the 0.13, 0.14, 0.15 or 0.16 entry points look for the symbols (dlsym / getattr), as zk-nullifier-sig_amd/capi.py does.  0.16: signed raw Ethereum
 * transactions from unsigned payloads (plume_eth_tx_sign_batch*); 0.15: Keccak Merkle allow-lists
 * (plume_merkle_*); 0.14: the senders of raw Ethereum transactions
 * (plume_eth_tx_parse_batch*, plume_eth_tx_sender_batch*); 0.13: deterministic ECDSA signatures with a recovery id
 * (plume_ecdsa_sign_batch*) and the digest a wallet signs (plume_eth_message_hash_batch*: Keccak-256 of ragged messages, EIP-191); 0.12: public keys and addresses from
 * ECDSA signatures (plume_ecdsa_recover_batch*: ecrecover); 0.11: Ethereum addresses of public keys (plume_eth_address_batch*: Keccak-256);
 * 0.10: point recovery (plume_recover_batch*: r_point, hashed_to_curve_r and hashed_to_curve from pk, nullifier, c, s);
 * 0.9: the signer's self-check (plume_set_sign_selfcheck, PLUME_STATUS_SELFCHECK_FAILED); 0.8: derived signing nonces (plume_sign_batch_rfc6979*); 0.7: the persistent nullifier set (plume_nullset_*); 0.5 (round 5): plume_set_stage_timing, stage events off by default; 0.4 (round 5): plume_get_sign_uniform, plume_set_host_lanes, plume_set_eq1_short;
 * the signer defaults to uniform level 1; the generator tables are built by the first call that needs them; stream = NULL means the stream of the context the caller
 * holds; plume_destroy waits for the context's own work only (its last call on any stream and its private streams), not for the whole device. */
const char* plume_version(void);
/* Upper bound on items processed per internal pass (workspace is ~3.9 KB per in-flight item). Default 1<<20. */
int plume_set_chunk(plume_ctx* ctx, size_t max_items_per_pass);
/* Device-resident verify / sign calls of >= 2^17 items can be cut into `sub_batches` slices: validation + hash_to_curve and the window tables of
 * slice k+1 then run on a second stream of the context beside the multi-scalar kernel of slice k.  Results do not depend on it.  Default 1 =
 * strictly serial launch order on the caller's stream, which is also the mode in which plume_last_stage_times reports one time per kernel:
 * on the MI355X the overlapped order measured 1-3 % SLOWER than the serial one (round 3, LABNOTES.md §6: kernels of two streams sharing the
 * compute units cost more than the table kernel's idle issue slots give back), so the knob is an experiment's record, not a recommendation.
 * Env PLUME_SUB_BATCHES=k sets the default of new contexts, PLUME_SERIAL=1 forces 1 (and wins when both are set). */
int plume_set_sub_batches(plume_ctx* ctx, int sub_batches);
/* Batches in flight (default 1).  A context runs its device-resident calls one at a time: they share its workspace, so calls issued on different streams queue.  With
 * batches = 2 the calls go in turn to two lanes of the context (each with a workspace, streams and events of its own; the generator's fixed tables are shared), and calls the
 * caller issues on DIFFERENT streams can run side by side: every kernel of a 2^20 batch fills the chip, yet the memory-bound table passes and the ramps / tails of one batch's
 * kernels fit beside the issue-bound multi-scalar kernel of the other (about 1 % per batch), and SMALL calls leave the chip mostly empty: two of them side by side take much less
 * than one after the other -- on the MI355X, two lanes against one (profiles/r06_hw_queues_small_calls.txt): 2^10-item verifies -49 % per call, 2^12 -31 %, 2^14 -26 %,
 * 2^16 -13.6 % (1.17 instead of 1.36 ms per call), 2^17 -6.5 %, 2^18 -2.3 %; 2^20 signs -3 %; a third lane gains nothing more (1..4 accepted).
 * THE CALLER'S STREAMS MUST SIT ON DIFFERENT HARDWARE QUEUES for any of this: the HIP runtime multiplexes a process's streams onto GPU_MAX_HW_QUEUES (default 4) hardware
 * queues per priority level, and streams that share a queue run their kernels one after the other (round 6's kernel trace of two torch streams: every kernel of both on one
 * queue, no gain at any size).  Set GPU_MAX_HW_QUEUES=8 in the environment of the process before its first HIP call (the Python package and bench.py do; the figures above are
 * with it).  Do NOT give the two callers' streams different priorities instead: the command processor runs a high-priority queue's kernels alone.
 * Results do not depend on any of it; calls on one stream keep that stream's order -- including NULL, which always means the stream of the context the caller holds,
 * whichever lane serves the call (so a sign followed by a verify of its outputs, both with stream = NULL, stay ordered).  Costs a second per-batch workspace.  Env
 * PLUME_IN_FLIGHT_MIN=<items> keeps smaller calls on the first lane (default 0: none).  Single-device contexts only (a multi-device context
 * already runs its shards side by side).  plume_last_stage_times / plume_last_redo_tasks then report the lane of the last device-resident call. */
int plume_set_in_flight(plume_ctx* ctx, int batches);
/* The signer's schedule.  k256's scalar multiplication is constant-time (call sites rust-k256/src/randomizedsigner.rs:51-70), so the DEFAULT here is level 1
 * since round 5 (library 0.4; rounds 1-4 defaulted to level 0).  Env PLUME_SIGN_UNIFORM=<level> sets the default of new contexts; plume_set_sign_uniform(ctx, 0) opts out.
 *   level 0: fastest.  NOT uniform: zero digits of sk and r are skipped, digit signs are branches, table rows are gathered at digit-dependent addresses -- the instruction
 *            trace and the memory addresses of k_sign_gmul / k_sign_hmul depend on the secrets.
 *   level 1: (default) the two kernels that walk those digits (sk*G, r*G by the comb; sk*H, r*H by windows; also the comb of the SEC1-DER export, whose scalars are secret
 *            keys) run the same instructions for every digit value: every slot adds (a zero digit adds row 1 to a copy that a masked select drops), signs are masked selects,
 *            the accumulator starts at a fixed offset point that is subtracted at the end.  UNIFORM: control flow, instruction count.  NOT uniform: the ADDRESS of the
 *            table row each slot gathers (cache / HBM-channel timing).  Price on the MI355X: +2.5 % per signature.
 *   level 2: level 1, and no address is derived from a digit: every slot reads all 3 rows of its table (P, theta P, 2P: csrc/plume_ec.h) and keeps one by masked selects (what k256 does with its
 *            16-entry tables); the multiplications by G then use a 52-window x 16-row table instead of the 18-bit comb (52 additions instead of 15).  UNIFORM: control flow,
 *            instruction count, every memory address.  Price: +47 %.
 * At every level: the scalar side (reduction mod n, GLV split, digit recoding, s = r + sk*c) is select-based; the range checks of sk and r are not (an out-of-range scalar
 * is a status bit, not a secret worth protecting); nothing is claimed about power / EM channels.  Outputs are bit-identical at every level.  Returns PLUME_ERR_ARG for a
 * level outside 0..2.  Measurements: DESIGN.md §9. */
int plume_set_sign_uniform(plume_ctx* ctx, int level);
/* the level this context signs at (0, 1, 2), or a negative error code */
int plume_get_sign_uniform(const plume_ctx* ctx);
/* The signer's self-check (library 0.9), off by default: a deterministic signer that computes one signature wrongly and releases it leaks sk (s = r + sk c: the same
 * derived r under two challenges gives sk = (s - s') / (c - c')), and a pk_in that is on the curve but is not sk G yields status 0 and records no verifier accepts.
 * mode 0 = off: every byte, status, stage and table of the signer is what it was before 0.9.  mode 1 = check every item; any other mode is PLUME_ERR_ARG.
 * Env PLUME_SIGN_SELFCHECK=<mode> sets the default of new contexts.  Like plume_set_sign_uniform the setting reaches in-flight lanes, the host pipeline's lanes and the
 * shards of a plume_init_multi context, and it applies to EVERY sign entry point: plume_sign_batch, _sec1, _rfc6979 and their _device forms.  With mode 1, for item i:
 *   - the signer's own status is non-zero: the item is released exactly as mode 0 writes it, same bytes, same status;
 *   - otherwise pk (derived or pk_in), nullifier, c, s, r_point, hashed_to_curve_r are checked with msg_i as verify_non_zk(version, ..., digest_private = c) -- H
 *     recomputed from (msg, pk), the challenge re-hashed, both group equations; that covers all six outputs for V1 and V2 and, for a status-0 item, is true exactly when
 *     PlumeSignature::verify is.  Verdict 1: the records are released byte-identical to mode 0, status 0.  Any other verdict: EVERY output record of the item is all
 *     zero (64-, 33- and 32-byte forms alike) and status[i] = PLUME_STATUS_SELFCHECK_FAILED.
 * Nothing unchecked reaches caller memory: the sign kernels write context-owned staging (always 64-byte records; the _sec1 signers compress after the gate), the check
 * reads the staging, and one kernel (k_sign_release) writes the caller's arrays -- device-resident arrays on the caller's stream as well as the host pipeline's slots.
 * The staging is wiped on the call's stream behind the release.  The device-resident forms gain no host synchronisation.  The check runs the verifier's own stages on
 * the workspace the sign call holds and obeys the short-form / pair / split rules of a plume_verify_non_zk_batch_device call of that size; its cost is that call's
 * (plus 0.8 GB of copies per 2^20 items), its workspace the verifier's (3.9 KB per item in flight) plus 322 B of staging per item, its tables: plume_init.
 * plume_last_stage_times after such a call lists the sign stages, then the check's stages, then "sign_release"; plume_last_msm_kernel / plume_last_redo_tasks report the check's verify.
 * The check detects a wrong RESULT.  It says nothing about power or EM side channels, and a fault that hits signer and check alike (a wrong msg buffer) is out of its reach. */
int plume_set_sign_selfcheck(plume_ctx* ctx, int mode);
int plume_get_sign_selfcheck(const plume_ctx* ctx);
/* The verifier's first equation, R' = s G - c pk compared with the given r_point (rust-k256/src/lib.rs:101,115-121), for calls that GIVE r_point as a 64-byte record (V1
 * verify, verify_non_zk).  It is an identity check, so it may be multiplied by any tau != 0: with (tau, upsilon) from a half-GCD of c in the Eisenstein integers
 * (tau c = upsilon mod n through lambda; all four coefficients of about 64 bits -- csrc/plume_eis.h) the GPU checks  k G - upsilon pk - (tau - 1) R == R,  k = tau s mod n:
 * 66 doublings instead of 128 on that equation, the generator's term from the signer's comb, one more window table per item (R).  Verdicts are identical by construction:
 * the equivalence is exact, not probabilistic, and the pair is re-checked per item (tau c == upsilon mod n) before it is used -- a failure, which cannot happen, would send
 * the item to the long form.
 *   mode 1 (default): short form for calls of at least PLUME_EQ1_SHORT_MIN items (plume_get_eq1_short reports the threshold)
 *   mode 3: short form for calls of any size          mode 0: long form always
 *   mode 2: test mode -- every item takes the scalar stage's fallback, i.e. the long form inside the checked chain of the redo launch
 * Env PLUME_EQ1_SHORT, PLUME_EQ1_SHORT_MIN set the defaults of new contexts.  Measured on the MI355X, 2^20 V1 verifies (round 5, three-row tables): k_verify_msm -7 %,
 * the step -2.5 % (the fourth table and the half-GCD take the rest back: DESIGN.md). */
int plume_set_eq1_short(plume_ctx* ctx, int mode);
/* the mode in force (0..3, or a negative error code); min_items, when not NULL, receives the smallest call (items) that takes the short form in mode 1.  The rule looks at
 * the CALL's n, also when plume_set_sub_batches cuts the call into slices. */
int plume_get_eq1_short(const plume_ctx* ctx, size_t* min_items);
/* Environment knobs read when a context is created (tuning and A/B runs; results never depend on them):
 *   PLUME_SUB_BATCHES, PLUME_SERIAL, PLUME_OVERLAP_MIN   sub-batch overlap of the device-resident calls (plume_set_sub_batches)
 *   PLUME_HOST_PIECE, PLUME_HOST_FIRST_PIECE, PLUME_HOST_TAIL_PIECE, PLUME_HOST_REGISTER_MIN, PLUME_HOST_LANES (1 | 2), PLUME_HOST_SCHEDULE (explicit piece list, read per call)
 *                                                        the host-pointer pipeline (plume_set_host_*)
 *   PLUME_INGEST_SPLIT_MAX   verify calls of at most this many items run the ingest stage with two lanes per item (default 65536; 0: never)
 *   PLUME_MSM_PAIR_MAX       verify calls of at most this many items run every long-form chain of the multi-scalar stage as two half chains on two lanes, joined by one checked
 *                            addition (default 16384; 0: never): on a machine a small call leaves empty, the kernel's time is one chain's latency
 *   PLUME_JOBS_PER_LANE      jobs per lane of the table passes (default: 3..6 by batch size)
 *   PLUME_SIGN_UNIFORM       default level of plume_set_sign_uniform (0, 1, 2; default 1)
 *   PLUME_SIGN_SELFCHECK     default mode of plume_set_sign_selfcheck (0, 1; default 0)
 *   PLUME_EQ1_SHORT, PLUME_EQ1_SHORT_MIN   plume_set_eq1_short's mode and the smallest call that takes the short form (default 1, 65536)
 *   PLUME_NO_AFFINITY        multi-device contexts: leave the shard threads' CPU affinity alone */
/* Host-pointer calls only: a call is cut into pieces; piece k+1 uploads while piece k computes and piece k-1 downloads (an upload, a download and the compute streams,
 * four staging slots), so only the first upload and the last download are exposed.  The first piece is small (default 1<<16 items), each following piece up to three times
 * the one before, up to the largest piece (default 1<<19, capped by the chunk size); calls with large outputs (the signer: 320 bytes down per item) taper instead -- a first
 * piece of twice the tail piece (default 1<<16), a body of pieces of at most half the largest, then 3, 2 and 1 tail pieces -- so that the last, unhidden download is short.
 * The pieces of a VERIFY call alternate between the context and a second lane of its own (workspace + stream, created on the first such call) when EVERY array of the call
 * is page-locked.  The signer under the same condition (round 6, now that two lanes' kernels really run side by side -- plume_set_in_flight's note on hardware queues): uniform
 * pieces of the tail size dealt to the two lanes in turn (twice the tail size beyond 32 of them); 2^18..2^20 signs gain 2-7 %, 2^22 0.7 % over the tapered one-lane
 * schedule, which pageable callers and PLUME_HOST_SIGN_LANES=1 still get.  The copy streams are created at high priority: the runtime multiplexes a process's streams onto
 * a few hardware queues per priority level, and a copy stream that shares a queue with a compute stream waits for its kernels (round 5: a finished piece's download started
 * 6 ms late).  Env PLUME_HOST_TRACE=1 prints every call's timeline to stderr (per piece: upload, kernels, download on the GPU's clock; no profiler needed -- and none should be
 * attached: rocprofv3's memory-copy trace turns the downloads into blit kernels).  2^20 items from page-locked arrays on the MI355X: verify 19.3-20.5 ms, sign 17.9-18.7 ms
 * over the boxes met (round 5: 20.4-21.1 and 18.7-19.1), 0.89-0.94 of the device-resident rates.  Results do not depend on any of this. */
int plume_set_host_piece(plume_ctx* ctx, size_t largest_piece_items);
int plume_set_host_first_piece(plume_ctx* ctx, size_t items);
int plume_set_host_tail_piece(plume_ctx* ctx, size_t items);
/* 1 = every piece of a host-pointer call runs on the context itself, 2 (default) = pieces alternate between the context and a second lane (env PLUME_HOST_LANES) */
int plume_set_host_lanes(plume_ctx* ctx, int lanes);
/* Host-pointer calls: caller arrays of at least `bytes` bytes that are not page-locked yet are registered (hipHostRegister) for the
 * duration of the call; 0 (default) = never.  Registration costs more than one batch's copies save: callers that reuse their buffers
 * should page-lock them ONCE with the helpers below instead. */
int plume_set_host_register_min(plume_ctx* ctx, size_t bytes);

/* ---- page-locked host memory ----------------------------------------------------------------------------------
 * The host-pointer entry points accept any memory.  When the caller's arrays are page-locked the GPU's copy engines read and
 * write them directly and every transfer overlaps the kernels of the neighbouring pieces; pageable arrays go through the
 * runtime's staging copies and block the calling thread.  plume_host_alloc returns page-locked memory (NULL on failure);
 * plume_host_register page-locks memory the caller already owns (e.g. a Rust Vec's buffer) until plume_host_unregister. */
void* plume_host_alloc(size_t bytes);
void plume_host_free(void* p);
int plume_host_register(void* p, size_t bytes);
int plume_host_unregister(void* p);

/* ---- PlumeSignature::verify, batched  (rust-k256/src/lib.rs:93-145) -------------------------------------
 * version 1: V1 (v1specific = Some{r_point, hashed_to_curve_r}); version 2: V2 (r_point, hashed_to_curve_r NULL).
 * ok[i] = 1 iff the reference's verify() returns true for item i, else 0.  Inputs the Rust types cannot even
 * represent (c or s outside [1, n-1], coordinates >= p, points off the curve) give ok = 0.
 * Host-pointer form: copies in, runs, copies ok[] out, returns when done. */
int plume_verify_batch(plume_ctx* ctx, int version, size_t n,
                       const uint8_t* msgs, const uint64_t* msg_off,
                       const uint8_t* pk, const uint8_t* nullifier, const uint8_t* c, const uint8_t* s,
                       const uint8_t* r_point, const uint8_t* hashed_to_curve_r,
                       uint8_t* ok);

/* ---- plume_arkworks' verify_non_zk, batched  (rust-arkworks/src/tests.rs:28-78; the verification the arkworks crate's tests and the
 * circuit's witness checks use) -------------------------------------------------------------------------------------------------
 * Inputs as the reference takes them: pk, message, PlumeSignaturePublic{s, nullifier}, PlumeSignaturePrivate{hashed_to_curve_r,
 * r_point, digest_private}.  Differences from plume_verify_batch: the challenge c' = SHA256(..) mod n is hashed from the GIVEN
 * r_point / hashed_to_curve_r (6 encodings for V1, 3 for V2: compute_c_v1 / compute_c_v2, rust-arkworks/src/lib.rs:120-163); BOTH
 * equations s*G - digest_private*pk == r_point and s*H - digest_private*nullifier == hashed_to_curve_r are checked for V1 AND V2;
 * s and digest_private are Fr elements, so zero is a value (>= n cannot be represented: ok = 0).
 * ok[i] = 1 Ok(true), 0 Ok(false), 2 Err(HashToCurveError) (pk is the identity, rust-arkworks/src/lib.rs:99-101). */
int plume_verify_non_zk_batch(plume_ctx* ctx, int version, size_t n,
                              const uint8_t* msgs, const uint64_t* msg_off,
                              const uint8_t* pk, const uint8_t* nullifier, const uint8_t* s,
                              const uint8_t* r_point, const uint8_t* hashed_to_curve_r, const uint8_t* digest_private,
                              uint8_t* ok);

/* ---- verify with SEC1-compressed points (33-byte records) --------------------------------------------------
 * The wire format of the reference's serde / wasm layer (javascript/src/lib.rs:95-118,147-184; sec1_affine,
 * rust-arkworks/src/lib.rs:76-88): 02|03 || x big-endian, or a record whose first byte is 00 for the identity (the
 * remaining 32 bytes are ignored).  Decompression (y = sqrt(x^3 + 7), parity from the tag) and on-curve validation run
 * on the GPU; a record that would fail to deserialize in the reference (other tag, x >= p, x not on the curve) gives
 * ok = 0.  Everything else as plume_verify_batch. */
int plume_verify_batch_sec1(plume_ctx* ctx, int version, size_t n,
                            const uint8_t* msgs, const uint64_t* msg_off,
                            const uint8_t* pk33, const uint8_t* nullifier33, const uint8_t* c, const uint8_t* s,
                            const uint8_t* r_point33, const uint8_t* hashed_to_curve_r33,
                            uint8_t* ok);

/* ---- PlumeSigner::try_sign_with_rng / PlumeSignature::sign_v1|sign_v2, batched, nonce supplied -----------
 * (rust-k256/src/randomizedsigner.rs:43-112, rust-k256/src/lib.rs:149-156; the RNG stays on the host: r[i] is
 * the 32 bytes the reference would draw, cf. the mock RNG in rust-k256/tests/signing.rs:23-44).
 * pk_in == NULL : pk = sk*G is derived (plume_rustcrypto shape).
 * pk_in != NULL : plume_arkworks::sign_with_r shape (rust-arkworks/src/lib.rs:229-278): pk supplied, not recomputed.
 * Outputs: pk (may be NULL), nullifier, c (= digest mod n), s, r_point, hashed_to_curve_r (always written, V1 and
 * V2), status[i] bit set as above.  version selects the c-hash (V1: G,pk,H,nul,R,Hr; V2: nul,R,Hr). */
int plume_sign_batch(plume_ctx* ctx, int version, size_t n,
                     const uint8_t* msgs, const uint64_t* msg_off,
                     const uint8_t* sk, const uint8_t* r, const uint8_t* pk_in,
                     uint8_t* pk, uint8_t* nullifier, uint8_t* c, uint8_t* s,
                     uint8_t* r_point, uint8_t* hashed_to_curve_r, uint8_t* status);

/* ---- hash_to_curve(m, pk), batched  (rust-k256/src/utils.rs:11-20) ----------------------------------------
 * h_out[i] = h2c(msg_i || SEC1c(pk_i)) with DST rust-k256/src/lib.rs:61.  pk == NULL hashes the raw message
 * bytes (Secp256k1::hash_from_bytes(&[msg], &[DST]); rust-k256/tests/verification.rs:148-156) for KAT pinning. */
int plume_hash_to_curve_batch(plume_ctx* ctx, size_t n,
                              const uint8_t* msgs, const uint64_t* msg_off,
                              const uint8_t* pk, uint8_t* h_out);

/* ---- circuit witness hints from the GPU hash_to_curve   -----------------------------------------------
 * The circom verifier (circuits/circom/verify_nullifier.circom:14-31,152-162) takes the hash_to_curve intermediates as
 * precomputed inputs; the GPU computes them anyway.  Per item, for h2c(msg_i || SEC1c(pk_i)) (pk == NULL: the raw message bytes):
 *   u       n x 64  : u0 | u1                                     hash_to_field (RFC 9380 §5.2)
 *   mapped  n x 128 : q0_x_mapped | q0_y_mapped | q1_x_mapped | q1_y_mapped     simplified-SWU outputs, affine, on the isogenous curve E'
 *   q       n x 128 : Q0.x | Q0.y | Q1.x | Q1.y                   after the 3-isogeny, on secp256k1 (identity = zeros)
 *   h       n x 64  : H = Q0 + Q1
 * Any output may be NULL.  registers = 0: every value is 32 big-endian bytes; registers = 1: every value is the circuit's 4 x 64-bit
 * little-endian registers (circuits/circom/utils.ts:11-17 scalarToCircuitValue), i.e. out + 32*k is a uint64_t[4].
 * q*_gx1_sqrt, q*_gx2_sqrt, q*_y_pos come from plume_h2c_hints_batch below (UNPINNED definitions).
 * An invalid pk (or malformed message offsets) zeroes the item's outputs. */
int plume_h2c_intermediates_batch(plume_ctx* ctx, size_t n,
                                  const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* pk,
                                  int registers, uint8_t* u, uint8_t* mapped, uint8_t* q, uint8_t* h);
/* The remaining hash_to_curve inputs of the circuit: q{0,1}_gx1_sqrt, q{0,1}_gx2_sqrt, q{0,1}_y_pos (verify_nullifier.circom:21-23,27-29).
 * UNPINNED: the reference obtains them from secp256k1_hash_to_curve_circom's ts/generate_inputs (circuits/circom/test/v1.test.ts:5,38-40), a package that is not in
 * the reference tree, and holds no vector of them -- so nothing here can be checked against the reference.  They are DEFINED as follows from RFC 9380 F.2 / F.2.1.2,
 * for each of the two maps k = 0, 1 with u = u_k, Z = -11, E': y^2 = x^3 + A'x + B':
 *     x1 = (-B'/A')(1 + 1/(Z^2 u^4 + Z u^2))   (B'/(Z A') when the denominator vanishes),   gx1 = x1^3 + A' x1 + B'
 *     x2 = Z u^2 x1,                                                                        gx2 = x2^3 + A' x2 + B'  ( = (Z u^2)^3 gx1: exactly one of gx1, gx2 is a square)
 *     qk_gx1_sqrt = the EVEN root r (r mod 2 = 0, 0 <= r < p) of  r^2 = gx1  if gx1 is a square,  of  r^2 = Z gx1  if it is not
 *     qk_gx2_sqrt = the EVEN root of  r^2 = gx2  if gx2 is a square,  of  r^2 = Z gx2  if it is not
 *                   (the second form is sqrt_ratio's return value for a non-residue, RFC 9380 F.2.1.2: a witness that gx is NOT a square, Z being a non-residue)
 *     qk_y_pos    = the root y of  y^2 = (gx1 if it is a square, else gx2)  with sgn0(y) = sgn0(u): the y the map returns, i.e. qk_y_mapped
 * A consumer whose generator fixes these choices differently (the other root; 1 in place of the non-residue witness) derives its values from these with a negation /
 * a constant.  hints: n x 192 bytes, q0_gx1_sqrt | q0_gx2_sqrt | q0_y_pos | q1_gx1_sqrt | q1_gx2_sqrt | q1_y_pos, each 32 bytes (registers as above).
 * tests: the algebraic definitions above against the Python oracle's big-integer restatement (oracle/plume_oracle.py h2c_hints), incl. RFC 9380 J.8.1's messages. */
int plume_h2c_hints_batch(plume_ctx* ctx, size_t n, const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* pk, int registers, uint8_t* hints);
/* 32-byte big-endian values (c, s, pk.x, pk.y, nullifier.x, ... of a signature) -> 4 x 64-bit little-endian registers each
 * (circuits/circom/utils.ts:11-17, verify_nullifier.circom:380-385).  Host memory; no context needed. */
int plume_registers_from_be(size_t nvalues, const uint8_t* be32, uint64_t* registers);

/* ---- SEC1-DER scalar marshalling  (the wasm layer's wire format for `s` and `digest_private`) --------------
 * der109[i] = SecretKey::from(scalar_i).to_sec1_der() (javascript/src/lib.rs:98-110): the 109-byte RFC 5915 ECPrivateKey
 *   30 6b 02 01 01 04 20 <scalar> a1 44 03 42 00 04 <x> <y>      with (x, y) = scalar * G
 * The generator multiplications run on the GPU (doubling-free comb).  status[i] = 0, or PLUME_STATUS_BAD_SCALAR with an all-zero
 * record when the scalar is outside [1, n-1] (no SecretKey holds it). */
int plume_scalars_to_sec1_der_batch(plume_ctx* ctx, size_t n, const uint8_t* scalars, uint8_t* der109, uint8_t* status);
/* SecretKey::from_sec1_der for that fixed form, with the reference's semantics (elliptic-curve's TryFrom<EcPrivateKey> validates the embedded public key): ok[i] = 1
 * iff record i has exactly this structure, a scalar in [1, n-1], AND a public-key field equal to scalar * G (recomputed on the GPU by the comb and compared byte for
 * byte); scalars[i] = the 32-byte scalar then, zeros otherwise. */
int plume_sec1_der_to_scalars_checked(plume_ctx* ctx, size_t n, const uint8_t* der109, uint8_t* scalars, uint8_t* ok);
/* The structure half alone (host memory, no context, no GPU): shape + scalar range.  The public-key field is NOT checked against the scalar, so a record with a
 * tampered public key passes here where the reference returns Err -- use the _checked form wherever the record comes from outside. */
int plume_sec1_der_to_scalars(size_t n, const uint8_t* der109, uint8_t* scalars, uint8_t* ok);

/* plume_sign_batch with the point outputs as 33-byte SEC1-compressed records (02|03 || x; identity = 00 followed by 32 zero
 * bytes) -- the wire format of the reference's serde / wasm layer (javascript/src/lib.rs:95-118).  pk_in stays 64-byte affine. */
int plume_sign_batch_sec1(plume_ctx* ctx, int version, size_t n,
                          const uint8_t* msgs, const uint64_t* msg_off,
                          const uint8_t* sk, const uint8_t* r, const uint8_t* pk_in,
                          uint8_t* pk33, uint8_t* nullifier33, uint8_t* c, uint8_t* s,
                          uint8_t* r_point33, uint8_t* hashed_to_curve_r33, uint8_t* status);

/* ---- nullifier-set post-processing: first occurrences   --------------------------------
 * PLUME exists so that an application can accept ONE nullifier per (pk, message) (reference README.md:5; the field
 * rust-k256/src/lib.rs:72-73); after verifying a batch the application has to find repeated nullifiers.
 *   nullifier : n x 64 B (x||y big-endian, all-zero = identity), as passed to / produced by the calls above
 *   live      : optional n bytes; 0 = the item takes no part (e.g. ok[i] == 0).  NULL = all items
 *   ids       : optional n distinct 64-bit ids deciding which of several equal nullifiers is "first" (smallest id); NULL = the
 *               position i.  Used when the arrays are one shard of a larger set (multi-GPU exchange)
 *   first     : out, n bytes: 1 iff the item is live and no live item with the same 64-byte nullifier has a smaller id
 *   n_unique  : out, optional: number of 1s in `first`
 * Deterministic whatever the execution order.  n <= 2^30. */
int plume_nullifier_first_occurrence(plume_ctx* ctx, size_t n, const uint8_t* nullifier, const uint8_t* live,
                                     const uint64_t* ids, uint8_t* first, uint64_t* n_unique);

/* ---- aggregate pre-filter: one random-linear-combination check of the whole batch   ---------
 * DIFFERENT SEMANTICS from the verify calls: all-or-nothing and probabilistic -- a fast way to learn that EVERY item of a batch would verify,
 * never a replacement for the per-item `ok`.  It applies where r_point and hashed_to_curve_r are GIVEN: mode 0 = PlumeSignature::verify of V1
 * signatures (rust-k256/src/lib.rs:93-135; version must be 1), mode 1 = verify_non_zk, V1 or V2 (rust-arkworks/src/tests.rs:28-78; `c` is
 * digest_private).  Per item the inputs are validated and the challenge hash is checked EXACTLY (hash_ok); the two group equations
 * s*G - c*pk == r_point and s*H - c*nullifier == hashed_to_curve_r are checked only in aggregate:
 *     A = sum_i a_i (s_i G - c_i pk_i - R_i) + b_i (s_i H_i - c_i nul_i - Hr_i) == identity,
 * one multi-scalar multiplication over 5n points (bucket method), with 127-bit coefficients a_i | b_i = SHA256(seed || be64(i)).  The
 * producer of the batch must not be able to predict `seed` (draw 32 fresh random bytes per call): a batch holding a false equation then
 * passes with probability <= 2^-126.  When the check fails, run the per-item verify to find the culprits.
 *   seed    : 32 bytes, HOST pointer in both forms; NULL = the library draws 32 bytes from the OS generator for this call (callers without fresh randomness of
 *             their own should pass NULL rather than anything constant, reused or known to the signers: the check is only as sound as the seed is unpredictable)
 *   hash_ok : out, optional, n bytes: 1 = the item's inputs are values of the reference's types and c equals the hash
 *   result  : out, PLUME_AGG_RESULT_BYTES = 72 bytes:
 *               [0] all_ok (n_bad == 0 and A is the identity)   [1] A is the identity   [2..4) zero   [4..8) n_bad, u32 little-endian
 *               (items with hash_ok == 0; they take no part in A when their inputs are not representable)
 *               [8..72) A as an affine point (x||y big-endian, zeros = identity) -- a pure function of the inputs and the seed, whatever
 *               the piece / shard cut: tests compare it with the oracle's
 * The multi-device context shards the batch; the shards' sums are added on the first shard's GPU. */
#define PLUME_AGG_RESULT_BYTES 72
int plume_aggregate_check(plume_ctx* ctx, int version, int mode, size_t n,
                          const uint8_t* msgs, const uint64_t* msg_off,
                          const uint8_t* pk, const uint8_t* nullifier, const uint8_t* c, const uint8_t* s,
                          const uint8_t* r_point, const uint8_t* hashed_to_curve_r,
                          const uint8_t seed[32], uint8_t* hash_ok, uint8_t* result);

/* ---- device-resident forms -------------------------------------------------------------------------------
 * Same semantics, but every data pointer is a DEVICE pointer on the context's GPU and the work is enqueued on
 * `stream` (a hipStream_t passed as void*; NULL = the context's own stream) without synchronising: the caller
 * orders and waits (e.g. torch.cuda streams/events).  n must not exceed the chunk size (plume_set_chunk).
 * msgs_bytes = the size of the msgs buffer: the offsets live on the device, so the kernels check them -- an item whose offsets
 * decrease or reach past msgs_bytes is rejected (verify: ok = 0; sign: PLUME_STATUS_BAD_SCALAR; hash_to_curve: identity) and its
 * lane never reads msgs.
 * Streams: the calls of one context share its workspace.  Each call first makes its stream wait (hipStreamWaitEvent) for the
 * previous call's last kernel, so calls issued on DIFFERENT streams of one context are safe (they serialise on the workspace);
 * outputs are ready when the stream the call was issued on reaches the end of the call.  One host thread per context at a time. */
int plume_verify_batch_device(plume_ctx* ctx, int version, size_t n,
                              const uint8_t* msgs, const uint64_t* msg_off, size_t msgs_bytes,
                              const uint8_t* pk, const uint8_t* nullifier, const uint8_t* c, const uint8_t* s,
                              const uint8_t* r_point, const uint8_t* hashed_to_curve_r,
                              uint8_t* ok, void* stream);
int plume_verify_non_zk_batch_device(plume_ctx* ctx, int version, size_t n,
                                     const uint8_t* msgs, const uint64_t* msg_off, size_t msgs_bytes,
                                     const uint8_t* pk, const uint8_t* nullifier, const uint8_t* s,
                                     const uint8_t* r_point, const uint8_t* hashed_to_curve_r, const uint8_t* digest_private,
                                     uint8_t* ok, void* stream);
int plume_verify_batch_sec1_device(plume_ctx* ctx, int version, size_t n,
                                   const uint8_t* msgs, const uint64_t* msg_off, size_t msgs_bytes,
                                   const uint8_t* pk33, const uint8_t* nullifier33, const uint8_t* c, const uint8_t* s,
                                   const uint8_t* r_point33, const uint8_t* hashed_to_curve_r33,
                                   uint8_t* ok, void* stream);
int plume_sign_batch_device(plume_ctx* ctx, int version, size_t n,
                            const uint8_t* msgs, const uint64_t* msg_off, size_t msgs_bytes,
                            const uint8_t* sk, const uint8_t* r, const uint8_t* pk_in,
                            uint8_t* pk, uint8_t* nullifier, uint8_t* c, uint8_t* s,
                            uint8_t* r_point, uint8_t* hashed_to_curve_r, uint8_t* status, void* stream);
int plume_hash_to_curve_batch_device(plume_ctx* ctx, size_t n,
                                     const uint8_t* msgs, const uint64_t* msg_off, size_t msgs_bytes,
                                     const uint8_t* pk, uint8_t* h_out, void* stream);
int plume_h2c_intermediates_batch_device(plume_ctx* ctx, size_t n,
                                         const uint8_t* msgs, const uint64_t* msg_off, size_t msgs_bytes, const uint8_t* pk,
                                         int registers, uint8_t* u, uint8_t* mapped, uint8_t* q, uint8_t* h, void* stream);
int plume_h2c_hints_batch_device(plume_ctx* ctx, size_t n, const uint8_t* msgs, const uint64_t* msg_off, size_t msgs_bytes, const uint8_t* pk, int registers,
                                 uint8_t* hints, void* stream);
int plume_scalars_to_sec1_der_batch_device(plume_ctx* ctx, size_t n, const uint8_t* scalars, uint8_t* der109, uint8_t* status, void* stream);
int plume_registers_from_be_device(plume_ctx* ctx, size_t nvalues, const uint8_t* be32, uint64_t* registers, void* stream);
int plume_sign_batch_sec1_device(plume_ctx* ctx, int version, size_t n,
                                 const uint8_t* msgs, const uint64_t* msg_off, size_t msgs_bytes,
                                 const uint8_t* sk, const uint8_t* r, const uint8_t* pk_in,
                                 uint8_t* pk33, uint8_t* nullifier33, uint8_t* c, uint8_t* s,
                                 uint8_t* r_point33, uint8_t* hashed_to_curve_r33, uint8_t* status, void* stream);
/* n_unique, when not NULL, is a DEVICE pointer to one uint64_t */
int plume_nullifier_first_occurrence_device(plume_ctx* ctx, size_t n, const uint8_t* nullifier, const uint8_t* live,
                                            const uint64_t* ids, uint8_t* first, uint64_t* n_unique, void* stream);

/* index_base: coefficient index of item 0 (pieces of one batch checked by separate calls must use disjoint index ranges); hash_ok (optional) and
 * result are DEVICE pointers, seed is a HOST pointer */
int plume_aggregate_check_device(plume_ctx* ctx, int version, int mode, size_t n,
                                 const uint8_t* msgs, const uint64_t* msg_off, size_t msgs_bytes,
                                 const uint8_t* pk, const uint8_t* nullifier, const uint8_t* c, const uint8_t* s,
                                 const uint8_t* r_point, const uint8_t* hashed_to_curve_r,
                                 const uint8_t seed[32], uint64_t index_base, uint8_t* hash_ok, uint8_t* result, void* stream);

/* ---- derived signing nonces: RFC 6979, optionally hedged  (library 0.8) ------------------------------------
 * plume_sign_batch with r computed on the GPU instead of supplied: PLUME's s = r + sk*c leaks sk when r repeats under two different c, or is biased.  For item i,
 * with version in {1, 2} and mode = 0 when pk_in is NULL, 1 otherwise:
 *     h1  = SHA-256( "PLUME-RFC6979" (13 ASCII bytes) || u8 version || u8 mode || pk_in[i] (64 B, mode 1 only) || msg_i )
 *     x   = sk[i], the 32 bytes as given
 *     r_i = RFC 6979 section 3.2 steps a-h with HMAC-SHA-256, q = n (the secp256k1 group order), qlen = hlen = 256, bits2octets(h1) = int2octets(int(h1) mod n);
 *           aux != NULL: k' = aux[i] (32 B) is appended after bits2octets(h1) in steps d and f (section 3.6, "hedged" signing); nothing is appended otherwise.
 * Every output (pk, nullifier, c, s, r_point, hashed_to_curve_r, status) is then byte-identical to plume_sign_batch given r[i] = r_i, at every
 * plume_set_sign_uniform level.  Version, mode and pk_in are in h1 because everything that feeds c feeds r: the same (sk, msg) signed as V1 and V2, or under two
 * supplied pk_in, gets two nonces.  Identical inputs give identical signatures.
 * Step h's retry (a candidate outside [1, n-1], probability ~2^-128) runs at most 16 candidates per item; an item that exhausts them (probability below 2^-2000)
 * gets r_i = 0 and so PLUME_STATUS_BAD_SCALAR.  sk outside [1, n-1], pk_in off the curve and rejected message offsets behave as in plume_sign_batch*; a rejected
 * offset hashes the empty message and msgs is not read for it.
 * The nonce exists only in the context's device workspace between the kernels that use it -- never in host memory -- and is wiped on the call's stream after the
 * last of them.  There is no API that returns it.  Argument checks, error codes, routing, sharding over plume_init_multi and threading are those of
 * plume_sign_batch / plume_sign_batch_device; aux may be NULL where those require r.  The host form stages aux like sk and wipes the staged copies. */
int plume_sign_batch_rfc6979(plume_ctx* ctx, int version, size_t n, const uint8_t* msgs, const uint64_t* msg_off,
                             const uint8_t* sk, const uint8_t* aux, const uint8_t* pk_in,
                             uint8_t* pk, uint8_t* nullifier, uint8_t* c, uint8_t* s,
                             uint8_t* r_point, uint8_t* hashed_to_curve_r, uint8_t* status);
int plume_sign_batch_rfc6979_device(plume_ctx* ctx, int version, size_t n,
                                    const uint8_t* msgs, const uint64_t* msg_off, size_t msgs_bytes,
                                    const uint8_t* sk, const uint8_t* aux, const uint8_t* pk_in,
                                    uint8_t* pk, uint8_t* nullifier, uint8_t* c, uint8_t* s,
                                    uint8_t* r_point, uint8_t* hashed_to_curve_r, uint8_t* status, void* stream);

/* ---- point recovery: r_point and hashed_to_curve_r from c and s  (library 0.10) -------------------------------
 * A V2 signature drops r_point and hashed_to_curve_r because they follow from the rest (circuits/circom/verify_nullifier.circom:140-222, check_ec_equations):
 *     r_point = s G - c pk          hashed_to_curve_r = s H - c nullifier          H = hash_to_curve(msg, pk)
 * plume_verify_batch(version 2) computes both for every item and hashes them; this call runs the same pipeline and RETURNS them, with H, in the requested record
 * format: the public outputs of the plume_v2 circuit, the missing half of a V1 record, or the points plume_verify_non_zk_batch / plume_aggregate_check want given.
 * Any of the four outputs may be NULL (it is then neither computed past what the others need nor written); at least one must not be.  For item i:
 *   validation  exactly plume_verify_batch(version 2)'s: c, s in [1, n-1]; coordinates below p; pk and nullifier on the curve or the all-zero identity; in the
 *               device form the message offsets.  A rejected item gets status PLUME_RECOVER_INVALID and all-zero records, and in the device form its lane never
 *               reads msgs.  An identity pk is accepted, with the single 00 byte in the preimages, as verify does.
 *   points      an accepted item gets the three points whatever the hash says.  s G = c pk and s H = c nullifier give identity records.
 *   status      version 2: PLUME_RECOVER_MATCH iff c == SHA256(enc(nullifier), enc(r_point), enc(hashed_to_curve_r)) mod n, i.e. iff plume_verify_batch(2, ...) gives
 *               ok = 1;  version 1: the six-encoding hash (G, pk, H, nullifier, r_point, hashed_to_curve_r), i.e. iff plume_verify_batch(1, ...) gives ok = 1 when
 *               handed the recovered points.  PLUME_RECOVER_MISMATCH otherwise.
 * Inputs are 64-byte points and 32-byte scalars as for plume_verify_batch.  Argument checks, error codes, the chunk limit, workspace waits, in-flight lanes,
 * plume_set_sub_batches, the small-call rules and sharding over plume_init_multi are those of plume_verify_batch / plume_verify_batch_device; the measurement hooks
 * report the call as a V2 verify whose last stage is "recover_finalize".  Output arrays of the 64-byte formats should be 16-byte aligned (hipMalloc, torch and numpy
 * arrays are): the records are then written with 16-byte stores; any alignment is correct. */
#define PLUME_RECOVER_MISMATCH 0   /* points computed; c is not the version's hash of them */
#define PLUME_RECOVER_MATCH    1   /* points computed; c matches */
#define PLUME_RECOVER_INVALID  3   /* an input is no value of the reference's types; every output record of the item is all zero */
#define PLUME_RECOVER_FMT_AFFINE64  0   /* 64 B x||y big-endian, zeros = identity */
#define PLUME_RECOVER_FMT_SEC1      1   /* 33 B, 02|03||x; identity = 00 + 32 zero bytes */
#define PLUME_RECOVER_FMT_REGISTERS 2   /* 64 B = uint64_t[2][4]: x then y as four little-endian registers (circuits/circom/utils.ts pointToCircuitValue); identity = zeros */
int plume_recover_batch(plume_ctx* ctx, int version, int format, size_t n,
                        const uint8_t* msgs, const uint64_t* msg_off,
                        const uint8_t* pk, const uint8_t* nullifier, const uint8_t* c, const uint8_t* s,
                        uint8_t* r_point, uint8_t* hashed_to_curve_r, uint8_t* hashed_to_curve, uint8_t* status);
int plume_recover_batch_device(plume_ctx* ctx, int version, int format, size_t n,
                               const uint8_t* msgs, const uint64_t* msg_off, size_t msgs_bytes,
                               const uint8_t* pk, const uint8_t* nullifier, const uint8_t* c, const uint8_t* s,
                               uint8_t* r_point, uint8_t* hashed_to_curve_r, uint8_t* hashed_to_curve, uint8_t* status, void* stream);

/* ---- Ethereum addresses of public keys (Keccak-256)  (library 0.11) ------------------------------------------
 * The identity an application holds for an Ethereum key is its 20-byte address: allow-lists (airdrop snapshots, voter rolls, token holders) are lists of addresses and
 * ERC-7524's wallet call names the signing key by its address.  For item i:
 *     address = Keccak-256(x || y)[12..32)      x || y: the 64 big-endian bytes of the affine point
 * Keccak-256 is the ORIGINAL padding (0x01 ... 0x80, rate 136), not SHA3-256.
 *   pk        PLUME_ETH_PK_AFFINE64: 64 B x||y as everywhere else; PLUME_ETH_PK_SEC1: 33 B 02|03||x.  A key is valid when its coordinates are below p and the point is on the
 *             curve and is NOT the identity: the all-zero record is PLUME_ETH_INVALID here, because an Ethereum key has no identity, although plume_verify_batch accepts
 *             it as a public key.  SEC1 input is invalid when the prefix byte is not 02 / 03 (00, the verifier's identity, included), when x >= p, or when x^3 + 7 has no
 *             square root.
 *   expect    optional (NULL): the address each key is claimed to have, ALWAYS 20 raw bytes per item whatever addr_format is.
 *   address   optional when expect is given: PLUME_ETH_ADDR_RAW20 20 B; PLUME_ETH_ADDR_RECORD64 64 B = 44 zero bytes, then the address -- a record plume_nullset_* and
 *             plume_nullifier_first_occurrence take as is (an allow-list is a nullifier set of such records, the gate is plume_nullset_contains);
 *             PLUME_ETH_ADDR_EIP55 42 ASCII bytes "0x" + 40 hex digits with the EIP-55 mixed-case checksum (a second Keccak-256 over the 40 lower-case digits; digit i is
 *             upper-cased iff nibble i of that hash is at least 8), no terminator.
 *   status    optional when address is given.  An invalid item has status PLUME_ETH_INVALID and an all-zero record whatever expect holds.
 * At least one of address and status must be given.  The call needs no table and no workspace and builds none: a context that only ever computes addresses never pays for
 * the verifier's 1 GiB window table.  The host form cuts the batch into pieces of at most plume_set_chunk items and splits it over the shards of a plume_init_multi
 * context, as plume_scalars_to_sec1_der_batch does; the device form (a single-device context) takes any n < 2^32 - 16, enqueues one kernel on `stream` and does not
 * synchronise.  The arrays may sit at any byte offset; a 16-byte aligned pk array of 64-byte records is read with 16-byte loads. */
#define PLUME_ETH_MISMATCH 0   /* address computed; differs from expect[i] */
#define PLUME_ETH_MATCH    1   /* address computed; expect is NULL or equals it */
#define PLUME_ETH_INVALID  3   /* pk is not a non-identity curve point in the given format; the output record is all zero */
#define PLUME_ETH_PK_AFFINE64 0   /* 64 B x||y big-endian, as everywhere else */
#define PLUME_ETH_PK_SEC1     1   /* 33 B 02|03||x */
#define PLUME_ETH_ADDR_RAW20    0 /* 20 B */
#define PLUME_ETH_ADDR_RECORD64 1 /* 64 B: 44 zero bytes, then the 20 address bytes -- a record plume_nullset_* / plume_nullifier_first_occurrence take as is */
#define PLUME_ETH_ADDR_EIP55    2 /* 42 ASCII bytes: "0x" + 40 hex digits with the EIP-55 mixed-case checksum; no terminator */
int plume_eth_address_batch(plume_ctx* ctx, int pk_format, int addr_format, size_t n, const uint8_t* pk, const uint8_t* expect, uint8_t* address, uint8_t* status);
int plume_eth_address_batch_device(plume_ctx* ctx, int pk_format, int addr_format, size_t n, const uint8_t* pk, const uint8_t* expect, uint8_t* address, uint8_t* status,
                                   void* stream);

/* ---- public keys and addresses from ECDSA signatures (ecrecover)  (library 0.12) --------------------------------
 * Every other call here takes a public key, and an application holds addresses: the only place the key of an Ethereum account is ever published is an ECDSA signature by
 * that account -- a transaction, a personal_sign, the "proof of ECDSA" the reference's README pairs with a PLUME proof.  This call recovers the key, and its address, from
 * such signatures: building the anonymity set of a list of addresses, or binding a claimed pk to an account, without leaving the GPU.  The semantics are those of Ethereum's
 * ecrecover precompile, except that v is ONE byte and may also be 0 or 1.  For item i:
 *   v        0, 1, 27 or 28: the parity of R's y is v & 1 for 0 / 1, v - 27 for 27 / 28.  Any other byte is invalid; EIP-155 values are the caller's to normalise.  The two
 *            candidates with x = r + n are not produced, as in the precompile.
 *   r, s     32 big-endian bytes each, 1 <= r < n and 1 <= s < n, else invalid.  With PLUME_ECDSA_LOW_S in flags (the EIP-2 rule for transactions) s > (n - 1) / 2 is
 *            invalid as well.
 *   R        the curve point with x = r and y of the given parity; no square root means invalid.
 *   hash     any 32 bytes: z = hash mod n.
 *   Q        r^-1 (s R - z G) = u1 G + u2 R with u1 = -z r^-1 and u2 = s r^-1 (mod n); Q = identity means invalid.
 *   address  Keccak-256(Qx || Qy)[12..32).
 *   expect   optional (NULL): the address each signer is claimed to have, ALWAYS 20 raw bytes per item whatever addr_format is, as for plume_eth_address_batch.
 *   pk       optional: PLUME_ETH_PK_AFFINE64 64 B x||y, or PLUME_ETH_PK_SEC1 33 B 02|03||x.
 *   address  optional: PLUME_ETH_ADDR_RAW20, PLUME_ETH_ADDR_RECORD64 (a record plume_nullset_* take as is) or PLUME_ETH_ADDR_EIP55, byte for byte what
 *            plume_eth_address_batch writes for the recovered key.
 *   status   optional: PLUME_ECDSA_MATCH -- recovered, and the address equals expect[i] or no expect was given; PLUME_ECDSA_MISMATCH -- recovered, and the address
 *            differs: pk and address are written all the same; PLUME_ECDSA_INVALID -- every record of the item is all zero, whatever expect holds.
 * At least one of pk, address and status must be given.  Unknown flags bits or formats return PLUME_ERR_ARG; n = 0 is a successful no-op.  Everything here is public data.
 * The call builds the comb of G on its first use (252 MiB, shared with the signer) and never the verifier's 1 GiB window table; its workspace is the context's.  The host
 * form cuts the batch into pieces of at most plume_set_chunk items and splits it over the shards of a plume_init_multi context; the device form (a single-device context,
 * n at most the chunk size) enqueues on `stream`, waits for and leaves behind the workspace event like plume_verify_batch_device, honours plume_set_sub_batches and does
 * not synchronise.  The arrays may sit at any byte offset; 16-byte aligned arrays of 64-byte records are written with 16-byte stores.  With stage timing on the stages are
 * "ecdsa_prepare", "tables", "ecdsa_mul", "to_affine", "ecdsa_finalize". */
#define PLUME_ECDSA_MISMATCH 0   /* key recovered; its address differs from expect[i] */
#define PLUME_ECDSA_MATCH    1   /* key recovered; expect is NULL or equals its address */
#define PLUME_ECDSA_INVALID  3   /* v, r or s out of range, no point with x = r, or Q is the identity; every output record is all zero */
#define PLUME_ECDSA_LOW_S    1   /* flags bit 0: s > (n - 1) / 2 is invalid (EIP-2) */
int plume_ecdsa_recover_batch(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* hash, const uint8_t* r, const uint8_t* s, const uint8_t* v,
                              const uint8_t* expect, uint8_t* pk, uint8_t* address, uint8_t* status);
int plume_ecdsa_recover_batch_device(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* hash, const uint8_t* r, const uint8_t* s,
                                     const uint8_t* v, const uint8_t* expect, uint8_t* pk, uint8_t* address, uint8_t* status, void* stream);

/* ---- the digest a wallet signs: Keccak-256 of ragged messages, EIP-191  (library 0.13) ---------------------------
 * plume_ecdsa_recover_batch and plume_ecdsa_sign_batch take a 32-byte digest; this call makes it from the message.  Message i is msgs[msg_off[i] .. msg_off[i + 1])
 * (n + 1 offsets, as everywhere else; item lengths below 2^32), and hash32 gets 32 bytes per item:
 *   PLUME_ETH_HASH_KECCAK256   Keccak-256(msg): the ORIGINAL padding (0x01 ... 0x80, rate 136), not SHA3-256
 *   PLUME_ETH_HASH_EIP191      Keccak-256("\x19Ethereum Signed Message:\n" || decimal(len(msg)) || msg): what personal_sign / eth_sign hash.  The prefix is 26 bytes; the
 *                              length is ASCII decimal without leading zeros ("0" for the empty message)
 * Any other mode returns PLUME_ERR_ARG; n = 0 is a successful no-op.  Like plume_eth_address_batch the call needs no table and no workspace and everything is public
 * data.  The host form cuts the batch into pieces of at most plume_set_chunk items and splits it over the shards of a plume_init_multi context; offsets that decrease
 * return PLUME_ERR_ARG there.  The device form (a single-device context) is ONE kernel enqueued on `stream` with no synchronisation; an item whose offsets decrease or
 * reach past msgs_bytes hashes the empty message and never reads msgs, as in the other device forms.  msgs and hash32 may sit at any byte offset (msg_off: 8-byte
 * aligned); message bytes are read with aligned 8-byte loads where the words lie inside msgs.  With stage timing on the stage is "eth_message_hash". */
#define PLUME_ETH_HASH_KECCAK256 0
#define PLUME_ETH_HASH_EIP191    1
int plume_eth_message_hash_batch(plume_ctx* ctx, int mode, size_t n, const uint8_t* msgs, const uint64_t* msg_off, uint8_t* hash32);
int plume_eth_message_hash_batch_device(plume_ctx* ctx, int mode, size_t n, const uint8_t* msgs, const uint64_t* msg_off, size_t msgs_bytes, uint8_t* hash32, void* stream);

/* ---- deterministic ECDSA signatures with a recovery id  (library 0.13) -------------------------------------------
 * The signer's counterpart of plume_ecdsa_recover_batch: the personal_sign, the transaction signature, the "proof of ECDSA" that publishes a key -- produced where the
 * keys already are, so that sk never has to leave the engine for a CPU library.  The result is byte-identical to what geth, ethers and libsecp256k1 produce for the same
 * key and digest.  For item i, with hash 32 bytes, sk 32 big-endian bytes and aux NULL or 32 bytes per item:
 *   z     int(hash) mod n.
 *   k     RFC 6979 section 3.2 with HMAC-SHA-256, q = n, x = sk as given, h1 = hash: plain RFC 6979 over the digest itself, NOT the "PLUME-RFC6979" preimage of
 *         plume_sign_batch_rfc6979.  aux non-NULL appends its 32 bytes in steps d and f (section 3.6), exactly as there.  The nonce loop stops after the same
 *         PLUME_NONCE_ROUNDS (16) candidates.  k is derived, used and wiped on the device; no call returns it.
 *   R     k G;  r = R.x mod n;  s = k^-1 (z + r sk) mod n.
 *   low s ALWAYS: if s > (n - 1) / 2 then s <- n - s and the parity flips (EIP-2; what plume_ecdsa_recover_batch accepts under PLUME_ECDSA_LOW_S).
 *   v     the parity of R.y after that flip: 0 or 1, or 27 or 28 with PLUME_ECDSA_SIGN_V27 in flags.
 *   status  0: signed.  PLUME_STATUS_BAD_SCALAR: sk outside [1, n - 1], or the nonce cap ran out.  PLUME_STATUS_IDENTITY: a degenerate outcome -- r = 0, s = 0, or
 *         R.x >= n.  The last one is a valid signature elsewhere, with a recovery id of 2 or 3 that the one-byte v here and plume_ecdsa_recover_batch do not represent; its
 *         probability is about 2^-128 and there is NO retry with another nonce (that would leave RFC 6979).  Any non-zero status writes all-zero r, s, v.
 * Unknown flags bits return PLUME_ERR_ARG; n = 0 is a successful no-op; all four outputs are required.  Outputs are bit-identical at every plume_set_sign_uniform level.
 * Everything that touches sk, k, k^-1 or z + r sk is select-based at every level: the reduction of R.x, the low-s negation, the zeroing of failed items; the inversion of
 * k is the fixed-iteration safegcd.  The comb's digit-dependent schedule and addresses are what plume_set_sign_uniform says of r G in plume_sign_batch.
 * plume_set_sign_selfcheck(ctx, 1) covers this entry point: the signatures are staged in the context together with sk G, the stages of plume_ecdsa_recover_batch recover a
 * key from every staged (hash, r, s, v), and one release kernel writes the caller's arrays -- byte-identical to mode 0 where the recovered key is sk G, all zero with
 * PLUME_STATUS_SELFCHECK_FAILED for any other item whose own status was 0, and as mode 0 writes it for an item with a status of its own.  The staging is wiped.
 * Routing is that of plume_sign_batch_rfc6979*: the host form runs the signer's pipeline (pieces, plume_set_chunk, both host lanes, the shards of a plume_init_multi context;
 * sk and aux are staged and wiped like the signer's); the device form (a single-device context, n at most the chunk size) enqueues on `stream`, waits for and leaves behind
 * the workspace event, honours plume_set_sub_batches and plume_set_in_flight and does not synchronise.  The call builds the comb of G (or the level-2 scanned table) on
 * first use and never the verifier's 1 GiB window table.  The arrays may sit at any byte offset.  With stage timing on the stages are "ecdsa_sign_nonce",
 * "ecdsa_sign_gmul", "to_affine", "ecdsa_sign_finalize"; with the self-check on, the stages of plume_ecdsa_recover_batch and "ecdsa_sign_release" follow them. */
#define PLUME_ECDSA_SIGN_V27 1   /* flags bit 0: v is 27 or 28 instead of 0 or 1 */
int plume_ecdsa_sign_batch(plume_ctx* ctx, int flags, size_t n, const uint8_t* hash, const uint8_t* sk, const uint8_t* aux, uint8_t* r, uint8_t* s, uint8_t* v,
                           uint8_t* status);
int plume_ecdsa_sign_batch_device(plume_ctx* ctx, int flags, size_t n, const uint8_t* hash, const uint8_t* sk, const uint8_t* aux, uint8_t* r, uint8_t* s, uint8_t* v,
                                  uint8_t* status, void* stream);

/* ---- the senders of raw Ethereum transactions  (library 0.14) ----------------------------------------------------
 * An account publishes its key in the signatures it makes, and by far the most of those are transactions.  These calls take signed transactions as they travel on the
 * wire -- item i is txs[tx_off[i] .. tx_off[i + 1]), n + 1 offsets as everywhere else, item lengths below 2^32 -- and give what plume_ecdsa_recover_batch takes (parse)
 * or the sender itself (sender).  THIS IS A SENDER RECOVERY, NOT A CONSENSUS DECODER: the envelope, the top-level framing and the signature fields are checked; the
 * contents of every other field, the nested access, blob-hash and authorization lists included, are skipped by their header and copied verbatim into the hash.  A
 * transaction a node accepts gets the same sender here; one a node rejects for an inner field may still get one.
 *   RLP       first byte 00-7f: a one-byte string, the byte itself; 80-b7: a string of b - 0x80 bytes; b8-bf: b - 0xb7 big-endian length bytes, then the string; c0-f7: a
 *             list with a payload of b - 0xc0 bytes; f8-ff: a list with b - 0xf7 length bytes.  Canonical: a one-byte string below 0x80 uses the single-byte form, the long
 *             form only serves lengths above 55, length bytes have no leading zero.  A canonical integer is a string without a leading zero byte; zero is the empty string.
 *   envelope  first byte >= 0xc0: legacy, tx_type 0, one list that covers the item exactly, 9 items (nonce, gasPrice, gasLimit, to, value, data, v, r, s).  First byte 01,
 *             02, 03, 04 (EIP-2930, EIP-1559, EIP-4844 in its canonical form, EIP-7702): tx_type is that byte, the rest is one list that covers it exactly, with 11, 12, 14,
 *             13 items, the first chainId, the last three yParity, r, s.  Anything else (the empty item, 00, 05-7f, 80-bf) is invalid, and so is the EIP-4844 network
 *             wrapper, by its item count.
 *   framing   the outer header and every top-level header canonical; every item inside the payload; the items tile the payload exactly, with the exact count; v / yParity,
 *             r, s and a typed chainId canonical integers; r and s at most 32 bytes; legacy v and typed chainId at most 8 bytes; yParity 0 or 1.
 *   v         legacy: 27 or 28 -> parity v - 27, chain_id 0 (unprotected); v >= 37 -> parity (v - 35) & 1, chain_id (v - 35) >> 1 (1 .. 2^63 - 18); any other value, 35
 *             and 36 included, is invalid.  Typed: the parity is yParity, chain_id the first field (below 2^64).
 *   hash32    with body = the input from the first top-level item to the start of v / yParity and list(x) = the canonical list header of len(x), then x:
 *             Keccak-256(list(body)) for an unprotected legacy item, Keccak-256(list(body || rlp_int(chain_id) || 80 80)) under EIP-155, Keccak-256(type || list(body))
 *             for a typed one.
 *   r, s      32 big-endian bytes, left-padded;  v: one byte, 0 or 1;  chain_id: uint64_t;  tx_type: one byte.
 *   status    PLUME_ETH_TX_OK, or PLUME_ETH_TX_INVALID: the item breaks a rule above and EVERY record of it is zero.  In the device forms an item whose offsets decrease or
 *             reach past txs_bytes is invalid and never reads txs.
 * 1 <= r, s < n, the low-s rule and "no point with x = r" are NOT checked by the parse: they belong to the recover stages.  The transaction id is Keccak-256 of the raw
 * item: plume_eth_message_hash_batch with PLUME_ETH_HASH_KECCAK256 over the same txs / tx_off gives it, so there is no output for it here.
 * plume_eth_tx_parse_batch: hash32, r, s and v are required, chain_id, tx_type and status optional.  No table, no workspace.  The host form routes exactly like
 * plume_eth_message_hash_batch (pieces of at most plume_set_chunk items, the shards of a plume_init_multi context, decreasing offsets return PLUME_ERR_ARG); the device form
 * is ONE kernel (k_eth_tx_parse) on `stream` with no synchronisation.  With stage timing on the stage is "eth_tx_parse".
 * plume_eth_tx_sender_batch: k_eth_tx_parse into staging the context owns, then the unchanged stages of plume_ecdsa_recover_batch on the staged (hash, r, s, v).  flags,
 * pk_format, addr_format, expect, pk, address and status (PLUME_ECDSA_MATCH / MISMATCH / INVALID) mean what they mean there; PLUME_ECDSA_LOW_S is the right setting for
 * anything after Homestead.  An item invalid in the framing stages r = 0, so it leaves the recover stages invalid with zero records.  chain_id and tx_type (optional) report
 * the FRAMING: they are zero only for framing-invalid items, and are written as parsed for an item whose signature then fails to recover.  Routing, the workspace event,
 * plume_set_sub_batches and the chunk limit of the device form are those of plume_ecdsa_recover_batch*.  With stage timing on the stages are "eth_tx_parse" followed by the
 * five recover stages.  The call builds the comb of G on first use and never the 1 GiB window table.
 * Both: n = 0 is a successful no-op; unknown flags or formats return PLUME_ERR_ARG; the arrays may sit at any byte offset (tx_off and chain_id: 8-byte aligned);
 * everything is public data. */
#define PLUME_ETH_TX_OK      1
#define PLUME_ETH_TX_INVALID 3
int plume_eth_tx_parse_batch(plume_ctx* ctx, size_t n, const uint8_t* txs, const uint64_t* tx_off, uint8_t* hash32, uint8_t* r, uint8_t* s, uint8_t* v, uint64_t* chain_id,
                             uint8_t* tx_type, uint8_t* status);
int plume_eth_tx_parse_batch_device(plume_ctx* ctx, size_t n, const uint8_t* txs, const uint64_t* tx_off, size_t txs_bytes, uint8_t* hash32, uint8_t* r, uint8_t* s,
                                    uint8_t* v, uint64_t* chain_id, uint8_t* tx_type, uint8_t* status, void* stream);
int plume_eth_tx_sender_batch(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* txs, const uint64_t* tx_off, const uint8_t* expect,
                              uint8_t* pk, uint8_t* address, uint64_t* chain_id, uint8_t* tx_type, uint8_t* status);
int plume_eth_tx_sender_batch_device(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* txs, const uint64_t* tx_off, size_t txs_bytes,
                                     const uint8_t* expect, uint8_t* pk, uint8_t* address, uint64_t* chain_id, uint8_t* tx_type, uint8_t* status, void* stream);

/* ---- signing raw Ethereum transactions: unsigned payload in, wire bytes out  (library 0.16) ------------------------
 * The producer of what the 0.14 calls parse.  Item i is txs[tx_off[i] .. tx_off[i + 1]), n + 1 offsets as everywhere else: the UNSIGNED serialization wallets pass around,
 * exactly the bytes whose Keccak-256 the sender signs.  THIS IS A SIGNER OF WELL-FRAMED PAYLOADS, NOT A CONSENSUS ENCODER: the envelope, the outer header and every
 * top-level header must be canonical and tile the payload exactly, by the rules stated for the parser above; inner fields are skipped by their header and copied verbatim.
 *   input     legacy, unprotected: one list that covers the item, 6 items (nonce, gasPrice, gasLimit, to, value, data).  Legacy, EIP-155: one list, 9 items, the seventh
 *             chainId, a canonical integer in 1 .. 2^63 - 18 (the range the parser accepts: v fits 64 bits), the eighth and ninth each exactly the empty string 80; nine
 *             items with anything else in the last three are invalid (so a signed transaction given as input is).  Typed: first byte 01, 02, 03 or 04, then one list that
 *             covers the rest, with 8, 9, 11 or 10 items (the signed form's count less three), the first chainId, a canonical integer of at most 8 bytes.
 *   hash      Keccak-256(item): the whole item, no prefix, no suffix.
 *   signature exactly plume_ecdsa_sign_batch on that hash: RFC 6979 over the digest, aux (optional, 32 bytes per item) hedges it, always low s, parity 0 / 1, the same
 *             nonce cap, no retry.
 *   output    with body = the input from the first top-level item to the end of the last unsigned field (EIP-155: to the start of the chainId item) and list(x) the
 *             canonical list header of len(x), then x:
 *                 legacy, unprotected   list(body || rlp_int(27 + parity) || rlp_int(r) || rlp_int(s))
 *                 legacy, EIP-155       list(body || rlp_int(35 + 2 chainId + parity) || rlp_int(r) || rlp_int(s))
 *                 typed                 type || list(body || rlp_int(parity) || rlp_int(r) || rlp_int(s))
 *             integers canonical: no leading zero byte, zero is 80, a value below 0x80 is its own byte.
 *   slots     nothing depends on lengths that are only known after signing: slot i starts at out + (tx_off[i] - tx_off[0]) + 68 i and is len_i + 68 bytes long;
 *             out_len[i] (uint32_t) is the signed length and the slot's bytes beyond it are written as zero, so whole buffers compare byte for byte.  out needs
 *             tx_off[n] - tx_off[0] + 68 n bytes: plume_eth_tx_sign_out_bytes(n, tx_off[n] - tx_off[0]).  Why 68 (PLUME_ETH_TX_SIGN_GROWTH): the payload gains at most
 *             1 + 33 + 33 bytes; an EIP-155 item trades rlp_int(chainId) 80 80 for rlp_int(v), at most two bytes longer than rlp_int(chainId), never a net gain; a growth
 *             of at most 67 crosses at most one of the header thresholds 55/56, 255/256, 65535/65536, so the list header gains at most one byte.
 *   records   (each optional) hash32, r, s: 32 bytes per item; v: the parity, 0 / 1; chain_id: uint64_t (0 for an unprotected legacy item); tx_type: one byte.  They are
 *             what plume_eth_tx_parse_batch would report for the item written, so a caller need not parse its own output again.
 *   status    (required) the sign status bits.  0: signed.  PLUME_STATUS_BAD_SCALAR, PLUME_STATUS_IDENTITY, PLUME_STATUS_SELFCHECK_FAILED: as in plume_ecdsa_sign_batch.
 *             PLUME_STATUS_BAD_TX: the item breaks a rule above; or, in the device form, its offsets decrease or reach past txs_bytes (such an item never reads txs and,
 *             having no slot, writes no byte of out), or its slot reaches past out_bytes (it then writes no byte of out either).  BAD_TX is reported alone, whatever the
 *             key is.  One outcome is added to PLUME_STATUS_IDENTITY: chainId 2^63 - 18 signed with parity 1 has v = 2^64, which 64 bits -- and the parser -- do not
 *             hold; like R.x >= n it is a recovery id without a representation, and there is no retry.  Any non-zero status: an all-zero slot, out_len = 0 and zero in
 *             every optional record.
 * Device side: k_eth_tx_sign_frame (framing and hash, into staging the context owns), the unchanged stages of plume_ecdsa_sign_batch on the staged hash --
 * plume_set_sub_batches, plume_set_sign_uniform, plume_set_sign_selfcheck and the chunk limit apply as they do there --, k_eth_tx_sign_assemble (one lane per item writes
 * exactly its slot).  The staged signatures are wiped behind it: what was signed for an item that reports a status is never released.  With stage timing on the stages are
 * "eth_tx_sign_frame", the signer's own, "eth_tx_sign_assemble".  The device form needs a single-device context and n <= the chunk size, waits for and leaves the
 * workspace event, builds the signer's tables on first use (plus the comb with the self-check on), never the 1 GiB window table, and does not synchronise; with device
 * offsets that are not non-decreasing the slots of sound items may overlap, and what an overlap holds is unspecified (nothing outside out_bytes is ever written).  The host
 * form is a serial call like plume_eth_tx_sender_batch: pieces of at most plume_set_chunk items, the shards of a plume_init_multi context, sk and aux wiped from the staging
 * behind the kernels.  Decreasing offsets anywhere in tx_off[0 .. n] return PLUME_ERR_ARG before anything is staged or written: the offsets of the whole call place every
 * piece's and every shard's share of out.
 * Both: flags must be 0 (unknown bits return PLUME_ERR_ARG); n = 0 is a successful no-op; byte arrays may sit at any byte offset; tx_off and chain_id are 8-byte aligned,
 * out_len 4-byte aligned.  The transaction id is Keccak-256 of the signed item: plume_eth_message_hash_batch over the compacted output gives it. */
#define PLUME_ETH_TX_SIGN_GROWTH 68
size_t plume_eth_tx_sign_out_bytes(size_t n, uint64_t txs_bytes);
int plume_eth_tx_sign_batch(plume_ctx* ctx, int flags, size_t n, const uint8_t* txs, const uint64_t* tx_off, const uint8_t* sk, const uint8_t* aux, uint8_t* out,
                            uint32_t* out_len, uint8_t* hash32, uint8_t* r, uint8_t* s, uint8_t* v, uint64_t* chain_id, uint8_t* tx_type, uint8_t* status);
int plume_eth_tx_sign_batch_device(plume_ctx* ctx, int flags, size_t n, const uint8_t* txs, const uint64_t* tx_off, size_t txs_bytes, const uint8_t* sk, const uint8_t* aux,
                                   uint8_t* out, size_t out_bytes, uint32_t* out_len, uint8_t* hash32, uint8_t* r, uint8_t* s, uint8_t* v, uint64_t* chain_id,
                                   uint8_t* tx_type, uint8_t* status, void* stream);

/* ---- BIP-32 child keys, public keys and addresses  (library 0.17) ------------------------------------------------
 * Wallets, custodians and test networks hold one seed or one account node, not an array of raw keys.  These calls derive the keys where the signers use them:
 * the child_sk of the device form is the sk pointer plume_ecdsa_sign_batch_device, plume_eth_tx_sign_batch_device and plume_sign_batch*_device take, and the address
 * records are what plume_nullset_* and plume_merkle_leaf_batch take.
 *   I = HMAC-SHA512(key = c_par, data), IL = I[0:32], IR = I[32:64], the index i as four big-endian bytes, serP the 33-byte SEC1 compressed form:
 *   private   data = 00 || ser256(k_par) || i when i >= 2^31 (hardened), serP(k_par G) || i otherwise;  k_i = IL + k_par mod n, c_i = IR
 *   public    non-hardened only: data = serP(K_par) || i;  K_i = IL G + K_par, c_i = IR
 *   master    I = HMAC-SHA512(key = "Bitcoin seed", seed), 16 <= seed_len <= 64, the same for all items;  k = IL, c = IR
 * Item i walks `depth` levels (1 .. PLUME_HD_MAX_DEPTH): the indices path[i][0 .. depth), uint32_t in host order, row-major.  flags: PLUME_HD_SHARED_PARENT -- the parent
 * arrays hold ONE record, used for every item; PLUME_HD_SHARED_PATH -- path holds ONE row.  pk_format / addr_format are PLUME_ETH_PK_* / PLUME_ETH_ADDR_*: parent_pk
 * and child_pk are in pk_format, address in addr_format.  child_chain32, child_pk (private form) and address may be NULL.
 *   status    (required) 0: derived.  PLUME_STATUS_BAD_SCALAR: parent sk outside [1, n - 1], or parent pk not a non-identity curve point in the given format.
 *             PLUME_STATUS_HD_NO_KEY, PLUME_STATUS_HD_HARDENED: above.  The first level that fails decides.  An item with any non-zero status has every output record
 *             all zero; a zero sk fed on into a signer reports PLUME_STATUS_BAD_SCALAR there.
 * Argument errors return PLUME_ERR_ARG with nothing written: depth outside 1 .. PLUME_HD_MAX_DEPTH, unknown flag bits, seed_len outside 16 .. 64, an unknown format, a
 * null required array.  n = 0 is a successful no-op.  Arrays may sit at any byte offset.
 * Device side, one lane per item: the private form runs, for every level and once more at the end, k G by the signer's comb at the context's uniform level
 * (plume_set_sign_uniform) and the batched conversion to affine -- for EVERY item, hardened or not, so no lane's work depends on its path --, then the HMAC and the tweak;
 * the hardened or the public preimage is chosen by select on the index bit, and the range check, the reduction, zero detection and the zeroing of a failed item are
 * selects too.  The public form hashes serP(K), multiplies IL (public) by the comb and adds K.  k, the chain codes and the images of k G between the levels live in
 * staging the context owns and are wiped on the call's stream behind the last kernel, on failure paths too.  There is no self-check for derivation.  With stage timing on
 * the stages are "hd_master"; "hd_priv_load", "hd_gmul", "to_affine", "hd_priv_step", "hd_finish"; "hd_pub_load", "hd_pub_step".  The device forms need a single-device
 * context and n <= the chunk size, wait for and leave the workspace event (master: no workspace), build the signer's table on first use and do not synchronise.  The host
 * forms are serial calls: pieces of at most plume_set_chunk items, the shards of a plume_init_multi context; sk, chain codes and seeds -- going in and coming out -- are
 * wiped from the staging behind their use or their download; a shared parent or path is uploaded once per piece or once per call. */
#define PLUME_HD_MAX_DEPTH 8
#define PLUME_HD_SHARED_PARENT 1 /* flags bit 0: the parent arrays hold ONE record, used for every item */
#define PLUME_HD_SHARED_PATH 2   /* flags bit 1: path holds ONE row of `depth` indices, used for every item */
int plume_hd_master_batch(plume_ctx* ctx, size_t n, const uint8_t* seed, size_t seed_len, uint8_t* sk32, uint8_t* chain32, uint8_t* status);
int plume_hd_master_batch_device(plume_ctx* ctx, size_t n, const uint8_t* seed, size_t seed_len, uint8_t* sk32, uint8_t* chain32, uint8_t* status, void* stream);
int plume_hd_derive_priv_batch(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* parent_sk32, const uint8_t* parent_chain32,
                               const uint32_t* path, size_t depth, uint8_t* child_sk32, uint8_t* child_chain32, uint8_t* child_pk, uint8_t* address, uint8_t* status);
int plume_hd_derive_priv_batch_device(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* parent_sk32, const uint8_t* parent_chain32,
                                      const uint32_t* path, size_t depth, uint8_t* child_sk32, uint8_t* child_chain32, uint8_t* child_pk, uint8_t* address,
                                      uint8_t* status, void* stream);
int plume_hd_derive_pub_batch(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* parent_pk, const uint8_t* parent_chain32,
                              const uint32_t* path, size_t depth, uint8_t* child_pk, uint8_t* child_chain32, uint8_t* address, uint8_t* status);
int plume_hd_derive_pub_batch_device(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* parent_pk, const uint8_t* parent_chain32,
                                     const uint32_t* path, size_t depth, uint8_t* child_pk, uint8_t* child_chain32, uint8_t* address, uint8_t* status, void* stream);

/* ---- BIP-39 seeds: PBKDF2-HMAC-SHA512, one output block, for a batch  (library 0.18) ----------------------------------
 * A wallet holds a mnemonic sentence, not a seed: seed = PBKDF2-HMAC-SHA512(password = the sentence, salt = "mnemonic" || passphrase, 2048 iterations, 64 bytes), 4096
 * compressions per item, where a BIP-32 step costs four.  This call makes the seeds where plume_hd_master_batch_device takes them, so that "mnemonic in, addresses and
 * signed transactions out" is one chain of device calls and neither a seed nor a key is ever made in host memory.
 *   U_1 = HMAC(P, S || 00000001), U_j = HMAC(P, U_(j-1)), T_1 = U_1 ^ .. ^ U_iterations (RFC 8018); out[i] = T_1[0 .. dklen), 1 <= dklen <= 64.  Only T_1 is computed:
 *   a larger dklen returns PLUME_ERR_ARG, it is not truncated silently.
 *   password  item i's is pw[pw_off[i] .. pw_off[i + 1]): n + 1 offsets, any length from 0 up.  HMAC's rule applies: up to 128 bytes zero-padded, a longer one replaced
 *             by its SHA-512 (a 24-word sentence usually is longer).
 *   salt      salt_len bytes per item, 0 .. PLUME_KDF_MAX_SALT, the same length for every item; NULL is allowed when salt_len is 0.  PLUME_KDF_SHARED_SALT: salt holds
 *             ONE record, used for every item.  PLUME_KDF_BIP39: the eight bytes "mnemonic" are put in front of every item's salt on the device.  There is no ragged
 *             per-item salt: a passphrase is absent or one per batch in practice.
 *   status    (required) 0: derived.  PLUME_STATUS_KDF_BAD_INPUT (device form only): pw_off[i + 1] < pw_off[i] or pw_off[i + 1] > pw_bytes; that item reads no byte of
 *             pw and its record is all zero, its neighbours are derived.  The host form returns PLUME_ERR_ARG for decreasing offsets anywhere, before anything is
 *             staged or written.
 * Argument errors return PLUME_ERR_ARG with nothing written: iterations outside 1 .. PLUME_KDF_MAX_ITERATIONS (a guard against a typo that queues hours of work, not a
 * measured figure), dklen or salt_len out of range, unknown flag bits, a null required array.  n = 0 is a successful no-op.  Arrays may sit at any byte offset, pw_off
 * 8-byte aligned.  No byte outside [pw, pw + pw_bytes) and outside the salt and out arrays is read or written.
 * Device side, one lane per item: "kdf_key" (the password read once and hashed if long, the two HMAC midstates, U_1), "kdf_iter" (the remaining iterations, two
 * compressions each, enqueued in slices of 256 so that no dispatch of a large call runs for the whole derivation: once per slice in the stage list) and "kdf_finish".
 * Between them the midstates, U and T live in staging the context owns, 256 bytes per item, wiped on the call's stream behind the last kernel, on failure paths too.
 * Lengths are public: the lanes branch on and address by offsets, lengths, salt_len and the iteration count only, never by a byte of a password, a salt, a midstate or
 * U / T; a wavefront takes as long as its longest password needs to be read.  The device form needs a single-device context and n <= the chunk size, waits for and leaves
 * the workspace event, needs no table and does not synchronise.  The host form is a serial call: pieces of at most plume_set_chunk items, the shards of a plume_init_multi
 * context; the passwords, the salt and the output are wiped from the staging behind their use or their download.
 * Out of scope: the BIP-39 word list (sentence <-> entropy, checksum validation -- the seed derivation does not need it), dklen > 64, other PRFs.  A caller with non-ASCII
 * text normalises it (NFKD) before it hands over the bytes. */
#define PLUME_KDF_BIP39        1   /* flags bit 0: the salt of every item is "mnemonic" || salt (8 bytes put in front on the device) */
#define PLUME_KDF_SHARED_SALT  2   /* flags bit 1: salt holds ONE record of salt_len bytes, used for every item */
#define PLUME_KDF_MAX_SALT     256
#define PLUME_KDF_MAX_ITERATIONS (1u << 24)
#define PLUME_STATUS_KDF_BAD_INPUT 128
int plume_pbkdf2_sha512_batch(plume_ctx* ctx, int flags, size_t n, const uint8_t* pw, const uint64_t* pw_off, const uint8_t* salt, size_t salt_len, uint32_t iterations,
                              size_t dklen, uint8_t* out, uint8_t* status);
int plume_pbkdf2_sha512_batch_device(plume_ctx* ctx, int flags, size_t n, const uint8_t* pw, const uint64_t* pw_off, size_t pw_bytes, const uint8_t* salt, size_t salt_len,
                                     uint32_t iterations, size_t dklen, uint8_t* out, uint8_t* status, void* stream);

/* ---- Keccak Merkle allow-lists of addresses  (library 0.15) -------------------------------------------------------
 * An application that gates on a list of accounts usually publishes ONE 32-byte root and lets every claimant bring a proof.  These calls build that tree, hand out proofs
 * and check proofs against a root, in the form OpenZeppelin's StandardMerkleTree (@openzeppelin/merkle-tree) builds and MerkleProof.verify checks on chain.
 *   leaf       PLUME_MERKLE_LEAF_HASH32: the caller's 32 bytes as they are.  PLUME_MERKLE_LEAF_ADDRESS: Keccak-256(Keccak-256(0^12 || addr20)), the tree of ["address"].
 *              PLUME_MERKLE_LEAF_ADDRESS_UINT256: Keccak-256(Keccak-256(0^12 || addr20 || amount32)), amount32 big-endian: the tree of ["address", "uint256"].
 *              Addresses come as PLUME_ETH_ADDR_RAW20 (20 bytes per item) or PLUME_ETH_ADDR_RECORD64 (64 bytes per item: what plume_eth_address_batch,
 *              plume_ecdsa_recover_batch and plume_eth_tx_sender_batch write); a RECORD64 whose first 44 bytes are not zero is invalid.  PLUME_ETH_ADDR_EIP55 returns
 *              PLUME_ERR_ARG.  With HASH32 an item is 32 bytes and addr_format (still 0 or 1) and amount are ignored; amount is also ignored with ADDRESS.
 *   node       hash_pair(a, b) = Keccak-256(min(a, b) || max(a, b)), the 32-byte values compared as big-endian numbers.
 *   tree       n >= 1 leaves L[0 .. n) give tree[0 .. 2n - 1) of 32-byte nodes: tree[2n - 2 - i] = L[i], tree[i] = hash_pair(tree[2i + 1], tree[2i + 2]) for
 *              i = n - 2 .. 0; the root is tree[0].  With PLUME_MERKLE_SORT_LEAVES L is the input sorted ascending by (leaf bytes, input index) -- the index makes
 *              leaf_pos deterministic for duplicate leaves -- and without it L is the input order.  leaf_pos[j] is the tree index of input leaf j.
 *   proof      of tree index t: while t > 0 emit tree[t odd ? t + 1 : t - 1], then t = (t - 1) / 2.  Its length is floor(log2(t + 1)), at most
 *              plume_merkle_max_proof_len(n) = floor(log2(2n - 1)); when n is no power of two the leaves' proofs differ in length by one.
 *   verify     MerkleProof.processProof: h = leaf, h = hash_pair(h, p) for every proof element p in turn, compare h with the root.
 * plume_merkle_leaf_batch: leaf32[i] and status[i] (optional): PLUME_MERKLE_MATCH for a valid item, PLUME_MERKLE_INVALID and the all-zero leaf for an invalid one.
 * plume_merkle_tree_build: tree holds (2n - 1) * 32 bytes; leaf_pos (n words) is optional; n = 0 or n > 2^26 returns PLUME_ERR_ARG; unknown flag bits too.  The sort is a
 * bitonic network on the whole (leaf, index) key; its workspace, 36 bytes per leaf of n rounded up to a power of two, belongs to the context, so the device form joins the
 * workspace chain of the other device-resident calls.  The host form stages the whole tree on ONE device: a plume_init_multi context uses its first.
 * plume_merkle_proof_batch: the proofs of m tree indices pos[k] (any node, not only leaves), each in `depth` slots of 32 bytes (depth <= 64), unused slots zero;
 * proof_len[k] is one byte.  A pos[k] outside [0, 2n - 1) or a proof longer than depth gives PLUME_MERKLE_BAD_PROOF (255) and zero slots.  The host form uploads the tree
 * once and takes the indices in pieces of at most plume_set_chunk, on the first device of a plume_init_multi context.
 * plume_merkle_verify_batch: item k is an address (or, with HASH32, a leaf), its amount where the format has one, `depth` proof slots and proof_len[k]; the leaf is computed
 * in the same kernel, so the records of plume_eth_tx_sender_batch go in as they are.  status[k] (required): PLUME_MERKLE_MATCH the proof leads to root32,
 * PLUME_MERKLE_MISMATCH it does not, PLUME_MERKLE_INVALID an invalid item or proof_len[k] > depth.  The host form routes like plume_eth_address_batch (pieces of at most
 * plume_set_chunk items, the shards of a plume_init_multi context).
 * All: m = 0 (n = 0 for the leaf call) is a successful no-op; the device forms enqueue on `stream` and do not synchronise; byte arrays may sit at any byte offset (16-byte
 * aligned arrays take the vector loads), leaf_pos and pos need 4-byte alignment; with stage timing on the stages are "merkle_leaf", "merkle_sort", "merkle_place",
 * "merkle_levels" (one launch per depth of more than 256 parents), "merkle_top" (the depths above, one launch), "merkle_proof", "merkle_verify"; everything is public
 * data. */
#define PLUME_MERKLE_LEAF_HASH32          0
#define PLUME_MERKLE_LEAF_ADDRESS         1
#define PLUME_MERKLE_LEAF_ADDRESS_UINT256 2
#define PLUME_MERKLE_SORT_LEAVES          1
#define PLUME_MERKLE_MISMATCH  0
#define PLUME_MERKLE_MATCH     1
#define PLUME_MERKLE_INVALID   3
#define PLUME_MERKLE_BAD_PROOF 255
size_t plume_merkle_max_proof_len(size_t n);
int plume_merkle_leaf_batch(plume_ctx* ctx, int leaf_format, int addr_format, size_t n, const uint8_t* address, const uint8_t* amount, uint8_t* leaf32, uint8_t* status);
int plume_merkle_leaf_batch_device(plume_ctx* ctx, int leaf_format, int addr_format, size_t n, const uint8_t* address, const uint8_t* amount, uint8_t* leaf32, uint8_t* status,
                                   void* stream);
int plume_merkle_tree_build(plume_ctx* ctx, int flags, size_t n, const uint8_t* leaf32, uint8_t* tree, uint32_t* leaf_pos);
int plume_merkle_tree_build_device(plume_ctx* ctx, int flags, size_t n, const uint8_t* leaf32, uint8_t* tree, uint32_t* leaf_pos, void* stream);
int plume_merkle_proof_batch(plume_ctx* ctx, size_t n, const uint8_t* tree, size_t m, const uint32_t* pos, size_t depth, uint8_t* proof, uint8_t* proof_len);
int plume_merkle_proof_batch_device(plume_ctx* ctx, size_t n, const uint8_t* tree, size_t m, const uint32_t* pos, size_t depth, uint8_t* proof, uint8_t* proof_len,
                                    void* stream);
int plume_merkle_verify_batch(plume_ctx* ctx, int leaf_format, int addr_format, size_t m, const uint8_t* address_or_leaf, const uint8_t* amount, size_t depth,
                              const uint8_t* proof, const uint8_t* proof_len, const uint8_t* root32, uint8_t* status);
int plume_merkle_verify_batch_device(plume_ctx* ctx, int leaf_format, int addr_format, size_t m, const uint8_t* address_or_leaf, const uint8_t* amount, size_t depth,
                                     const uint8_t* proof, const uint8_t* proof_len, const uint8_t* root32, uint8_t* status, void* stream);

/* ---- persistent nullifier set: reject repeats across batches  (library 0.7) ----------------------------------
 * A consumer that verifies a STREAM of batches (a vote tally, a claim relayer, a rate limiter) must reject a nullifier it accepted any number of
 * batches ago.  A set S is a GPU-resident table of distinct 64-byte records that persists across calls (csrc/plume_nullset.h); records are opaque
 * and compared byte for byte, exactly as plume_nullifier_first_occurrence compares them (the all-zero identity is an ordinary record).
 *   insert   : fresh[i] = 1 iff live[i] (live NULL = all items), nullifier[i] was not in S before the call, and no live item j of the call with the
 *              same record has ids[j] < ids[i] (ids NULL = the position in the call; ids are distinct).  Afterwards S holds every live record;
 *              n_fresh (optional) = the number of 1s = the growth of |S|.  Equivalently: first-occurrence marking over every live item of every
 *              earlier insert into this set followed by this call's items, restricted to this call.  Independent of lane order, hash key and table size.
 *   contains : found[i] = 1 iff nullifier[i] is in S (read-only).
 *   size     : |S| and the table's capacity in slots (synchronises).   reserve: room for `items` records without growing.   clear: S = {}.
 *   export   : every record, in no particular order.  records NULL or cap < size: *count = size and nothing is written (PLUME_ERR_ARG when records
 *              is not NULL); otherwise the records and *count = size.  Export, then insert into another set, is the way to move or save a set.
 * Limits: n <= 2^30 per call; |S| <= 2^31; the table is at most half full and grows by itself to the next power of two >= 2 (|S| + n).  A request above
 * the limits returns PLUME_ERR_ARG before anything is allocated; a growth or allocation that fails returns PLUME_ERR_HIP and leaves the set unchanged and usable.
 * The set lives on the context's device (the first shard's for a plume_init_multi context) with a stream, buffers and "last operation" event of its own:
 * it never touches the context's workspace and may outlive the context.  The handle is used by one host thread at a time.
 * Device forms: every data pointer is a DEVICE pointer on the set's device, n_fresh (optional) is a device pointer to one uint64_t; the work is enqueued
 * on `stream` (NULL = the set's own stream), after the set's previous operation whatever stream that ran on; nothing synchronises, except when the host's
 * upper bound on |S| says the call might cross half the capacity -- the exact size is read then, and a growth synchronises once before it frees the old table.
 * Host forms synchronise before they return. */
int plume_nullset_create(plume_ctx* ctx, size_t reserve_items, void** set);
void plume_nullset_destroy(void* set);
int plume_nullset_reserve(void* set, size_t items);
int plume_nullset_clear(void* set);
int plume_nullset_size(void* set, uint64_t* size, uint64_t* capacity);
int plume_nullset_insert(void* set, size_t n, const uint8_t* nullifier, const uint8_t* live, const uint64_t* ids, uint8_t* fresh, uint64_t* n_fresh);
int plume_nullset_contains(void* set, size_t n, const uint8_t* nullifier, uint8_t* found);
int plume_nullset_export(void* set, size_t cap, uint8_t* records, uint64_t* count);
int plume_nullset_insert_device(void* set, size_t n, const uint8_t* nullifier, const uint8_t* live, const uint64_t* ids, uint8_t* fresh, uint64_t* n_fresh,
                                void* stream);
int plume_nullset_contains_device(void* set, size_t n, const uint8_t* nullifier, uint8_t* found, void* stream);

/* ---- measurement hooks (bench.py) -------------------------------------------------------------------------
 * Per-stage device time of the most recent *_device call on this context, measured with HIP events recorded on
 * the stream the kernels were launched on.  Fills up to `cap` entries: names[i] (static strings) and ms[i];
 * returns the number of stages, or a negative error.  Synchronises the recorded events. */
int plume_last_stage_times(plume_ctx* ctx, const char** names, float* ms, int cap);
/* The events behind plume_last_stage_times are recorded only on request (library 0.5; always before): a timing event between two kernels of a stream leaves the GPU idle
 * for about 6 us (rocprofv3 kernel trace of back-to-back 2^16-item verifies: 6.1 +- 0.2 us at each of the five stage boundaries, 0.0-0.2 us between kernels with no event
 * in between) -- 2 % of a 2^16-item call, 0.2 % of a 2^20-item one.  on = 1 before the call to be timed; env PLUME_STAGE_TIMES=1 sets the default of new contexts.  With
 * timing off plume_last_stage_times returns PLUME_ERR_ARG. */
int plume_set_stage_timing(plume_ctx* ctx, int on);
/* Measurement / test hook: the number of multi-scalar tasks (two per item) of the last verify call on this context whose unchecked addition chain met p == +-q and that
 * the second, dense launch redid with checked additions (k_verify_msm_redo).  Honest batches: 0.  Crafted items (pk = +-k G for small k with s = +-c, ...) file one or two
 * tasks each: that is all they cost -- their wavefront neighbours no longer wait for them.  Counts the last device-resident call (for a host-pointer call: its last piece;
 * for a multi-device context: the first shard).  A sign call with the self-check on (plume_set_sign_selfcheck) counts as a verify call here: its check's.  Synchronises with the device.
 * The redo list is scratch that the ECDSA recovery shares (plume_ecdsa_recover_batch*, and through it plume_eth_tx_sender_batch* and a self-checked plume_ecdsa_sign_batch* /
 * plume_eth_tx_sign_batch*): once such a call has run on the context (or lane) this hook would read, the verifier's counters are gone and the hook returns PLUME_ERR_ARG,
 * with a message that says so, instead of a count taken from another family's list.  The next verify call there re-arms it. */
int plume_last_redo_tasks(plume_ctx* ctx, uint64_t* count);
/* Measurement hook: the multi-scalar kernel the last verify call served by this context launched -- "k_verify_msm" (both equations in the long form), "k_verify_msm_s"
 * (equation 1 in the short form) or "k_verify_msm_pair" (half chains: small calls); NULL before the first verify.  Reports the same call as plume_last_stage_times; after a sign call with the self-check on, the kernel of its check.  A static string. */
const char* plume_last_msm_kernel(const plume_ctx* ctx);
/* Measurement hook: the shader clock (GHz) the multi-scalar kernel of the last verify call on this context ran at, sampled INSIDE that kernel -- one workgroup in 32 adds the
 * shader-clock cycles and the constant-rate wall-clock ticks it lived for to two counters.  kernel time x this clock = the kernel's duration in cycles, a figure that does not
 * move with the box's power / thermal state the way the time does.  Only when stage timing was on (plume_set_stage_timing) for THAT call; PLUME_ERR_ARG otherwise (an earlier call's sample is never handed out). */
int plume_last_msm_clock(plume_ctx* ctx, double* ghz);
/* VALU issue-rate microbenchmark (32 waves per CU, 8 independent chains per lane, `iters` x 8 instructions per lane):
 * returns operations per second chip-wide (<= 0 on error).  kind: 0 v_mad_u64_u32, 1 v_addc_co_u32, 2 v_mul_lo_u32,
 * 3 v_mad_u32_u24, 4 v_add_u32, 5 one Fp multiplication, 6 one Fp squaring, 7 v_fma_f64, 8 v_lshl_add_u64.
 * kind 9 is the calibration probe of the HBM counters: 2048 x CUs lanes each gather, `iters` times, the five 16-byte quads of a table addition from a
 * pseudo-random 128-byte row of the context's window-table buffer (needs a verify of >= 2^19 items on the context first); returns gathers per second.  Run under
 * `rocprofv3 --pmc FETCH_SIZE` it tells what the counter reports per gather of this access pattern (profiles/README.md). */
double plume_microbench(plume_ctx* ctx, int kind, int iters);
/* s_memtime ticks that workgroup 0 spent inside the last microbenchmark kernel (and its event duration in ms). */
double plume_microbench_last_ticks(float* ms);

#ifdef __cplusplus
}
#endif
#endif /* PLUME_HIP_H */
