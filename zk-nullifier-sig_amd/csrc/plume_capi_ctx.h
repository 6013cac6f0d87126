// What the call families' translation units (plume_eth_capi.hip, plume_eth_hash_capi.hip, plume_ecdsa_capi.hip, plume_eth_tx_capi.hip, plume_merkle_capi.hip,
// plume_ecdsa_sign_capi.hip, plume_eth_tx_sign_capi.hip, plume_hd_capi.hip, plume_kdf_capi.hip) share with plume_capi.hip: the context and its buffers, routing, the workspace chain, the tables
// and the host-call machinery -- all defined once, in plume_capi.hip -- and the stages one family lends another.  Internal: not part of the ABI, every function hidden in
// the shared object.  The three launcher hooks that remain (nonce, release, recover) are plume_capi_internal.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/plume_hip.h"
#include "plume_launch.h"

namespace plume {
// sets this thread's plume_last_error() text; returns code
__attribute__((visibility("hidden"))) int fail(int code, const std::string& msg);
}  // namespace plume
#define HIPCHK(expr)                                                                                                     \
    do {                                                                                                                 \
        hipError_t e__ = (expr);                                                                                         \
        if (e__ != hipSuccess) return plume::fail(PLUME_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));    \
    } while (0)

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { p = nullptr; return plume::fail(PLUME_ERR_HIP, std::string("hipMalloc(") + std::to_string(want) + "): " + hipGetErrorString(e)); }
        cap = want;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return (T*)p; }
};

// page-locked host scratch (hipHostMalloc): the source of uploads the library itself prepares.  A pageable source would make the runtime stage the copy and move it with a
// blit KERNEL, which then queues behind the saturating multi-scalar kernel and stalls the upload stream (seen in the round-4 pipeline trace: tests/gpu_debug/e2e_trace.py)
struct PinnedBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e != hipSuccess) { p = nullptr; return plume::fail(PLUME_ERR_HIP, std::string("hipHostMalloc(") + std::to_string(want) + "): " + hipGetErrorString(e)); }
        cap = want;
        return 0;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};

struct StageTimer {
    std::vector<const char*> names;
    std::vector<hipEvent_t> ev;   // ev[0] start, ev[i+1] after stage i
    size_t used = 0;
    uint64_t runs = 0;            // calls that started a timeline here, i.e. put work on this context (Route)
    bool on = false;              // plume_set_stage_timing: a timing event between two kernels of a stream costs ~6 us of idle GPU (rocprofv3 trace of 2^16-item calls, round 5:
                                  // kernels without an event between them follow each other within 0.2 us), five or six per call -- 2 % of a 2^16-item verify, so only on request
    void begin(hipStream_t st) { runs++; names.clear(); used = 0; if (on) mark(st); }
    void mark(hipStream_t st) {
        if (used == ev.size()) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return; ev.push_back(e); }
        (void)hipEventRecord(ev[used++], st);
    }
    void stage(const char* name, hipStream_t st) { if (!on) return; names.push_back(name); mark(st); }
    void destroy() { for (auto e : ev) (void)hipEventDestroy(e); ev.clear(); }
};

// staging for one piece of a host-pointer call
struct HostSlot {
    DevBuf msgs, off, in[6], out[8];
    DevBuf ragged;                                                    // the ragged output of a serial call that has one (HostCall::ragged)
    PinnedBuf relbuf;                                                 // piece-relative message offsets (source of an upload: lives until the slot is reused), page-locked
    uint64_t* rel = nullptr;
    hipEvent_t ready = nullptr, computed = nullptr, drained = nullptr;   // uploads landed / kernels finished / downloads landed
    bool in_flight = false;
};

struct Worker;   // one worker thread per shard of a multi-device context (plume_capi.hip)

// The generator's fixed tables (the verifier's 2^23-row window table, 1 GiB; the signer's comb, 252 MiB; 18 ms to build both) depend on nothing but G: every context of a
// process on the same device shares ONE read-only copy, freed with the last context (a second batch in flight -- a second context -- then costs its workspace only).
// Round 4: each table is built by the first call that needs it (need_gtab: verify, verify_non_zk; need_gcomb: sign, SEC1-DER export, the aggregate check), so a
// verify-only process never holds the comb, a sign-only one never the 1 GiB window table, and plume_init itself allocates neither.
struct FixedTables {
    std::mutex m;                 // the tables of ONE device: their build (18 ms, synchronous) holds this lock, not the process-wide one -- the shards of a multi-device context
                                  // build theirs side by side (the CPU pipeline harness showed eight shards' first call queueing behind one lock: tests/hostsim)
    DevBuf gtab, gcomb, gscan;
    int refs = 0;                 // under g_fixed_mutex
    bool gtab_built = false, gcomb_built = false, gscan_built = false;
};

struct plume_ctx {
    int device = 0;
    hipStream_t stream = nullptr, up = nullptr, down = nullptr;   // kernels / host->HBM / HBM->host
    hipStream_t side = nullptr;                                   // aggregate check: the generator term and the upper windows' reduction run beside the main stream
    hipStream_t pre = nullptr;                                    // overlapped verify / sign: the stages BEFORE the multi-scalar kernel of sub-batch k+1 run here, beside that kernel of sub-batch k
    hipEvent_t pre_begin = nullptr;                               // ... the caller's stream has reached the call (inputs are there, the workspace is free)
    std::vector<hipEvent_t> pre_ready;                            // ... sub-batch k's window tables are built
    const char* last_msm_kernel = nullptr;                         // the multi-scalar kernel the last verify call on this context launched (plume_last_msm_kernel)
    bool last_msm_sampled = false;                                 // ... and whether that launch sampled its clocks (plume_last_msm_clock: stage timing was on for the call)
    std::vector<size_t> redo_counters;                            // word offsets (in `redo`) of the last verify call's redo counters, one per sub-batch (plume_last_redo_tasks)
    bool redo_foreign = false;                                    // ... the last call that laid out `redo` on this context was not a verify call (ecdsa_device: one counter per slice at lo + k),
                                                                  // so those offsets hold another family's list: plume_last_redo_tasks refuses until a verify call has run here
    int sub_batches = 1;                                          // device-resident verify / sign: number of sub-batches; 1 = strictly serial launch order (the default: measured on the MI355X, r03, kernels of two
                                                                  // streams sharing the CUs cost MORE than the table kernel's idle issue slots give back -- 21.85 ms serial vs 22.1-22.4 ms for 2..16 sub-batches, LABNOTES.md §6)
    size_t overlap_min = (size_t)1 << 17;                         // ... batches below this many items always run serial (a sub-batch must still fill the chip)
    hipEvent_t agg_ev[4] = {nullptr, nullptr, nullptr, nullptr};  // terms ready / upper bucket sums ready / generator term ready / upper windows reduced
    hipEvent_t ws_free = nullptr;     // recorded behind the last kernel of every device-resident call: the next call's stream waits on it before it
    bool ws_used = false;             // touches the per-context workspace, so calls on DIFFERENT streams of one context cannot race on that scratch
    hipStream_t ws_stream = nullptr;  // the stream ws_free was last recorded on
    size_t chunk = (size_t)1 << 20;
    size_t host_piece = (size_t)1 << 19;                            // host-pointer calls: largest pipelined piece
    size_t host_first_piece = (size_t)1 << 16;                      // ... the first piece (its upload is the only one no kernel hides); pieces then grow 3x per step
    size_t host_tail_piece = (size_t)1 << 16;                       // ... the last piece of calls with large outputs (its download is the only one no kernel hides)
    size_t host_register_min = 0;                                   // host-pointer calls: page-lock caller arrays of at least this many bytes for the call (0 = never)
    // multi-device parent (plume_init_multi): the shards are complete single-device contexts, one worker thread each; a parent owns no GPU state
    std::vector<plume_ctx*> shards;
    std::vector<Worker*> workers;
    HostSlot slot[4];                                              // host-pointer calls: staging slots (two for the one-lane pipeline, four when two lanes take the pieces in turn)
    plume_ctx* host_lane = nullptr;                                // ... the second lane of the host-pointer pipeline: a complete single-device context (workspace, streams), created on first use
    size_t msm_pair_max = (size_t)1 << 14;                          // verify calls (slices) of at most this many items run k_verify_msm_pair (env PLUME_MSM_PAIR_MAX; 0: never)
    bool split_scalars = true;                                      // ... and the scalar stage in that kernel's idle role (env PLUME_SPLIT_SCALARS=0: a launch of its own, A/B)
    size_t ingest_split_max = (size_t)1 << 16;                     // verify calls (slices) of at most this many items run the ingest stage with two lanes per item (latency-bound there)
    int sign_uniform = 1;                                          // plume_set_sign_uniform: the signer's schedule (level 0, 1, 2).  Default 1 since round 5: no branch on a digit of sk or r
                                                                   // (k256's multiplication is constant-time, rust-k256/src/randomizedsigner.rs:51-70; measured price +2.5 % per signature)
    int host_lanes = 2;                                            // ... 1 = every piece on the context itself (rounds 1-3), 2 = pieces alternate between the context and host_lane
    int host_sign_lanes = 2;                                       // ... the signer's host-pointer call: lanes it may use (env PLUME_HOST_SIGN_LANES).  2 since round 6, with uniform 2^16-item pieces (plume_host_logic.h)
    bool host_lane_failed = false;                                 // ... the second lane could not be created once (out of memory): do not retry on every call
    int jobs_per_lane = plume::kTableJobsPerLane;
    bool jobs_per_lane_forced = false;
    FixedTables* fixed = nullptr;                                 // this device's shared generator tables (g_fixed)
    // batches in flight (plume_set_in_flight): device-resident calls are dealt out in turn to this context and to `lanes`, complete single-device contexts of their own
    // (workspace, streams, events; the fixed tables are shared), so that calls the caller issues on DIFFERENT streams run side by side instead of queueing for one workspace
    std::vector<plume_ctx*> lanes;
    size_t lane_next = 0;
    size_t in_flight_min = 0;                                      // verify / sign calls of fewer items are not dealt out to the lanes (env PLUME_IN_FLIGHT_MIN; 0, the default: every call is)
    plume_ctx* lane_last = nullptr;                               // the lane the last device-resident call went to (plume_last_stage_times, plume_last_redo_tasks)
    DevBuf bases, jobflags, itemflags, tab, tabscr, res, resinf, res2, res2inf, pkaff, sink, redo, digs, eq1fall, eq1k, clk;
    int sign_selfcheck = 0;                                        // plume_set_sign_selfcheck: 1 = every sign call stages its outputs here, verifies them and releases what verifies (sign_device)
    DevBuf scstage;                                                // ... the staging: six records in the 64-byte form, the signer's status and the check's verdict, 322 B / item; wiped after the release
    DevBuf txstage;                                                // plume_eth_tx_sender_batch: what k_eth_tx_parse hands the recover stages -- hash, r, s, v, 97 B / item (public data: not wiped)
    DevBuf txsign;                                                 // plume_eth_tx_sign_batch: the framing (chain id, packed frame word), the signing hash and what the sign stages make of it -- 114 B / item; r, s, v and status wiped behind the assemble
    DevBuf hdws;                                                   // plume_hd_derive_*_batch: k, the chain code and the status of every item between the levels, 65 B / item; wiped behind finish
    DevBuf kdfws;                                                  // plume_pbkdf2_sha512_batch: the midstates, U and T of every item between the kernels, 256 B / item; wiped behind finish
    DevBuf mrksort;                                                // plume_merkle_tree_build: the sort's records, nine word arrays of npad words, 36 B / padded leaf (public data: not wiped)
    DevBuf nonce;                                                  // the derived-nonce signer: r of the call in flight, 32 B / item, wiped on the call's stream after sign_final
    int eq1_short = 1;                                             // verify calls that give R: equation 1 in its short form (plume_eis.h).  0 = long form always (A/B), 2 = test: every item takes the fallback
    size_t eq1_short_min = (size_t)1 << 16;                        // ... for calls of at least this many items.  Round 6 sweep on one box, interleaved (profiles/r06_eq1_threshold.txt), now that the
                                                                   // scalar stage -- half-GCD included -- of calls up to 2^16 runs in role B of the two-role ingest kernel: 2^16 items 1.385 -> 1.343 ms
                                                                   // (-3.0 %), 2^17 -4.4 %, 2^18 -4.1 %; 2^15 +6.3 % (0.928 -> 0.987: one wavefront per SIMD, the chain's latency is the
                                                                   // kernel's time and equation 2's chain is the long one either way), <= 2^14 +35 % (the half chains of k_verify_msm_pair
                                                                   // need the long form).  Round 5's threshold, before the scalar stage moved: 2^17
    DevBuf dec[4], preflags;
    DevBuf agg[15];      // aggregate check (plume_aggregate.h): haff, scal, flags, gs, hash_ok, counters, count, sort tiles, sorted, bsum, bsuminf, red, redinf, ssum, perm + its histogram
    DevBuf agg_record;   // the running record of a host-pointer aggregate call (pieces of one batch)
    DevBuf dslots, dminid, dmyslot, dcount, dblockcnt;   // nullifier-set post-processing (plume_dedup.h)   // SEC1 ingest: decompressed 64-byte records + per-item reject flags
    StageTimer timer;
};

// One host-pointer call, stated once: the caller's arrays in the order of HostSlot::in[k] / out[k].  Registration, the page-lock check for two lanes, the copies and
// the shard offsets are all read off this table, so they cannot disagree (round 4's page-lock check listed its arrays by hand and missed some: ADVICE r4).
struct HostArray {
    const void* p = nullptr;   // the caller's array; null: not given
    size_t stride = 0;         // bytes per item; 0 = unused entry
    bool secret = false;       // the staged copy is wiped once it has served: an input behind the kernels that read it, an output (serial calls only) behind its download
    bool whole = false;        // serial calls only: `stride` bytes in all, not per item.  An input is given once for the call: uploaded in front of the first piece, not advanced by shard()
};
struct HostCall {
    const uint8_t* msgs;       // may be null when the offsets give it no bytes
    const uint64_t* msg_off;   // null (serial calls only): the call has no messages and stages none
    HostArray in[6], out[8];
    bool out_heavy = false, may_use_two_lanes = false;
    bool msgs_secret = false;                                         // serial calls only: the staged message bytes are wiped behind the kernels, as an input marked secret is
    const char *off_name = "msg_off", *msgs_name = "message";         // what the argument errors of the message staging call the two
    // serial calls only: a ragged output tied to the messages.  Item i owns the ragged_growth i + (msg_off[i] - msg_off[0]) .. bytes of it, its message's length plus
    // ragged_growth of them; a piece's share is contiguous, staged in HostSlot::ragged and downloaded in one copy behind the fixed-stride outputs
    void* ragged = nullptr;
    size_t ragged_growth = 0;
    size_t ragged_at(size_t i) const { return (size_t)(msg_off[i] - msg_off[0]) + ragged_growth * i; }
    // items [lo, ...) of the same call: msg_off keeps the caller's absolute offsets into the same msgs buffer
    HostCall shard(size_t lo) const {
        HostCall c = *this;
        if (c.ragged) c.ragged = (uint8_t*)c.ragged + ragged_at(lo);
        if (c.msg_off) c.msg_off += lo;
        for (HostArray& a : c.in) if (a.p && !a.whole) a.p = (const uint8_t*)a.p + a.stride * lo;
        for (HostArray& a : c.out) if (a.p && !a.whole) a.p = (const uint8_t*)a.p + a.stride * lo;
        return c;
    }
};
// what a host-pointer call runs per piece: run(slot, cnt, lane) enqueues the kernels of one piece and picks which of the slot's buffers they get
using HostRun = std::function<int(HostSlot&, size_t, plume_ctx*)>;

namespace plume {

// a single-device context's device made current; PLUME_ERR_ARG for a null or a multi-device context (the device-resident entry points)
__attribute__((visibility("hidden"))) int bind(plume_ctx* ctx);
// the workspace chain: the wait in front of a device-resident call's first touch of the context's scratch (WsHold then leaves the event behind its last kernel)
__attribute__((visibility("hidden"))) int ws_acquire(plume_ctx* ctx, hipStream_t st);
// the generator's tables, built by the first call that needs them: the comb; the signer's table (the comb, or at level 2 of the uniform schedule the scanned table)
__attribute__((visibility("hidden"))) int need_gcomb(plume_ctx* ctx);
__attribute__((visibility("hidden"))) int need_sign_tables(plume_ctx* ctx);
// the slices plume_set_sub_batches cuts a call of n items into: cut[k] .. cut[k + 1]
__attribute__((visibility("hidden"))) std::vector<size_t> sub_batch_bounds(const plume_ctx* ctx, size_t n);
// the window tables of njobs bases (into ctx->tabscr, of at least table_stage_scratch bytes)
__attribute__((visibility("hidden"))) size_t table_stage_scratch(const plume_ctx* ctx, size_t njobs, size_t nthrees);
__attribute__((visibility("hidden"))) void table_stage(plume_ctx* ctx, uint32_t* tab, const uint32_t* bases, const uint8_t* jobflags, size_t njobs, size_t nthrees, hipStream_t st);
// The host-pointer forms, arguments already checked (plume_capi.hip, "host-pointer pipelines" and "serial host-pointer calls"; its own calls instantiate the templates these
// forward to).  `run` is called once per piece, in front of a stream synchronise or of thousands of items of kernel work.
__attribute__((visibility("hidden"))) int host_call_any(plume_ctx* ctx, size_t n, const HostCall& call, HostRun run);
__attribute__((visibility("hidden"))) int serial_host_piece(plume_ctx* ctx, const HostCall& call, size_t i0, size_t cnt, HostRun run);
__attribute__((visibility("hidden"))) int serial_host_call(plume_ctx* ctx, size_t n, const HostCall& call, HostRun run);
__attribute__((visibility("hidden"))) int serial_host_call_any(plume_ctx* ctx, size_t n, const HostCall& call, HostRun run);

// ---- stages one family lends another: defined in the lender's file
// plume_ecdsa_capi.hip, for the transaction sender and the ECDSA signer's self-check.  continue_timer: the caller holds the workspace already and has begun the timeline
__attribute__((visibility("hidden"))) int ecdsa_args_ok(int flags, int pk_format, int addr_format, size_t n, const void* hash, const void* r, const void* s, const void* v,
                                                        const void* pk, const void* address, const void* status);
__attribute__((visibility("hidden"))) int ecdsa_device(plume_ctx* ctx, int flags, int pk_format, int addr_format, size_t n, const uint8_t* hash, const uint8_t* r,
                                                       const uint8_t* s, const uint8_t* v, const uint8_t* expect, uint8_t* pk, uint8_t* address, uint8_t* status, hipStream_t st,
                                                       bool continue_timer = false);
// plume_ecdsa_sign_capi.hip, for the transaction signer
__attribute__((visibility("hidden"))) int ecdsa_sign_args_ok(int flags, size_t n, const void* hash, const void* sk, const void* r, const void* s, const void* v,
                                                             const void* status);
__attribute__((visibility("hidden"))) int ecdsa_sign_device(plume_ctx* ctx, int flags, size_t n, const uint8_t* hash, const uint8_t* sk, const uint8_t* aux, uint8_t* r,
                                                            uint8_t* s, uint8_t* v, uint8_t* status, hipStream_t st, bool continue_timer = false);
// the transaction calls and the transaction signer (defined here: neither file links the other): their host-pointer forms stage their bytes as a message-hash call does; the
// argument errors speak of transactions
inline HostCall eth_tx_call(const HostCall& call) { HostCall c = call; c.off_name = "tx_off"; c.msgs_name = "transaction"; return c; }

}  // namespace plume

// The lane a device-resident call runs on -- the context itself, or one of its in-flight lanes in turn -- and the stream it runs on.  The stream is resolved against the
// context the CALLER holds before the call is dealt out: NULL means "that context's own stream" whichever lane serves the call, so successive NULL-stream calls stay
// ordered against each other (a sign followed by a verify of its outputs) exactly as they are without lanes.  (Round 3 resolved NULL after routing, i.e. to the lane's
// private stream, which changes from call to call: ADVICE r3.)  A lane's workspace is guarded by its ws_free event, so running it on a stream it does not own is safe.
struct Route {
    plume_ctx* held;           // the context the caller holds
    plume_ctx* lane;           // the lane that serves this call
    hipStream_t st;
    size_t next0 = 0;
    plume_ctx* last0 = nullptr;
    uint64_t epoch0 = 0;
    Route(plume_ctx* ctx, void* stream, size_t n = (size_t)-1) : held(ctx), lane(ctx) {
        st = stream ? (hipStream_t)stream : (ctx ? ctx->stream : nullptr);
        if (!ctx) return;
        next0 = ctx->lane_next; last0 = ctx->lane_last;
        if (!ctx->lanes.empty() && n >= ctx->in_flight_min) {                 // (a small call stays on the first lane: plume_set_in_flight)
            const size_t k = ctx->lanes.size() + 1, i = ctx->lane_next++ % k;
            lane = i == 0 ? ctx : ctx->lanes[i - 1];
        }
        ctx->lane_last = lane;
        epoch0 = lane->timer.runs;
    }
    Route(const Route&) = delete;
    Route& operator=(const Route&) = delete;
    // A call that is refused before it starts its lane's stage timeline (an argument check, n above the chunk size, an empty batch) never happened as far as the lanes are concerned:
    // it neither takes a turn nor becomes "the last device-resident call" that plume_last_stage_times / plume_last_redo_tasks report.  (Found by the CPU pipeline harness,
    // tests/hostsim: a refused call moved lane_last to a lane that had run nothing, and the stage times read afterwards -- and the wait they imply -- were another call's.)
    ~Route() { if (held && lane->timer.runs == epoch0) { held->lane_next = next0; held->lane_last = last0; } }
};
// Holds the workspace from a successful ws_acquire to the end of the call.  A call that fails half way (an allocation, a launch) must still leave ws_free behind
// whatever it has already enqueued -- on the caller's stream and on the context's side stream -- or the next call, on another stream, would run into it.
struct WsHold {
    plume_ctx* ctx;
    hipStream_t st;
    bool released = false;
    WsHold(plume_ctx* c, hipStream_t s) : ctx(c), st(s) {}
    WsHold(const WsHold&) = delete;
    WsHold& operator=(const WsHold&) = delete;
    int release();             // records ws_free behind the call's last kernel (plume_capi.hip)
    ~WsHold() {
        if (released) return;
        if (ctx->side) (void)hipStreamSynchronize(ctx->side);      // failure path only: side-stream work the caller's stream never joined
        if (ctx->pre) (void)hipStreamSynchronize(ctx->pre);
        (void)hipEventRecord(ctx->ws_free, st);
        ctx->ws_used = true;
        ctx->ws_stream = st;
    }
};
