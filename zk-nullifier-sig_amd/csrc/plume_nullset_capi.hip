// C ABI of the persistent nullifier set (include/plume_hip.h, plume_nullset_*; method in plume_nullset.h).  Host code only: every pass over the data is a
// gfx950 kernel of plume_nullset_kernels.hip.  A translation unit of its own, so that plume_capi.hip keeps exactly the launchers it had (the CPU harness of
// tests/hostsim compiles that file against its own host loops); it reaches the context only through plume_capi_internal.h.
//
// A set owns its device, stream, "last operation" event, table and scratch: it never touches a context's workspace and may outlive the context it was made
// from.  Every operation waits for the previous one (the event), so operations issued on different streams are serialised.  Nothing synchronises except
// the growth decision: the host keeps an upper bound on |S| (exact after any synchronising call) and reads the exact size only when bound + n would cross
// capacity / 2; a growth then rehashes on the operation's stream and synchronises once before the old table is freed.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <string>

#include "../../include/plume_hip.h"
#include "plume_capi_internal.h"
#include "plume_nullset_launch.h"

using namespace plume;

namespace {

int fail(int code, const std::string& msg) { return capi_fail(code, msg.c_str()); }
#define NSCHK(expr)                                                                                             \
    do {                                                                                                        \
        hipError_t e__ = (expr);                                                                                \
        if (e__ != hipSuccess) return fail(PLUME_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));  \
    } while (0)

struct Buf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {                  // (the old contents are not kept: scratch and staging only)
        if (bytes <= cap) return 0;
        release();
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) { p = nullptr; return fail(PLUME_ERR_HIP, std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e)); }
        cap = bytes;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as(size_t byte_off = 0) const { return (T*)((char*)p + byte_off); }
};

struct NullSet {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t last = nullptr;                  // recorded behind every operation
    hipStream_t last_stream = nullptr;          // ... on this stream
    uint64_t cap = 0;                           // slots
    uint64_t bound = 0;                         // upper bound on |S|
    NullsetTable t{};
    unsigned long long* dsize = nullptr;        // device word: |S|
    Buf scratch;                                // per insert: minid, owner, slot, blockcnt
    Buf in, out;                                // host-pointer forms: staged inputs / outputs
};

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// the operation's stream waits for the set's previous operation; a Hold leaves the event behind whatever the operation enqueued, on success or failure
struct Hold {
    NullSet* s;
    hipStream_t st;
    Hold(NullSet* set, hipStream_t stream) : s(set), st(stream) {}
    Hold(const Hold&) = delete;
    Hold& operator=(const Hold&) = delete;
    int acquire() {
        if (s->last_stream != st) NSCHK(hipStreamWaitEvent(st, s->last, 0));
        return 0;
    }
    ~Hold() {
        (void)hipEventRecord(s->last, st);
        s->last_stream = st;
    }
};

int bind(NullSet* s) {
    if (!s) return fail(PLUME_ERR_ARG, "null nullifier set");
    NSCHK(hipSetDevice(s->device));
    return 0;
}

// waits for everything issued on the set (through its own stream: the event's latest record is behind all the earlier ones); reads the exact size, which then is the bound
int exact_size(NullSet* s, uint64_t* size) {
    if (s->last_stream != s->stream) NSCHK(hipStreamWaitEvent(s->stream, s->last, 0));
    unsigned long long v = 0;
    NSCHK(hipMemcpyAsync(&v, s->dsize, 8, hipMemcpyDeviceToHost, s->stream));
    NSCHK(hipStreamSynchronize(s->stream));
    s->bound = v;
    *size = v;
    return 0;
}

// a table of new_cap slots holding every record; the set is unchanged if it fails.  Runs on st (which already waits for the set's last operation).
int grow(NullSet* s, uint64_t new_cap, hipStream_t st) {
    NullsetTable nt{};
    nt.mask = (uint32_t)(new_cap - 1);
    if (!capi_os_random(nt.key, sizeof nt.key)) return fail(PLUME_ERR_HIP, "getrandom failed: no hash key for the nullifier set");
    nt.key[1] |= 1u; nt.key[3] |= 1u;
    hipError_t e = hipMalloc((void**)&nt.tag, (size_t)new_cap * 4);
    if (e != hipSuccess) return fail(PLUME_ERR_HIP, std::string("hipMalloc(nullifier set tags, ") + std::to_string(new_cap * 4) + "): " + hipGetErrorString(e));
    e = hipMalloc((void**)&nt.rec, (size_t)new_cap * 64);
    if (e != hipSuccess) {
        (void)hipFree(nt.tag);
        return fail(PLUME_ERR_HIP, std::string("hipMalloc(nullifier set records, ") + std::to_string(new_cap * 64) + "): " + hipGetErrorString(e));
    }
    e = hipMemsetAsync(nt.tag, 0xFF, (size_t)new_cap * 4, st);
    if (e == hipSuccess && s->t.tag) { launch_nullset_rehash(s->t, s->cap, nt, st); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipStreamSynchronize(st);         // the one synchronisation of a growth: the old table is read until here
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        (void)hipFree(nt.rec); (void)hipFree(nt.tag);
        return fail(PLUME_ERR_HIP, std::string("nullifier set growth: ") + hipGetErrorString(e));
    }
    if (s->t.tag) { (void)hipFree(s->t.rec); (void)hipFree(s->t.tag); }
    s->t = nt;
    s->cap = new_cap;
    return 0;
}

// |S| + n <= 2^31, checked before anything is allocated (synchronises only when the bound says it might not hold)
int check_limit(NullSet* s, uint64_t n) {
    if (s->bound + n <= PLUME_NS_MAX_SIZE) return 0;
    uint64_t size = 0;
    if (int rc = exact_size(s, &size)) return rc;
    return size + n > PLUME_NS_MAX_SIZE ? fail(PLUME_ERR_ARG, "the nullifier set would exceed 2^31 records") : 0;
}
// before an insert of n items: the capacity that keeps the table at most half full (0: the current one does)
int plan_room(NullSet* s, uint64_t n, uint64_t* new_cap) {
    *new_cap = 0;
    if (s->bound + n <= s->cap / 2) return 0;
    uint64_t size = 0;
    if (int rc = exact_size(s, &size)) return rc;
    if (size + n > s->cap / 2) *new_cap = nullset_table_size(size + n);
    return 0;
}

int insert_device(NullSet* s, size_t n, const uint8_t* nul, const uint8_t* live, const uint64_t* ids, uint8_t* fresh, uint64_t* n_fresh, hipStream_t st) {
    Hold hold(s, st);
    if (int rc = hold.acquire()) return rc;
    if (n == 0) { if (n_fresh) NSCHK(hipMemsetAsync(n_fresh, 0, 8, st)); return 0; }
    if (int rc = check_limit(s, n)) return rc;
    uint64_t new_cap = 0;
    if (int rc = plan_room(s, n, &new_cap)) return rc;
    const size_t minid_b = align256(8 * n), owner_b = align256(4 * n), slot_b = align256(4 * n);
    if (s->scratch.ensure(minid_b + owner_b + slot_b + nullset_blockcnt_bytes(n))) return PLUME_ERR_HIP;   // scratch first: a failed growth then changes nothing
    if (new_cap) if (int rc = grow(s, new_cap, st)) return rc;
    NullsetInsertArgs a;
    a.t = s->t; a.n = (uint32_t)n; a.nul = nul; a.live = live; a.ids = ids; a.fresh = fresh;
    a.minid = s->scratch.as<unsigned long long>(); a.owner = s->scratch.as<uint32_t>(minid_b); a.slot = s->scratch.as<uint32_t>(minid_b + owner_b);
    a.blockcnt = s->scratch.as<uint32_t>(minid_b + owner_b + slot_b);
    a.size = s->dsize; a.n_fresh = (unsigned long long*)n_fresh;
    NSCHK(hipMemsetAsync(a.minid, 0xFF, 8 * n, st));
    launch_nullset_insert(a, st);
    NSCHK(hipGetLastError());
    s->bound += n;
    return 0;
}

int contains_device(NullSet* s, size_t n, const uint8_t* nul, uint8_t* found, hipStream_t st) {
    Hold hold(s, st);
    if (int rc = hold.acquire()) return rc;
    if (n == 0) return 0;
    NullsetQueryArgs a;
    a.t = s->t; a.n = (uint32_t)n; a.nul = nul; a.found = found;
    launch_nullset_contains(a, st);
    NSCHK(hipGetLastError());
    return 0;
}

int call_ok(NullSet* s, size_t n, const void* nul, const void* out) {
    if (int rc = bind(s)) return rc;
    if (n > PLUME_NS_MAX_CALL) return fail(PLUME_ERR_ARG, "n above 2^30");
    if (n && (!nul || !out)) return fail(PLUME_ERR_ARG, "null array");
    return 0;
}

}  // namespace

extern "C" int plume_nullset_create(plume_ctx* ctx, size_t reserve_items, void** set) {
    if (!set) return fail(PLUME_ERR_ARG, "null output pointer");
    *set = nullptr;
    int device = 0;
    if (int rc = capi_ctx_device(ctx, &device)) return rc;
    if (reserve_items > PLUME_NS_MAX_SIZE) return fail(PLUME_ERR_ARG, "reserve above 2^31 records");
    NSCHK(hipSetDevice(device));
    NullSet* s = new (std::nothrow) NullSet;
    if (!s) return fail(PLUME_ERR_HIP, "out of host memory");
    s->device = device;
    int rc = 0;
    hipError_t e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->last, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc((void**)&s->dsize, 8);
    if (e == hipSuccess) e = hipMemsetAsync(s->dsize, 0, 8, s->stream);
    if (e != hipSuccess) rc = fail(PLUME_ERR_HIP, std::string("nullifier set: ") + hipGetErrorString(e));
    if (!rc) rc = grow(s, nullset_table_size(reserve_items), s->stream);
    if (!rc) { e = hipEventRecord(s->last, s->stream); if (e != hipSuccess) rc = fail(PLUME_ERR_HIP, std::string("hipEventRecord: ") + hipGetErrorString(e)); }
    if (rc) { plume_nullset_destroy(s); return rc; }
    s->last_stream = s->stream;
    *set = s;
    return 0;
}

extern "C" void plume_nullset_destroy(void* set) {
    NullSet* s = (NullSet*)set;
    if (!s || hipSetDevice(s->device) != hipSuccess) return;
    if (s->last && s->stream && s->last_stream != s->stream) (void)hipStreamWaitEvent(s->stream, s->last, 0);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    if (s->t.tag) { (void)hipFree(s->t.rec); (void)hipFree(s->t.tag); }
    if (s->dsize) (void)hipFree(s->dsize);
    s->scratch.release(); s->in.release(); s->out.release();
    if (s->last) (void)hipEventDestroy(s->last);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

extern "C" int plume_nullset_reserve(void* set, size_t items) {
    NullSet* s = (NullSet*)set;
    if (int rc = bind(s)) return rc;
    if (items > PLUME_NS_MAX_SIZE) return fail(PLUME_ERR_ARG, "reserve above 2^31 records");
    const uint64_t want = nullset_table_size(items);
    if (want <= s->cap) return 0;
    Hold hold(s, s->stream);
    if (int rc = hold.acquire()) return rc;
    return grow(s, want, s->stream);
}

extern "C" int plume_nullset_clear(void* set) {
    NullSet* s = (NullSet*)set;
    if (int rc = bind(s)) return rc;
    Hold hold(s, s->stream);
    if (int rc = hold.acquire()) return rc;
    NSCHK(hipMemsetAsync(s->t.tag, 0xFF, (size_t)s->cap * 4, s->stream));
    NSCHK(hipMemsetAsync(s->dsize, 0, 8, s->stream));
    s->bound = 0;
    return 0;
}

extern "C" int plume_nullset_size(void* set, uint64_t* size, uint64_t* capacity) {
    NullSet* s = (NullSet*)set;
    if (int rc = bind(s)) return rc;
    uint64_t v = 0;
    if (int rc = exact_size(s, &v)) return rc;
    if (size) *size = v;
    if (capacity) *capacity = s->cap;
    return 0;
}

extern "C" int plume_nullset_insert_device(void* set, size_t n, const uint8_t* nullifier, const uint8_t* live, const uint64_t* ids, uint8_t* fresh, uint64_t* n_fresh,
                                           void* stream) {
    NullSet* s = (NullSet*)set;
    if (int rc = call_ok(s, n, nullifier, fresh)) return rc;
    return insert_device(s, n, nullifier, live, ids, fresh, n_fresh, stream ? (hipStream_t)stream : s->stream);
}

extern "C" int plume_nullset_contains_device(void* set, size_t n, const uint8_t* nullifier, uint8_t* found, void* stream) {
    NullSet* s = (NullSet*)set;
    if (int rc = call_ok(s, n, nullifier, found)) return rc;
    return contains_device(s, n, nullifier, found, stream ? (hipStream_t)stream : s->stream);
}

// host-pointer forms: staged through the set's own buffers on its own stream, synchronised at the end
extern "C" int plume_nullset_insert(void* set, size_t n, const uint8_t* nullifier, const uint8_t* live, const uint64_t* ids, uint8_t* fresh, uint64_t* n_fresh) {
    NullSet* s = (NullSet*)set;
    if (int rc = call_ok(s, n, nullifier, fresh)) return rc;
    if (n == 0) { if (n_fresh) *n_fresh = 0; return 0; }
    if (int rc = check_limit(s, n)) return rc;
    const size_t nul_b = align256(64 * n), live_b = align256(n);
    if (s->in.ensure(nul_b + live_b + 8 * n) || s->out.ensure(align256(n) + 8)) return PLUME_ERR_HIP;
    hipStream_t st = s->stream;
    uint8_t* dnul = s->in.as<uint8_t>();
    uint8_t* dlive = live ? s->in.as<uint8_t>(nul_b) : nullptr;
    uint64_t* dids = ids ? s->in.as<uint64_t>(nul_b + live_b) : nullptr;
    uint8_t* dfresh = s->out.as<uint8_t>();
    uint64_t* dcnt = s->out.as<uint64_t>(align256(n));
    {
        Hold hold(s, st);                           // (the staging buffers of the previous host-form call are free: it synchronised)
        if (int rc = hold.acquire()) return rc;
        NSCHK(hipMemcpyAsync(dnul, nullifier, 64 * n, hipMemcpyHostToDevice, st));
        if (live) NSCHK(hipMemcpyAsync(dlive, live, n, hipMemcpyHostToDevice, st));
        if (ids) NSCHK(hipMemcpyAsync(dids, ids, 8 * n, hipMemcpyHostToDevice, st));
    }
    int rc = insert_device(s, n, dnul, dlive, dids, dfresh, dcnt, st);
    uint64_t cnt = 0;
    if (!rc) {
        hipError_t e = hipMemcpyAsync(fresh, dfresh, n, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(&cnt, dcnt, 8, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) rc = fail(PLUME_ERR_HIP, std::string("nullifier set download: ") + hipGetErrorString(e));
    }
    const hipError_t e = hipStreamSynchronize(st);
    if (rc) return rc;
    if (e != hipSuccess) return fail(PLUME_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    if (n_fresh) *n_fresh = cnt;
    s->bound -= n - cnt;                           // synchronised: the bound is exact again
    return 0;
}

extern "C" int plume_nullset_contains(void* set, size_t n, const uint8_t* nullifier, uint8_t* found) {
    NullSet* s = (NullSet*)set;
    if (int rc = call_ok(s, n, nullifier, found)) return rc;
    if (n == 0) return 0;
    if (s->in.ensure(64 * n) || s->out.ensure(n)) return PLUME_ERR_HIP;
    hipStream_t st = s->stream;
    int rc = 0;
    {
        Hold hold(s, st);
        if ((rc = hold.acquire())) return rc;
        NSCHK(hipMemcpyAsync(s->in.p, nullifier, 64 * n, hipMemcpyHostToDevice, st));
    }
    rc = contains_device(s, n, s->in.as<uint8_t>(), s->out.as<uint8_t>(), st);
    if (!rc) {
        const hipError_t e = hipMemcpyAsync(found, s->out.p, n, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) rc = fail(PLUME_ERR_HIP, std::string("nullifier set download: ") + hipGetErrorString(e));
    }
    const hipError_t e = hipStreamSynchronize(st);
    if (rc) return rc;
    if (e != hipSuccess) return fail(PLUME_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    return 0;
}

extern "C" int plume_nullset_export(void* set, size_t cap, uint8_t* records, uint64_t* count) {
    NullSet* s = (NullSet*)set;
    if (int rc = bind(s)) return rc;
    if (!count) return fail(PLUME_ERR_ARG, "null count");
    uint64_t size = 0;
    if (int rc = exact_size(s, &size)) return rc;
    *count = size;
    if (!records) return 0;
    if (cap < size) return fail(PLUME_ERR_ARG, "records holds fewer than size() records");
    if (size == 0) return 0;
    const size_t nb = nullset_export_blocks(s->cap), cnt_b = align256(4 * nb);
    if (s->in.ensure(cnt_b + 8) || s->out.ensure((size_t)size * 64)) return PLUME_ERR_HIP;
    hipStream_t st = s->stream;
    NullsetExportArgs a;
    a.t = s->t; a.cap = s->cap; a.blockcnt = s->in.as<uint32_t>(); a.count = s->in.as<unsigned long long>(cnt_b); a.out = s->out.as<uint8_t>(); a.rows = size;
    unsigned long long written = 0;
    int rc = 0;
    {
        Hold hold(s, st);
        if ((rc = hold.acquire())) return rc;
        launch_nullset_export(a, st);
        NSCHK(hipGetLastError());
        NSCHK(hipMemcpyAsync(&written, a.count, 8, hipMemcpyDeviceToHost, st));
        NSCHK(hipMemcpyAsync(records, a.out, (size_t)size * 64, hipMemcpyDeviceToHost, st));
    }
    NSCHK(hipStreamSynchronize(st));
    if (written != size) return fail(PLUME_ERR_HIP, "nullifier set export: the table holds " + std::to_string(written) + " records, the size word says " + std::to_string(size));
    return rc;
}
