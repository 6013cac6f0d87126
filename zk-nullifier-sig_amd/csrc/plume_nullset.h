// Persistent nullifier set (include/plume_hip.h, plume_nullset_*): the step after plume_dedup.h for a consumer that verifies a STREAM of batches and must
// reject a nullifier accepted any number of batches ago.  A set is an open-addressing table in HBM that lives across calls:
//
//   rec[cap]   64-byte records (64-byte aligned), opaque, compared byte for byte; the all-zero identity is an ordinary record
//   tag[cap]   one uint32 per slot: PLUME_NS_EMPTY (all ones), PLUME_NS_FULL | 30-bit fingerprint, or -- only while an insert runs -- the index i < 2^30
//              of the item of that call that claimed the slot ("pending")
//
// cap is a power of two and the table is at most half full (plume_nullset_capi.hip grows it before a call could cross that), so every probe ends.  Two keyed
// hashes of the record (dedup_hash under key[0..1] and key[2..3]; the key is drawn from the OS generator when the set is made and again at every growth):
// the first picks the home slot, the second gives the fingerprint, so most probes that meet another record skip its 64-byte gather.  Results do not depend on
// the key, the table size or the order the lanes run in.
//
// insert = launches with no spin anywhere (scratch per call, sized by n: owner, slot, minid per item):
//   probe   per live item, from the home slot: FULL with its fingerprint -> compare with rec[h]: equal = the record was in the set before (not fresh, done);
//           EMPTY -> atomicCAS(EMPTY -> i): won = claimant, lost = the returned tag is read as below; pending j -> compare with the INPUT record j: equal =
//           share j's slot (atomicMin of the item's id into minid[j]); anything else -> h + 1.  Tags only go EMPTY -> pending during the launch and FULL
//           entries were written by an earlier launch, so a stale plain read can only show EMPTY where a tag is pending, and the CAS corrects that (the
//           argument plume_dedup.h relies on across XCDs).  No record of the set can be missed: linear probing without deletion keeps every slot between a
//           record's home and its slot non-empty.
//   commit  fresh[i] = the item's slot was claimed in this call and minid[claimant] is its id; each claimant writes its record and FULL | fingerprint;
//           per-workgroup counts of fresh items, then one small kernel adds their sum to the device-side size (as k_dedup_sum does).
// contains = a read-only probe over FULL slots that stops at EMPTY.  rehash (growth) = per FULL slot of the old table, atomicCAS(EMPTY -> FULL | fp) in the
// new one and the record written behind it: the records are distinct, so no compare.  export = count per block of slots, one-block scan, scatter.
#pragma once
#include <stdint.h>

#include "plume_dedup.h"

namespace plume {

#define PLUME_NS_EMPTY 0xFFFFFFFFu
#define PLUME_NS_FULL 0x80000000u               // FULL | fingerprint: 0x80000000 .. 0xBFFFFFFF
#define PLUME_NS_FP_MASK 0x3FFFFFFFu
#define PLUME_NS_MAX_CALL (1u << 30)            // items per call (pending tags are item indices below this)
#define PLUME_NS_MAX_SIZE (1ull << 31)          // records per set
#define PLUME_NS_NOT_LIVE 0xFFFFFFFFu           // owner[i] of an item that takes no part
#define PLUME_NS_PRESENT 0xFFFFFFFEu            // owner[i] of an item whose record was in the set before the call
#define PLUME_NS_EXPORT_PER_LANE 16u            // export: slots per lane of a 256-lane block (4096 slots per block)

struct NullsetTable {
    uint8_t* rec;                    // cap x 64 bytes
    uint32_t* tag;                   // cap words
    uint32_t mask;                   // cap - 1 (cap <= 2^32)
    uint32_t key[4];                 // home slot: dedup_hash under key[0..1]; fingerprint: under key[2..3]
};

struct NullsetInsertArgs {
    NullsetTable t;
    uint32_t n;
    const uint8_t* nul;              // 64 B / item, 16-byte aligned
    const uint8_t* live;             // optional, n bytes
    const uint64_t* ids;             // optional, n distinct ids; NULL: id = position
    uint8_t* fresh;                  // out, n bytes
    uint32_t* owner;                 // scratch, n: claimant index, PLUME_NS_PRESENT or PLUME_NS_NOT_LIVE
    uint32_t* slot;                  // scratch, n: the slot a claimant took
    unsigned long long* minid;       // scratch, n: smallest id among the items sharing claimant i's slot (all ones before the probe launch)
    uint32_t* blockcnt;              // scratch: fresh items per workgroup of the commit launch
    unsigned long long* size;        // device word: |S|, grows by the number of fresh items
    unsigned long long* n_fresh;     // optional device word: number of fresh items of this call
};

struct NullsetQueryArgs {
    NullsetTable t;
    uint32_t n;
    const uint8_t* nul;
    uint8_t* found;                  // out, n bytes
};

struct NullsetExportArgs {
    NullsetTable t;
    uint64_t cap;
    uint32_t* blockcnt;              // per block of 256 x PLUME_NS_EXPORT_PER_LANE slots: FULL slots, then (after the scan) the block's first output row
    unsigned long long* count;       // device word: number of records written
    uint8_t* out;                    // rows x 64 bytes
    uint64_t rows;                   // rows of out (|S|): a slot beyond them is counted, not written
};

// the table that holds `items` records at load <= 1/2: the next power of two >= 2 * items, at least 64
PLUME_HD uint64_t nullset_table_size(uint64_t items) {
    uint64_t m = 64;
    while (m < 2 * items) m <<= 1;
    return m;
}

PLUME_HD void nullset_load(const uint8_t* p, uint32_t r[16]) {
    const uint32_t* w = (const uint32_t*)__builtin_assume_aligned(p, 16);
    PLUME_UNROLL for (int k = 0; k < 16; k++) r[k] = w[k];
}
PLUME_HD bool nullset_equal(const uint8_t* p, const uint32_t r[16]) {
    const uint32_t* w = (const uint32_t*)__builtin_assume_aligned(p, 16);
    uint32_t diff = 0;
    PLUME_UNROLL for (int k = 0; k < 16; k++) diff |= w[k] ^ r[k];
    return diff == 0;
}
PLUME_HD void nullset_store(uint8_t* p, const uint32_t r[16]) {
    uint32_t* w = (uint32_t*)__builtin_assume_aligned(p, 16);
    PLUME_UNROLL for (int k = 0; k < 16; k++) w[k] = r[k];
}
PLUME_HD uint32_t nullset_home(const NullsetTable& t, const uint32_t r[16]) { return dedup_hash(r, t.key) & t.mask; }
PLUME_HD uint32_t nullset_full_tag(const NullsetTable& t, const uint32_t r[16]) { return PLUME_NS_FULL | (dedup_hash(r, t.key + 2) & PLUME_NS_FP_MASK); }
PLUME_HD bool nullset_is_full(uint32_t tag) { return (tag & 0xC0000000u) == PLUME_NS_FULL; }
PLUME_HD unsigned long long nullset_id(const NullsetInsertArgs& a, uint32_t i) { return a.ids ? (unsigned long long)a.ids[i] : (unsigned long long)i; }

PLUME_HD void nullset_probe(const NullsetInsertArgs& a, uint32_t i) {
    if (a.live && !a.live[i]) { a.owner[i] = PLUME_NS_NOT_LIVE; return; }
    uint32_t r[16];
    nullset_load(a.nul + 64 * (size_t)i, r);
    const uint32_t full = nullset_full_tag(a.t, r);
    uint32_t h = nullset_home(a.t, r);
    for (;;) {
        uint32_t tag = a.t.tag[h];
        if (tag == PLUME_NS_EMPTY) {
            tag = PLUME_ATOMIC_CAS_U32(&a.t.tag[h], PLUME_NS_EMPTY, i);
            if (tag == PLUME_NS_EMPTY) {                                               // claimed
                a.owner[i] = i;
                a.slot[i] = h;
                PLUME_ATOMIC_MIN_U64(&a.minid[i], nullset_id(a, i));
                return;
            }
        }
        if (nullset_is_full(tag)) {
            if (tag == full && nullset_equal(a.t.rec + 64 * (size_t)h, r)) { a.owner[i] = PLUME_NS_PRESENT; return; }   // in the set before this call
        } else if (nullset_equal(a.nul + 64 * (size_t)tag, r)) {                       // pending item `tag` of this call holds the same record: share its slot
            PLUME_ATOMIC_MIN_U64(&a.minid[tag], nullset_id(a, i));
            a.owner[i] = tag;
            return;
        }
        h = (h + 1) & a.t.mask;
    }
}
// returns the flag; the caller (kernel: workgroup reduction into blockcnt, host: plain sum) accumulates the count
PLUME_HD bool nullset_commit(const NullsetInsertArgs& a, uint32_t i) {
    const uint32_t o = a.owner[i];
    const bool f = o < PLUME_NS_MAX_CALL && a.minid[o] == nullset_id(a, i);
    a.fresh[i] = f ? 1 : 0;
    if (o == i) {                                                                      // the claimant writes the record, then makes the slot FULL
        uint32_t r[16];
        nullset_load(a.nul + 64 * (size_t)i, r);
        const uint32_t h = a.slot[i];
        nullset_store(a.t.rec + 64 * (size_t)h, r);
        a.t.tag[h] = nullset_full_tag(a.t, r);
    }
    return f;
}

PLUME_HD void nullset_contains(const NullsetQueryArgs& a, uint32_t i) {
    uint32_t r[16];
    nullset_load(a.nul + 64 * (size_t)i, r);
    const uint32_t full = nullset_full_tag(a.t, r);
    uint32_t h = nullset_home(a.t, r);
    uint8_t f = 0;
    for (;;) {
        const uint32_t tag = a.t.tag[h];
        if (tag == PLUME_NS_EMPTY) break;
        if (tag == full && nullset_equal(a.t.rec + 64 * (size_t)h, r)) { f = 1; break; }
        h = (h + 1) & a.t.mask;
    }
    a.found[i] = f;
}

// old slot s -> the new table (whose tags are all EMPTY before the launch)
PLUME_HD void nullset_rehash(const NullsetTable& from, const NullsetTable& to, uint64_t s) {
    if (!nullset_is_full(from.tag[s])) return;
    uint32_t r[16];
    nullset_load(from.rec + 64 * s, r);
    const uint32_t full = nullset_full_tag(to, r);
    uint32_t h = nullset_home(to, r);
    while (PLUME_ATOMIC_CAS_U32(&to.tag[h], PLUME_NS_EMPTY, full) != PLUME_NS_EMPTY) h = (h + 1) & to.mask;
    nullset_store(to.rec + 64 * (size_t)h, r);
}

// export: the s-th slot's record, if any, to dst
PLUME_HD bool nullset_slot_full(const NullsetTable& t, uint64_t s) { return nullset_is_full(t.tag[s]); }
PLUME_HD void nullset_copy_out(const NullsetTable& t, uint64_t s, uint8_t* dst) {
    uint32_t r[16];
    nullset_load(t.rec + 64 * s, r);
    nullset_store(dst, r);
}

}  // namespace plume
