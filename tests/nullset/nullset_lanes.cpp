// TEST INFRASTRUCTURE ONLY.  The per-lane bodies of csrc/plume_nullset.h compiled for the host (tests/test_nullset_lanes.py builds this with ASan + UBSan) and run the way the
// kernels run them -- one launch after another, the lanes of a launch in a random, reversed or forward permutation -- on tables of exactly the sizes the library
// allocates, against a std::set of the records and the definition of `fresh`.  Sequences of inserts with live masks and descending ids, growth between calls (rehash into a
// fresh key), clear, export round trips, contains after each step, and a 64-slot table where every record has the same home slot (the probes wrap around).
//   nullset_lanes <seed>
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <numeric>
#include <random>
#include <set>
#include <vector>

#include "plume_nullset.h"

using namespace plume;
using Rec = std::array<uint8_t, 64>;

#define REQUIRE(c)                                                                          \
    do {                                                                                    \
        if (!(c)) { std::fprintf(stderr, "nullset_lanes: %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(2); } \
    } while (0)

static std::mt19937_64 rng;

// lane orders: 0 forward, 1 reversed, 2 random
static std::vector<uint64_t> order(uint64_t n, int kind) {
    std::vector<uint64_t> o(n);
    std::iota(o.begin(), o.end(), 0);
    if (kind == 1) std::reverse(o.begin(), o.end());
    if (kind == 2) std::shuffle(o.begin(), o.end(), rng);
    return o;
}

struct Table {
    uint64_t cap = 0, size = 0;
    std::vector<uint8_t> rec;                 // exactly cap x 64 bytes (ASan sees any probe past the end)
    std::vector<uint32_t> tag;
    NullsetTable t{};
    void make(uint64_t c, const uint32_t* key = nullptr) {
        cap = c;
        rec.assign(64 * c, 0xA5);
        tag.assign(c, PLUME_NS_EMPTY);
        t.rec = rec.data(); t.tag = tag.data(); t.mask = (uint32_t)(c - 1);
        for (int k = 0; k < 4; k++) t.key[k] = key ? key[k] : (uint32_t)rng();
        t.key[1] |= 1u; t.key[3] |= 1u;
    }
};

static void grow(Table& tb, uint64_t new_cap) {
    Table nt;
    nt.make(new_cap);
    for (uint64_t s : order(tb.cap, (int)(rng() % 3))) nullset_rehash(tb.t, nt.t, s);
    nt.size = tb.size;
    tb = std::move(nt);
    tb.t.rec = tb.rec.data(); tb.t.tag = tb.tag.data();
}

struct Call {
    size_t n = 0;
    std::vector<uint8_t> nul, live;
    std::vector<uint64_t> ids;
    bool with_live = false, with_ids = false;
};

static Rec rec_at(const uint8_t* p) { Rec r; std::memcpy(r.data(), p, 64); return r; }

// one insert through the lane bodies, the lanes of each launch in their own order; checked against the definition
static void insert(Table& tb, const Call& c, std::set<Rec>& S, int kind, bool may_grow = true) {
    if (may_grow && tb.size + c.n > tb.cap / 2) grow(tb, nullset_table_size(tb.size + c.n));
    std::vector<uint8_t> fresh(c.n, 0xEE);
    std::vector<uint32_t> owner(c.n, 0xA5A5A5A5u), slot(c.n, 0xA5A5A5A5u);
    std::vector<unsigned long long> minid(c.n, ~0ull);
    NullsetInsertArgs a{};
    a.t = tb.t; a.n = (uint32_t)c.n; a.nul = c.nul.data(); a.live = c.with_live ? c.live.data() : nullptr; a.ids = c.with_ids ? c.ids.data() : nullptr;
    a.fresh = fresh.data(); a.owner = owner.data(); a.slot = slot.data(); a.minid = minid.data();
    for (uint64_t i : order(c.n, kind)) nullset_probe(a, (uint32_t)i);
    uint64_t cnt = 0;
    for (uint64_t i : order(c.n, (kind + 1) % 3)) cnt += nullset_commit(a, (uint32_t)i) ? 1 : 0;
    tb.size += cnt;
    // the definition
    std::map<Rec, uint64_t> best;
    for (size_t i = 0; i < c.n; i++) {
        if (c.with_live && !c.live[i]) continue;
        const uint64_t id = c.with_ids ? c.ids[i] : i;
        auto it = best.find(rec_at(&c.nul[64 * i]));
        if (it == best.end() || id < it->second) best[rec_at(&c.nul[64 * i])] = id;
    }
    uint64_t want = 0;
    for (size_t i = 0; i < c.n; i++) {
        const bool live = !c.with_live || c.live[i];
        const Rec r = rec_at(&c.nul[64 * i]);
        const bool f = live && !S.count(r) && best[r] == (c.with_ids ? c.ids[i] : i);
        REQUIRE(fresh[i] == (f ? 1 : 0));
        want += f;
    }
    REQUIRE(cnt == want);
    for (auto& kv : best) S.insert(kv.first);
    REQUIRE(tb.size == S.size());
}

static void check_contains(const Table& tb, const std::set<Rec>& S, const std::vector<Rec>& pool) {
    std::vector<uint8_t> q(64 * pool.size()), found(pool.size(), 0xEE);
    for (size_t j = 0; j < pool.size(); j++) std::memcpy(&q[64 * j], pool[j].data(), 64);
    NullsetQueryArgs a{};
    a.t = tb.t; a.n = (uint32_t)pool.size(); a.nul = q.data(); a.found = found.data();
    for (uint64_t i : order(pool.size(), 2)) nullset_contains(a, (uint32_t)i);
    for (size_t j = 0; j < pool.size(); j++) REQUIRE(found[j] == (S.count(pool[j]) ? 1 : 0));
}

// export as the kernels do it: count per block of slots, scan, scatter; the records must be S exactly
static std::vector<uint8_t> export_all(const Table& tb) {
    const uint64_t per = 256ull * PLUME_NS_EXPORT_PER_LANE, nb = (tb.cap + per - 1) / per;
    std::vector<uint64_t> first(nb);
    uint64_t total = 0;
    for (uint64_t b = 0; b < nb; b++) {
        first[b] = total;
        for (uint64_t s = b * per; s < std::min(tb.cap, (b + 1) * per); s++) total += nullset_slot_full(tb.t, s);
    }
    std::vector<uint8_t> out(64 * total);
    for (uint64_t b : order(nb, 2)) {
        uint64_t row = first[b];
        for (uint64_t s = b * per; s < std::min(tb.cap, (b + 1) * per); s++) if (nullset_slot_full(tb.t, s)) nullset_copy_out(tb.t, s, &out[64 * row++]);
    }
    return out;
}

static std::vector<Rec> make_pool(size_t k) {
    std::vector<Rec> pool(k);
    for (auto& r : pool) for (auto& b : r) b = (uint8_t)rng();
    pool[0].fill(0);
    pool[2] = pool[1]; pool[2][63] ^= 1;
    return pool;
}
static Call make_call(size_t n, const std::vector<Rec>& pool) {
    Call c;
    c.n = n;
    c.nul.resize(64 * n);
    c.live.resize(n);
    c.ids.resize(n);
    c.with_live = rng() % 2;
    c.with_ids = rng() % 2;
    for (size_t i = 0; i < n; i++) {
        std::memcpy(&c.nul[64 * i], pool[rng() % pool.size()].data(), 64);
        c.live[i] = rng() % 4 != 0;
        c.ids[i] = (1ull << 50) - 7 * i;               // descending: later duplicates win
    }
    return c;
}

static void sequences() {
    const std::vector<Rec> pool = make_pool(900);
    Table tb;
    tb.make(64);
    std::set<Rec> S;
    for (int round = 0; round < 2; round++) {
        for (size_t n : {1, 7, 64, 65, 300, 1000, 0, 2500, 33}) {
            insert(tb, make_call(n, pool), S, (int)(rng() % 3));
            check_contains(tb, S, pool);
            REQUIRE(2 * tb.size <= tb.cap);
        }
        // export round trip into a fresh table of another size and key
        const std::vector<uint8_t> out = export_all(tb);
        std::set<Rec> got;
        for (size_t j = 0; j < out.size() / 64; j++) got.insert(rec_at(&out[64 * j]));
        REQUIRE(got == S && out.size() / 64 == S.size());
        Table copy;
        copy.make(nullset_table_size(S.size() / 3 + 1));
        std::set<Rec> S2;
        Call c;
        c.n = out.size() / 64; c.nul = out; c.live.assign(c.n, 1); c.ids.resize(c.n);
        insert(copy, c, S2, 1);
        REQUIRE(S2 == S);
        check_contains(copy, S, pool);
        // clear
        std::fill(tb.tag.begin(), tb.tag.end(), PLUME_NS_EMPTY);
        tb.size = 0;
        S.clear();
        check_contains(tb, S, pool);
    }
}

// every record has the same home slot in a 64-slot table (found by trying random records under the table's key), near the end so that the probes wrap around
static void collisions() {
    Table tb;
    tb.make(64);
    const uint32_t home = 60;
    std::vector<Rec> pool;
    while (pool.size() < 32) {
        Rec r;
        for (auto& b : r) b = (uint8_t)rng();
        uint32_t w[16];
        std::memcpy(w, r.data(), 64);
        if (nullset_home(tb.t, w) == home) pool.push_back(r);
    }
    std::set<Rec> S;
    for (int k = 0; k < 4; k++) {
        std::vector<Rec> part(pool.begin(), pool.begin() + 8 * (k + 1));
        Call c;
        c.n = part.size() + 8;                         // every record so far, then repeats
        c.nul.resize(64 * c.n); c.live.assign(c.n, 1); c.ids.resize(c.n); c.with_ids = true;
        for (size_t i = 0; i < c.n; i++) { std::memcpy(&c.nul[64 * i], part[i < part.size() ? i : rng() % part.size()].data(), 64); c.ids[i] = 1000 - i; }
        insert(tb, c, S, k % 3, false);                // (at most 32 distinct records: the table never passes half full)
        check_contains(tb, S, pool);
    }
    REQUIRE(S.size() == 32);
    for (uint32_t s = 0; s < 64; s++) REQUIRE((tb.tag[s] != PLUME_NS_EMPTY) == (s >= home || s < home + 32 - 64));
}

int main(int argc, char** argv) {
    const unsigned long long seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
    rng.seed(seed * 0x9E3779B97F4A7C15ull + 99);
    REQUIRE(nullset_table_size(0) == 64 && nullset_table_size(32) == 64 && nullset_table_size(33) == 128 && nullset_table_size(1ull << 31) == (1ull << 32));
    sequences();
    collisions();
    std::printf("nullset_lanes %llu ok\n", seed);
    return 0;
}
