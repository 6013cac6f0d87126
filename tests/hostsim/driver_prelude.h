// TEST INFRASTRUCTURE ONLY.  What every call family's driver (tests/hostsim/*_driver.cpp, built and run by tests/_hostsim.py) opens with.  A driver defines DRIVER_NAME, a
// string literal, and includes this.  A failed REQUIRE prints "<name>: file:line: condition   [g_what] (the library's last error)" and exits with status 2: the tests match
// on that text.  (Everything is inline: a driver that does not use a piece gets no warning under -Werror.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../include/plume_hip.h"

#ifndef DRIVER_NAME
#error "define DRIVER_NAME before including driver_prelude.h"
#endif

inline std::string g_what;                                // what the driver is doing, for REQUIRE's message
#define REQUIRE(c)                                                                                                                       \
    do {                                                                                                                                 \
        if (!(c)) { std::fprintf(stderr, DRIVER_NAME ": %s:%d: %s   [%s] (%s)\n", __FILE__, __LINE__, #c, g_what.c_str(), plume_last_error()); std::exit(2); } \
    } while (0)

inline std::mt19937_64 rng;
constexpr uint8_t kFill = 0xAA;                           // what an output array holds before a call
inline bool all_of(const uint8_t* p, size_t bytes, uint8_t v) { for (size_t i = 0; i < bytes; i++) if (p[i] != v) return false; return true; }

// a caller array of exactly `bytes`, a copy of src or pre-filled
struct Arr {
    uint8_t* p = nullptr;
    size_t bytes = 0;
    int kind;                                             // 0 pageable, 1 page-locked, 2 device
    Arr(size_t b, int k, const void* src = nullptr) : bytes(b), kind(k) {
        if (k == 2) REQUIRE(hipMalloc((void**)&p, b ? b : 1) == hipSuccess); else p = (uint8_t*)(k ? plume_host_alloc(b ? b : 1) : std::malloc(b ? b : 1));
        REQUIRE(p);
        if (src) std::memcpy(p, src, b); else std::memset(p, kFill, b);
    }
    ~Arr() { if (kind == 2) (void)hipFree(p); else if (kind) plume_host_free(p); else std::free(p); }
    Arr(const Arr&) = delete;
    Arr& operator=(const Arr&) = delete;
    bool untouched() const { return all_of(p, bytes, kFill); }
};

// the stage names of the context's last call (stage timing on)
inline std::vector<std::string> last_stage_names(plume_ctx* ctx) {
    const char* names[64]; float ms[64];
    const int k = plume_last_stage_times(ctx, names, ms, 64);
    REQUIRE(k > 0 && k <= 64);
    return std::vector<std::string>(names, names + k);
}

// the mock runtime's live device allocations, host allocations, streams and events: taken before, compared after, nothing leaked
struct Outstanding {
    long v[4];
    Outstanding() { for (int k = 0; k < 4; k++) v[k] = mockhip::outstanding(k); }
    bool operator==(const Outstanding& o) const { return v[0] == o.v[0] && v[1] == o.v[1] && v[2] == o.v[2] && v[3] == o.v[3]; }
};
