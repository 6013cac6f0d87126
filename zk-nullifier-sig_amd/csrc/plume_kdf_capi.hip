// PBKDF2-HMAC-SHA512 for a batch (include/plume_hip.h, plume_pbkdf2_sha512_batch*): its C ABI and its host side.  Three kernels around ctx->kdfws, the midstates, U and T
// of every item (256 B / item): key, then the remaining iterations in slices of PLUME_KDF_SLICE, then finish.  No table.  The device form joins the ws_free chain; behind
// the last kernel, and on every path out of a call that fails half way, the workspace is wiped on the call's stream (StageWipe), in front of ws_free.  The host-pointer
// form is a serial call (serial_host_call_any) whose messages are the passwords, staged as secrets; the salt is a secret input, whole when shared; the output is secret.
#include <cstdlib>
#include <cstring>

#include "../../include/plume_hip.h"
#include "plume_capi_ctx.h"
#include "plume_kdf_launch.h"

using namespace plume;

static_assert(PLUME_KDF_BIP39 == PLUME_KDFK_BIP39 && PLUME_KDF_SHARED_SALT == PLUME_KDFK_SHARED_SALT && PLUME_KDF_MAX_SALT == PLUME_KDFK_MAX_SALT &&
                  PLUME_STATUS_KDF_BAD_INPUT == PLUME_ST_KDF_BAD_INPUT,
              "the header and the kernels state the same constants");

// the rounds per k_kdf_iter dispatch: PLUME_KDF_SLICE, or env PLUME_KDF_SLICE (measurement only: tests/gpu_debug/kdf_timing.py sweeps it; 0 = one dispatch for all)
static uint32_t kdf_slice() {
    const char* e = std::getenv("PLUME_KDF_SLICE");
    if (!e || !*e) return PLUME_KDF_SLICE;
    const unsigned long v = std::strtoul(e, nullptr, 10);
    return v == 0 || v > PLUME_KDF_MAX_ITERATIONS ? PLUME_KDF_MAX_ITERATIONS : (uint32_t)v;
}

static int kdf_args_ok(int flags, size_t n, const void* pw_off, const void* salt, size_t salt_len, uint32_t iterations, size_t dklen, const void* out, const void* status) {
    if (flags & ~(PLUME_KDFK_BIP39 | PLUME_KDFK_SHARED_SALT)) return fail(PLUME_ERR_ARG, "unknown flag bits");
    if (iterations < 1 || iterations > PLUME_KDF_MAX_ITERATIONS) return fail(PLUME_ERR_ARG, "iterations must be 1 .. PLUME_KDF_MAX_ITERATIONS");
    if (dklen < 1 || dklen > 64) return fail(PLUME_ERR_ARG, "dklen must be 1 .. 64 (one output block)");
    if (salt_len > PLUME_KDFK_MAX_SALT) return fail(PLUME_ERR_ARG, "salt_len must be 0 .. PLUME_KDF_MAX_SALT");
    if (n && (!pw_off || !out || !status || (salt_len && !salt))) return fail(PLUME_ERR_ARG, "null array");
    if (n > 0xFFFFFFF0u / 64) return fail(PLUME_ERR_ARG, "n too large");
    return 0;
}
static int kdf_device(plume_ctx* ctx, int flags, size_t n, const uint8_t* pw, const uint64_t* pw_off, size_t pw_bytes, const uint8_t* salt, size_t salt_len,
                      uint32_t iterations, size_t dklen, uint8_t* out, uint8_t* status, hipStream_t st) {
    if (n == 0) return 0;
    if (n > ctx->chunk) return fail(PLUME_ERR_ARG, "n exceeds the chunk size (plume_set_chunk)");
    if (!pw && pw_bytes) return fail(PLUME_ERR_ARG, "null password buffer");
    if (int rc = ws_acquire(ctx, st)) return rc;
    WsHold hold(ctx, st);
    const size_t ws_bytes = (size_t)PLUME_KDFK_WS_WORDS * 8 * n;
    if (ctx->kdfws.ensure(ws_bytes)) return PLUME_ERR_HIP;
    struct StageWipe {                                                          // every path out of here, in front of ws_free (~WsHold runs later): midstates, U, T
        plume_ctx* ctx; size_t ws; hipStream_t st;
        ~StageWipe() { (void)hipMemsetAsync(ctx->kdfws.p, 0, ws, st); }
    };
    KdfArgs a;
    memset(&a, 0, sizeof a);
    a.flags = flags; a.n = (uint32_t)n; a.salt_len = (uint32_t)salt_len; a.dklen = (uint32_t)dklen;
    a.pw = pw; a.pw_off = pw_off; a.pw_bytes = pw_bytes; a.salt = salt; a.out = out; a.status = status; a.ws = ctx->kdfws.as<uint64_t>();
    StageTimer& t = ctx->timer;
    t.begin(st);
    {
        StageWipe wipe{ctx, ws_bytes, st};
        launch_kdf_key(a, st); t.stage("kdf_key", st);
        const uint32_t slice = kdf_slice();
        for (uint32_t left = iterations - 1; left;) {
            a.iters = left < slice ? left : slice;
            launch_kdf_iter(a, st); t.stage("kdf_iter", st);
            left -= a.iters;
        }
        launch_kdf_finish(a, st); t.stage("kdf_finish", st);
    }
    HIPCHK(hipGetLastError());
    return hold.release();
}
extern "C" int plume_pbkdf2_sha512_batch_device(plume_ctx* ctx, int flags, size_t n, const uint8_t* pw, const uint64_t* pw_off, size_t pw_bytes, const uint8_t* salt,
                                                size_t salt_len, uint32_t iterations, size_t dklen, uint8_t* out, uint8_t* status, void* stream) {
    Route rt_(ctx, stream, n); ctx = rt_.lane; const hipStream_t st_ = rt_.st;
    if (int rc = bind(ctx)) return rc;
    if (int rc = kdf_args_ok(flags, n, pw_off, salt, salt_len, iterations, dklen, out, status)) return rc;
    return kdf_device(ctx, flags, n, pw, pw_off, pw_bytes, salt, salt_len, iterations, dklen, out, status, st_);
}
extern "C" int plume_pbkdf2_sha512_batch(plume_ctx* ctx, int flags, size_t n, const uint8_t* pw, const uint64_t* pw_off, const uint8_t* salt, size_t salt_len,
                                         uint32_t iterations, size_t dklen, uint8_t* out, uint8_t* status) {
    if (!ctx) return fail(PLUME_ERR_ARG, "null context");
    if (int rc = kdf_args_ok(flags, n, pw_off, salt, salt_len, iterations, dklen, out, status)) return rc;
    // the offsets of the whole call, before anything is staged or written: a piece only ever sees its own
    for (size_t i = 0; i < n; i++)
        if (pw_off[i + 1] < pw_off[i]) return fail(PLUME_ERR_ARG, "pw_off is not non-decreasing");
    if (n && pw_off[n] > pw_off[0] && !pw) return fail(PLUME_ERR_ARG, "null password buffer");
    const bool one_salt = (flags & PLUME_KDFK_SHARED_SALT) != 0;
    HostCall call{pw, pw_off, {{salt_len ? salt : nullptr, salt_len, true, one_salt}}, {{out, dklen, true}, {status, 1}}};
    call.msgs_secret = true; call.off_name = "pw_off"; call.msgs_name = "password";
    return serial_host_call_any(ctx, n, call, [&](HostSlot& sl, size_t cnt, plume_ctx* on) -> int {
        return kdf_device(on, flags, cnt, sl.msgs.as<uint8_t>(), sl.off.as<uint64_t>(), (size_t)sl.rel[cnt], salt_len ? sl.in[0].as<uint8_t>() : nullptr, salt_len, iterations,
                          dklen, sl.out[0].as<uint8_t>(), sl.out[1].as<uint8_t>(), on->stream);
    });
}
