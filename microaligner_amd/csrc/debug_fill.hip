// Test hook (include/microaligner_debug.h): fill the idle scratch memory of a context and of its companion with one byte.
// Called by nothing but tests; launches no kernel.
#include <cstring>

#include "ma_internal.h"
#include "../../include/microaligner_debug.h"

static int sync_streams(ma_ctx* c)
{
    MA_HIP(hipStreamSynchronize(c->stream));
    for (int e = 0; e < 3; e++)
        if (c->engine[e]) MA_HIP(hipStreamSynchronize(c->engine[e]));
    return MA_OK;
}

// every byte of the four kinds of idle scratch memory of one ctx; pool_live, the staging rings, dog_sticky_buf and
// round_flags are in use or hold state across calls and stay as they are
static int fill_one(ma_ctx* c, int byte, unsigned long long n[4])
{
    if (c->ws && c->ws_bytes) {
        MA_HIP(hipMemsetAsync(c->ws, byte, c->ws_bytes, c->stream));
        n[0] += c->ws_bytes;
    }
    for (auto& kv : c->pool_free) {
        MA_HIP(hipMemsetAsync(kv.second, byte, kv.first, c->stream));
        n[1] += kv.first;
    }
    if (c->dconst && c->dconst_bytes) {
        MA_HIP(hipMemsetAsync(c->dconst, byte, c->dconst_bytes, c->stream));
        n[2] += c->dconst_bytes;
    }
    MA_HIP(hipStreamSynchronize(c->stream));
    if (c->pinned && c->pinned_bytes) {
        memset(c->pinned, byte, c->pinned_bytes);
        n[3] += c->pinned_bytes;
    }
    return MA_OK;
}

extern "C" int ma_debug_fill_idle(ma_ctx* ctx, int byte, unsigned long long filled[4])
{
    MA_REQUIRE(ctx, "ctx is NULL");
    MA_REQUIRE(byte >= 0 && byte <= 255, "byte must be in 0..255");
    MA_HIP(hipSetDevice(ctx->device));
    unsigned long long n[4] = {0, 0, 0, 0};
    MA_TRY(sync_streams(ctx));
    if (ctx->side) MA_TRY(sync_streams(ctx->side));
    MA_TRY(fill_one(ctx, byte, n));
    if (ctx->side) MA_TRY(fill_one(ctx->side, byte, n));
    MA_TRY(sync_streams(ctx));
    if (ctx->side) MA_TRY(sync_streams(ctx->side));
    if (filled)
        for (int k = 0; k < 4; k++) filled[k] = n[k];
    return MA_OK;
}
