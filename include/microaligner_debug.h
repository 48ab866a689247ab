/* Test hook: fill the scratch memory a context keeps between calls with a chosen byte, so that a call which reads what
 * it has not written computes with that byte and not with what the previous call happened to leave there.  An extension
 * of libmicroaligner_hip.so with no counterpart in the reference; off the measured path (build.source_hash() does not
 * cover it) and called by nothing but tests. */
#ifndef MICROALIGNER_DEBUG_H
#define MICROALIGNER_DEBUG_H

#include "microaligner_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Waits for the ctx stream, the stream of the companion ctx (if ma_optflow_register has made one) and the three engine
 * streams; sets every byte of the idle scratch memory of ctx and of its companion to `byte` (0 .. 255); waits again.
 * Idle scratch memory is: the grow-only workspace, every buffer the 64 KiB-bucket cache holds free, the small device
 * buffer for taps and scalars, and the page-locked host buffer for scalar results.  filled[0 .. 3] (may be NULL) receive
 * the bytes filled of each kind, in that order, both contexts together.
 * Not touched: cache buffers in use, anything the caller holds (ma_malloc), the process-wide tap tables, the staging rings
 * of the transfer engines, the zero-flag buffers of the dog() chain.  MA_EINVAL for a NULL ctx or a byte out of range. */
int ma_debug_fill_idle(ma_ctx* ctx, int byte, unsigned long long filled[4]);

#ifdef __cplusplus
}
#endif

#endif /* MICROALIGNER_DEBUG_H */
