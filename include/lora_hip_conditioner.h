/*
 * lora_hip_conditioner.h -- C ABI of the MI355X IQ conditioner: one stream stage that removes what a direct-conversion front end
 * adds to a capture, a DC offset and a gain / phase mismatch between I and Q, on the device, in front of the resampler, the
 * channeliser, the filter bank or a gateway.  cf32 or sc16 / sc8 / cu8 in, cf32 out at the input's rate, item for item.  A handle of
 * its own; it changes nothing the other handles do.  Float64 model of the same definition: gr_lora_amd/conditioner.py (condition).
 *
 * DEFINITION.  The stream is x[n] = I[n] + j Q[n], n = 0, 1, ...: cf32, or sc16 / sc8 / cu8 converted by lora_hip_iq_format's table
 * (lora_hip.h).  Block k is items k B .. k B + B - 1, B a power of two; the window is W blocks.
 *   moments     every block has five sums in fp64, S_I, S_Q, S_II, S_QQ, S_IQ, of the items converted to double first, so every
 *               product is exact in double.
 *   window      block k's window sums run over the blocks max(0, k - W + 1) .. k, ascending, from +0, in fp64;
 *               cnt = (k - lo + 1) B.  (After lora_hip_conditioner_set_adaptive the window starts again at the next block.)
 *   estimates   fp64, each line one IEEE operation per operator as written, no contraction:
 *                 mI  = S_I / cnt            mQ  = S_Q / cnt
 *                 cII = S_II / cnt - mI mI   cQQ = S_QQ / cnt - mQ mQ   cIQ = S_IQ / cnt - mI mQ
 *                 r   = cIQ / cII            q   = cQQ / cII            e   = q - r r
 *                 b   = 1 / sqrt(e)          a   = -r b
 *               guard: unless cII > 0 and e > 2^-12 both hold (a NaN fails either), a = 0 and b = 1.  A block of exact zeros or of
 *               one constant therefore comes out finite.
 *   parameters  dI = fl32(mI), dQ = fl32(mQ), fl32(a), fl32(b): rounded once.  Without LORA_HIP_CONDITIONER_FLAG_DC dI = dQ = 0,
 *               without LORA_HIP_CONDITIONER_FLAG_IQ a = 0 and b = 1; the estimates use centred moments either way.
 *   output      block k with block k's parameters (its own block is inside its window), in fp32, one rounding per operation:
 *                 zI = I - dI      u = Q - dQ      zQ = (a zI) + (b u)
 *   model       for a proper signal behind y = I + j g (Q cos phi + I sin phi) + d:  cII = P, cIQ = g sin phi P, cQQ = g^2 P, so
 *               a = -tan phi and b = 1 / (g cos phi) undo the mismatch and leave I's scale untouched.
 *   counts      a call consumes all of n_in and emits the blocks its items complete, item-aligned with the input (no delay); at
 *               most B - 1 items are held back.  flush emits the held items with the parameters of the last complete block
 *               (identity if there was none); the item after a flush starts a new block, counters and window carry on.
 *
 * SUMMATION ORDER (every "bit for bit" below follows from it; it is fixed by B alone).  A block is B / 64 rows of 64 items.  Chain
 * p, p = 0 .. 63, starts from +0 and adds the terms of items p, p + 64, p + 128, ... of the block in ascending order.  The 64
 * totals t[0 .. 63] are then reduced by a halving tree: for s = 32, 16, 8, 4, 2, 1:  t[i] = t[i] + t[i + s] for every i < s; the
 * sum is t[0].  The five sums are five such reductions.  Nothing depends on the chunking, the input format, the grid or the
 * scheduling.  No float atomics.
 *
 * CARRIED STATE.  The partial block (cf32, on the device), the last W - 1 block records (on the device), 64-bit item and block
 * counters.
 *
 * Plain C types only; device pointers and the HIP stream travel as void*.  Same conventions as lora_hip_resampler.h: every
 * argument check comes before any device call; no CPU fallback.
 */
#ifndef LORA_HIP_CONDITIONER_H
#define LORA_HIP_CONDITIONER_H

#include <stddef.h>
#include <stdint.h>

#include "lora_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Limits (LORA_HIP_ERR_BAD_CONFIG outside them, before any device call). */
#define LORA_HIP_CONDITIONER_MIN_BLOCK 256u     /* B: a power of two, 256 .. 65536 (0 = 4096) */
#define LORA_HIP_CONDITIONER_MAX_BLOCK 65536u
#define LORA_HIP_CONDITIONER_MAX_WINDOW 256u    /* W: 1 .. 256 blocks (0 = 16) */

#define LORA_HIP_CONDITIONER_FLAG_DC 1u         /* remove the DC offset */
#define LORA_HIP_CONDITIONER_FLAG_IQ 2u         /* correct the IQ imbalance */

typedef struct lora_hip_conditioner_config {
    uint32_t struct_size;
    uint32_t block;     /* B (0 = 4096) */
    uint32_t window;    /* W (0 = 16) */
    uint32_t flags;     /* LORA_HIP_CONDITIONER_FLAG_*; any other bit is refused */
    int32_t  device;    /* HIP device ordinal */
} lora_hip_conditioner_config_t;

typedef struct lora_hip_conditioner lora_hip_conditioner_t;

/* LORA_HIP_ERR_ARG: cfg or out NULL, struct_size too small; LORA_HIP_ERR_BAD_CONFIG: a limit above, an unknown flag bit;
 * LORA_HIP_ERR_NO_DEVICE: no such HIP device (no CPU fallback). */
lora_hip_status lora_hip_conditioner_create(const lora_hip_conditioner_config_t *cfg, lora_hip_conditioner_t **out);
void            lora_hip_conditioner_destroy(lora_hip_conditioner_t *h);
const char     *lora_hip_conditioner_last_error(const lora_hip_conditioner_t *h);

/* Items the next call will emit for n_in input items: B times the blocks they complete. */
size_t          lora_hip_conditioner_output_items(const lora_hip_conditioner_t *h, size_t n_in);

/* The launch plan (read only; any pointer may be NULL): B and W; the moments kernel gives every block one wavefront,
 * blocks_per_group of them to a workgroup; a workgroup of the apply kernel streams items_per_group items of one block. */
lora_hip_status lora_hip_conditioner_get_plan(const lora_hip_conditioner_t *h, uint32_t *block, uint32_t *window, uint32_t *blocks_per_group,
                                              uint32_t *items_per_group);

/* Streaming, device-resident: d_in = n_in cf32 items continuing the stream; *n_out cf32 items are written to d_out (8-byte
 * aligned), and *first_out is the absolute index of the first of them.  d_out may not overlap d_in (LORA_HIP_ERR_ARG).
 * LORA_HIP_ERR_OVERFLOW, with *n_out set and nothing consumed (the stream is where it was), when n_in would yield more than
 * max_out.  Two launches on hip_stream with no host synchronisation between them; synchronous on return. */
lora_hip_status lora_hip_conditioner_run_device(lora_hip_conditioner_t *h, const void *d_in, size_t n_in, void *d_out, size_t max_out, size_t *n_out,
                                                uint64_t *first_out, void *hip_stream);

/* The same for n_in items of format fmt (lora_hip_iq_format, lora_hip.h: the conversion, scale and the checks made before any
 * device call): the kernels convert each item as they load it, the held items stay cf32.  Bit for bit the outputs and records of
 * lora_hip_conditioner_run_device fed the converted items; the format may change from call to call. */
lora_hip_status lora_hip_conditioner_run_device_raw(lora_hip_conditioner_t *h, const void *d_in, size_t n_in, int fmt, float scale, void *d_out,
                                                    size_t max_out, size_t *n_out, uint64_t *first_out, void *hip_stream);

/* Same with host buffers: in = n_in cf32 items, out = room for max_out cf32 items. */
lora_hip_status lora_hip_conditioner_work(lora_hip_conditioner_t *h, const float *in, size_t n_in, float *out, size_t max_out, size_t *n_out,
                                          uint64_t *first_out);

/* Same with n_in host items of format fmt: the raw bytes are uploaded and converted by the kernels. */
lora_hip_status lora_hip_conditioner_work_raw(lora_hip_conditioner_t *h, const void *in, size_t n_in, int fmt, float scale, float *out, size_t max_out,
                                              size_t *n_out, uint64_t *first_out);

/* Emits the held items (at most B - 1) with the newest parameters; LORA_HIP_ERR_OVERFLOW with *n_out set and nothing emitted
 * when they do not fit. */
lora_hip_status lora_hip_conditioner_flush_device(lora_hip_conditioner_t *h, void *d_out, size_t max_out, size_t *n_out, uint64_t *first_out,
                                                  void *hip_stream);
lora_hip_status lora_hip_conditioner_flush(lora_hip_conditioner_t *h, float *out, size_t max_out, size_t *n_out, uint64_t *first_out);

/* Drops the held items and the window: the next item is x[0] of a new stream, block 0, identity parameters.  The mode (fixed or
 * adaptive) stays. */
lora_hip_status lora_hip_conditioner_reset(lora_hip_conditioner_t *h);

/* Fixed mode, for an installation that has measured its front end: every item from the next call on gets exactly these four
 * constants (all finite, LORA_HIP_ERR_ARG otherwise) and nothing is estimated; the records of such a call hold zero moments. */
lora_hip_status lora_hip_conditioner_set_fixed(lora_hip_conditioner_t *h, float d_i, float d_q, float a, float b);
/* Back to estimation; the window starts again at the next block. */
lora_hip_status lora_hip_conditioner_set_adaptive(lora_hip_conditioner_t *h);

/* For tests and monitoring.  The records of the blocks the last run call completed: *n receives their number; moments (5 doubles
 * per block: S_I, S_Q, S_II, S_QQ, S_IQ) and params (4 floats per block: dI, dQ, a, b) are filled when not NULL and cap >= *n
 * blocks (LORA_HIP_ERR_OVERFLOW otherwise).  Separately the newest block of the stream, whichever call completed it:
 * newest_params (4 floats; what flush applies) and newest_estimates (4 doubles: mI, mQ, r, q of the definition, whatever the flags,
 * of the newest block that was estimated; zeros before the first).  Any pointer but n may be NULL. */
lora_hip_status lora_hip_conditioner_block_records(lora_hip_conditioner_t *h, double *moments, float *params, size_t cap, size_t *n,
                                                   float *newest_params, double *newest_estimates);

/* Kernel time of the last run (HIP events on the launch stream, both launches). */
float           lora_hip_conditioner_last_kernel_ms(const lora_hip_conditioner_t *h);

#ifdef __cplusplus
}
#endif
#endif /* LORA_HIP_CONDITIONER_H */
