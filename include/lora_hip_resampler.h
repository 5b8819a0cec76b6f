/*
 * lora_hip_resampler.h -- C ABI of the MI355X rational resampler: one stream stage from rate fs_in to rate fs_in * L / M, on the
 * device, in front of the channeliser, the filter bank or a gateway, for captures whose rate is no multiple of the LoRa bandwidth
 * (2.4 Msps -> 2.0 Msps is 5 / 6).  A handle of its own; it changes nothing the other handles do.  Float64 model of the same
 * definition: gr_lora_amd/resampler.py (resample).
 *
 * DEFINITION.  The stream is x[n], n = 0, 1, ..., with x[n < 0] = 0: cf32, or sc16 / sc8 / cu8 converted by lora_hip_iq_format's
 * table (lora_hip.h).  L / M is the ratio in lowest terms (the library reduces what it is given) and R = max(L, M).
 *   filter   ntaps = 2 Z R + 1;   h[k] = fl32( L * (c / R) * sinc((k - Z R) c / R) * kaiser_beta(k) ), formed in double and rounded
 *            once; sinc(t) = sin(pi t) / (pi t); kaiser_beta is the Kaiser window of length ntaps,
 *            I0(beta sqrt(1 - ((k - a) / a)^2)) / I0(beta) with a = (ntaps - 1) / 2.  Defaults: Z = 16 zero crossings per side,
 *            beta = 8.0, cutoff c = 0.8 of the lower of the two Nyquist rates.  Q = ceil(ntaps / L) taps per output; h[k >= ntaps]
 *            reads as 0.
 *   output   m:  t = m M,  p = t mod L,  n0 = t div L;   y[m] = sum_{j = 0 .. Q-1} h[p + j L] * x[n0 - j]        (cf32)
 *   count    after N input items in total exactly ceil(N L / M) outputs exist (every m with m M < N L); a call consumes all of
 *            n_in and emits the outputs its items complete, for every n_in, 0 included.
 *   delay    the group delay is Z R / M output items (lora_hip_resampler_delay).  Positions reported downstream refer to the
 *            resampled stream.
 *
 * SUMMATION ORDER (every "bit for bit" below follows from it).  An output is ONE ascending chain per component, j = 0, 1, ...,
 * Q - 1, starting from +0:  re = fma(h[p + j L], x[n0 - j].re, re),  im = fma(h[p + j L], x[n0 - j].im, im), every step one fused
 * multiply-add in fp32 (one rounding).  The order depends on j only: not on the chunking, the tile, the grid or the scheduling.
 * No float atomics.
 *
 * CARRIED STATE.  The last Q - 1 input items (cf32, on the device) and the next output's (n0, p) as 64-bit integers.  n0 counts
 * input items and grows by what is consumed; no product of an absolute count (m M, N L) is ever formed.
 *
 * Plain C types only; device pointers and the HIP stream travel as void*.  Same conventions as lora_hip_spectrum.h: every
 * argument check comes before any device call; no CPU fallback.
 */
#ifndef LORA_HIP_RESAMPLER_H
#define LORA_HIP_RESAMPLER_H

#include <stddef.h>
#include <stdint.h>

#include "lora_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Limits (LORA_HIP_ERR_BAD_CONFIG outside them, before any device call). */
#define LORA_HIP_RESAMPLER_MAX_RATIO 512u       /* 1 <= interpolation, decimation <= 512, as given (in any terms) */
#define LORA_HIP_RESAMPLER_MIN_ZERO_CROSSINGS 2u
#define LORA_HIP_RESAMPLER_MAX_ZERO_CROSSINGS 32u
#define LORA_HIP_RESAMPLER_MAX_BETA 20u         /* 0 <= beta <= 20 */
#define LORA_HIP_RESAMPLER_MAX_TAPS 16385u      /* ntaps = 2 Z R + 1 */
#define LORA_HIP_RESAMPLER_MAX_Q 1024u          /* taps per output; deep decimation is the channeliser's job */

typedef struct lora_hip_resampler_config {
    uint32_t struct_size;
    uint32_t interpolation;    /* L, in any terms */
    uint32_t decimation;       /* M */
    uint32_t zero_crossings;   /* Z (0 = 16) */
    double   beta;             /* Kaiser beta (0 = 8.0) */
    double   cutoff;           /* c of the lower Nyquist rate, 0 < c <= 1 (no zero default: 0 is refused) */
    int32_t  device;           /* HIP device ordinal */
    uint32_t flags;            /* reserved, 0 */
} lora_hip_resampler_config_t;

typedef struct lora_hip_resampler lora_hip_resampler_t;

/* LORA_HIP_ERR_ARG: cfg or out NULL, struct_size too small; LORA_HIP_ERR_BAD_CONFIG: a limit above, beta or cutoff out of range
 * or not a number, a flag bit set; LORA_HIP_ERR_NO_DEVICE: no such HIP device (no CPU fallback). */
lora_hip_status lora_hip_resampler_create(const lora_hip_resampler_config_t *cfg, lora_hip_resampler_t **out);
void            lora_hip_resampler_destroy(lora_hip_resampler_t *h);
const char     *lora_hip_resampler_last_error(const lora_hip_resampler_t *h);

/* The fp32 prototype h (ntaps values): *n receives ntaps; taps may be NULL to query it. */
lora_hip_status lora_hip_resampler_taps(const lora_hip_resampler_t *h, float *taps, size_t cap, size_t *n);

/* The reduced L and M, and Q (any pointer may be NULL). */
lora_hip_status lora_hip_resampler_ratio(const lora_hip_resampler_t *h, uint32_t *interpolation, uint32_t *decimation, uint32_t *q);

/* Z R / M, in output items (0 for a NULL handle). */
double          lora_hip_resampler_delay(const lora_hip_resampler_t *h);

/* The launch plan (read only; any pointer may be NULL): a workgroup of tile threads takes tiles_per_group consecutive tiles of
 * tile outputs; the phase table sits in LDS as L rows of row_stride floats beside the tile's input span, lds_bytes in all. */
lora_hip_status lora_hip_resampler_get_plan(const lora_hip_resampler_t *h, uint32_t *tile, uint32_t *tiles_per_group, uint32_t *row_stride,
                                            size_t *lds_bytes);

/* Outputs the next call will emit for n_in input items. */
size_t          lora_hip_resampler_output_items(const lora_hip_resampler_t *h, size_t n_in);

/* Streaming, device-resident: d_in = n_in cf32 items continuing the stream; *n_out cf32 items are written to d_out, and
 * *first_out is the absolute index m of the first of them.  LORA_HIP_ERR_OVERFLOW, with *n_out set and nothing consumed (the
 * stream is where it was), when n_in would yield more than max_out.  One launch; synchronous on return. */
lora_hip_status lora_hip_resampler_run_device(lora_hip_resampler_t *h, const void *d_in, size_t n_in, void *d_out, size_t max_out, size_t *n_out,
                                              uint64_t *first_out, void *hip_stream);

/* The same for n_in items of format fmt (lora_hip_iq_format, lora_hip.h: the conversion, scale and the checks made before any
 * device call): the kernel converts each item as it stages it, the carried items stay cf32.  Bit for bit the outputs of
 * lora_hip_resampler_run_device fed the converted items; the format may change from call to call. */
lora_hip_status lora_hip_resampler_run_device_raw(lora_hip_resampler_t *h, const void *d_in, size_t n_in, int fmt, float scale, void *d_out,
                                                  size_t max_out, size_t *n_out, uint64_t *first_out, void *hip_stream);

/* Same with host buffers: in = n_in cf32 items, out = room for max_out cf32 items. */
lora_hip_status lora_hip_resampler_work(lora_hip_resampler_t *h, const float *in, size_t n_in, float *out, size_t max_out, size_t *n_out,
                                        uint64_t *first_out);

/* Same with n_in host items of format fmt: the raw bytes are uploaded and converted by the kernel. */
lora_hip_status lora_hip_resampler_work_raw(lora_hip_resampler_t *h, const void *in, size_t n_in, int fmt, float scale, float *out, size_t max_out,
                                            size_t *n_out, uint64_t *first_out);

/* Drops the carried items; the next item is x[0] of a new stream and the next output is m = 0. */
lora_hip_status lora_hip_resampler_reset(lora_hip_resampler_t *h);

/* Kernel time of the last run (HIP events on the launch stream). */
float           lora_hip_resampler_last_kernel_ms(const lora_hip_resampler_t *h);

#ifdef __cplusplus
}
#endif
#endif /* LORA_HIP_RESAMPLER_H */
