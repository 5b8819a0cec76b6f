/*
 * lora_hip_filterbank.h -- C ABI of the MI355X polyphase DFT filter bank: the channeliser for a uniform channel grid
 * (a gateway's band plan: EU868's 8 channels, US915's 64 uplink channels, 200 kHz apart).
 *
 * Row c of the output is what the channeliser (include/lora_hip_channelizer.h) outputs for ONE channel at
 *     f = grid_offset_hz + channels[c] * samp_rate / n_grid          (Hz from the capture's centre)
 * with the same low-pass taps h (firdes::low_pass, same defaults and overrides):
 *     y[m] = sum_n h[n] x[mD - n] e^{-j 2 pi f (mD - n) / fs},   x[n < 0] = 0.
 * Computed as premix by grid_offset_hz, M = n_grid polyphase branch sums, and an M-point DFT evaluated for the selected
 * grid indices only: per output time one pass over the taps plus M * n_channels complex products, shared by every channel,
 * instead of a full FIR per channel.  Nothing needs to divide anything: M need not be a power of two, and neither of M
 * and the decimation D needs to divide the other.
 * Plain C types only; device pointers and the HIP stream travel as void*.  Same conventions as lora_hip.h.
 */
#ifndef LORA_HIP_FILTERBANK_H
#define LORA_HIP_FILTERBANK_H

#include <stddef.h>
#include <stdint.h>

#include "lora_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Limits (LORA_HIP_ERR_BAD_CONFIG outside them, before any device call). */
#define LORA_HIP_FILTERBANK_MAX_GRID 256u      /* 1 <= n_grid <= 256 */
#define LORA_HIP_FILTERBANK_MAX_DECIMATION 1024u /* 1 <= decimation <= 1024 */
#define LORA_HIP_FILTERBANK_MAX_TAPS 16384u    /* 2 <= 53 samp_rate / (22 transition) < 16384: the low-pass design's tap count (16 Msps at
                                                * the defaults: 3 855); below 2 it has one tap, whose Hamming window is 0 / 0 */
#define LORA_HIP_FILTERBANK_MAX_DST 8u         /* 1 <= n_dst <= 8 destinations per row (run_device_rows) */

typedef struct lora_hip_filterbank_config {
    uint32_t       struct_size;
    double         samp_rate;       /* fs of the wide-band input (Hz), > 0 */
    double         grid_offset_hz;  /* f0: frequency of grid index 0, relative to the capture's centre (Hz), finite */
    uint32_t       n_grid;          /* M: grid spacing fs / M */
    const int32_t *channels;        /* n_channels distinct grid indices in [-floor(M/2), ceil(M/2) - 1]; row c = channels[c] */
    uint32_t       n_channels;      /* 1 .. M */
    uint32_t       bandwidth;       /* LoRa bandwidth (Hz): default cutoff bandwidth/2 + 15 kHz, as the channeliser */
    uint32_t       decimation;      /* D: output rate fs / D */
    int32_t        device;          /* HIP device ordinal */
    float          cutoff_hz;       /* filter design overrides, 0 = the channeliser's own (cutoff bandwidth/2 + 15 kHz, */
    float          transition_hz;   /*   transition 10 kHz)                                                             */
    uint32_t       flags;           /* reserved, 0 */
} lora_hip_filterbank_config_t;

typedef struct lora_hip_filterbank lora_hip_filterbank_t;

/* LORA_HIP_ERR_ARG: cfg or out NULL, struct_size too small, channels NULL; LORA_HIP_ERR_BAD_CONFIG: a limit above, an index
 * out of range or repeated, samp_rate <= 0, flags != 0; LORA_HIP_ERR_NO_DEVICE: no such HIP device (no CPU fallback). */
lora_hip_status lora_hip_filterbank_create(const lora_hip_filterbank_config_t *cfg, lora_hip_filterbank_t **out);
void            lora_hip_filterbank_destroy(lora_hip_filterbank_t *h);
const char     *lora_hip_filterbank_last_error(const lora_hip_filterbank_t *h);

/* The low-pass prototype: *n receives the tap count; taps may be NULL to query it. */
lora_hip_status lora_hip_filterbank_taps(const lora_hip_filterbank_t *h, float *taps, size_t cap, size_t *n);

/* Output items per row the next call will produce for n_in input items (depends on the decimation phase carried over). */
size_t          lora_hip_filterbank_output_items(const lora_hip_filterbank_t *h, size_t n_in);

/* Streaming, device-resident: d_in = n_in cf32 items continuing the input stream; d_out receives n_channels rows of
 * out_stride cf32 items, row c = channels[c], *n_out items valid per row.  Filter history, absolute sample index (the
 * premix phase) and decimation phase carry over between calls: any chunking gives the same output stream.  One kernel
 * launch per call; synchronous on return.                                                                           */
lora_hip_status lora_hip_filterbank_run_device(lora_hip_filterbank_t *h, const void *d_in, size_t n_in, void *d_out,
                                               size_t out_stride, size_t *n_out, void *hip_stream);

/* The same for n_in items of format fmt (lora_hip_iq_format, lora_hip.h: the conversion, scale and the checks made before any
 * device call): the kernel converts each item as it stages it, the history stays cf32.  Bit for bit the rows of
 * lora_hip_filterbank_run_device fed the converted items; the format may change from call to call. */
lora_hip_status lora_hip_filterbank_run_device_raw(lora_hip_filterbank_t *h, const void *d_in, size_t n_in, int fmt, float scale,
                                                   void *d_out, size_t out_stride, size_t *n_out, void *hip_stream);

/* Same stream, each row stored to n_dst destinations (1 .. LORA_HIP_FILTERBANK_MAX_DST) instead of one 2-D buffer:
 * row_ptrs is a HOST array of n_dst * n_channels device pointers, row_ptrs[dst * n_channels + c] = where row c's first new item
 * goes for destination dst (any stride between them, any offset, 8-byte aligned).  Every destination receives the same bits
 * as lora_hip_filterbank_run_device's row.  The caller chooses n_in (lora_hip_filterbank_output_items tells what it yields)
 * and the call consumes all of it; max_out bounds the items written per row: LORA_HIP_ERR_OVERFLOW, with *n_out set and
 * nothing run, when n_in would yield more.  Argument checks (LORA_HIP_ERR_ARG: a NULL or misaligned pointer, n_dst out of
 * range) come before any device call.  The history update stays on the device for any n_in.  Synchronous on return. */
lora_hip_status lora_hip_filterbank_run_device_rows(lora_hip_filterbank_t *h, const void *d_in, size_t n_in, void *const *row_ptrs,
                                                    uint32_t n_dst, size_t max_out, size_t *n_out, void *hip_stream);

/* lora_hip_filterbank_run_device_rows for n_in items of format fmt (as lora_hip_filterbank_run_device_raw). */
lora_hip_status lora_hip_filterbank_run_device_rows_raw(lora_hip_filterbank_t *h, const void *d_in, size_t n_in, int fmt, float scale,
                                                        void *const *row_ptrs, uint32_t n_dst, size_t max_out, size_t *n_out,
                                                        void *hip_stream);

/* Same with host buffers: in = n_in cf32, out = n_channels rows of out_stride cf32. */
lora_hip_status lora_hip_filterbank_work(lora_hip_filterbank_t *h, const float *in, size_t n_in, float *out,
                                         size_t out_stride, size_t *n_out);

/* Same with n_in host items of format fmt: the raw bytes are uploaded (2-4 times fewer than cf32) and converted by the kernel. */
lora_hip_status lora_hip_filterbank_work_raw(lora_hip_filterbank_t *h, const void *in, size_t n_in, int fmt, float scale, float *out,
                                             size_t out_stride, size_t *n_out);

/* The tile shape the handle planned from (n_grid, decimation, tap count), read-only: a workgroup takes nc chunks of cw (<= 64)
 * output times, g chunks at a time, with q taps per polyphase branch (the tap count rounded up to q * n_grid), in lds_bytes of
 * LDS.  Any of the output pointers may be NULL.  For tests and measurements: it says which path of the kernel a case runs. */
lora_hip_status lora_hip_filterbank_get_plan(const lora_hip_filterbank_t *h, uint32_t *cw, uint32_t *g, uint32_t *nc, uint32_t *q,
                                             size_t *lds_bytes);

/* Kernel time of the last run (HIP events on the launch stream), for the measurements in DESIGN.md. */
float           lora_hip_filterbank_last_kernel_ms(const lora_hip_filterbank_t *h);

#ifdef __cplusplus
}
#endif
#endif /* LORA_HIP_FILTERBANK_H */
