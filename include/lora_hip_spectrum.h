/*
 * lora_hip_spectrum.h -- C ABI of the MI355X spectral scan: Welch power-spectrum rows and channel band powers of a wide-band
 * capture, computed on the device from the same buffer the channeliser and the filter bank are fed.  A handle of its own; it
 * changes nothing the other handles do.  Float64 model of the same definition: gr_lora_amd/spectrum.py (welch_rows).
 *
 * DEFINITION.  The stream is x[n], n = 0, 1, ...: cf32, or sc16 / sc8 / cu8 converted by lora_hip_iq_format's table (lora_hip.h).
 *   window   w[k] = fl32(0.5 - 0.5 cos(2 pi k / nfft)) (periodic Hann, formed in double, rounded once) or all ones (RECT);
 *            norm = 1 / (nfft * sum_k w[k]^2), the sum of the fp32 values taken in double
 *   segment  s covers x[s hop .. s hop + nfft - 1];   P_s[k] = | sum_n w[n] x[s hop + n] e^{-2 pi j k n / nfft} |^2
 *   row      r covers segments r n_avg .. (r + 1) n_avg - 1:
 *                psd[r][i]  = norm / n_avg * sum_s P_s[k]
 *                peak[r][i] = norm * max_s P_s[k]                          (LORA_HIP_SPECTRUM_FLAG_PEAK)
 *            stored centred, i = (k + nfft / 2) mod nfft: index i is frequency (i - nfft / 2) samp_rate / nfft, index nfft / 2 is
 *            DC.  Units: full-scale^2 per bin; by Parseval a row sums to the windowed mean power of its samples.
 *   band     b = (first_bin, n_bins) in centred indices, inside [0, nfft):  band[r][b] = sum of psd[r][i] over the band
 *   position row r starts at absolute sample r n_avg hop and spans (n_avg - 1) hop + nfft samples.
 *
 * STREAMING.  A call consumes all n_in items and emits every row whose last sample has arrived.  The samples of the segment in
 * progress (cf32, at most nfft - 1 items) and the partial sums of the row in progress stay on the device between calls: a call
 * too short to complete a segment emits nothing and loses nothing.  A trailing partial row is never emitted; reset drops it.
 *
 * SUMMATION ORDER (every "bit for bit" below follows from it).  A segment's transform is a fixed decimation-in-frequency
 * radix-4 network over nfft points (one last radix-2 stage where log2 nfft is odd) with twiddles from a table built in double;
 * its operation order depends on nfft and the bin only.  P = fl(fl(re re) + fl(im im)), no fused multiply-add.  A bin's row sum
 * is ONE sequential fp32 sum over the row's segments in ascending absolute segment index, starting from +0:
 * acc = fl(acc + P_s); the maximum likewise.  A row in progress at the end of a call leaves acc in the handle and the next call
 * continues the same sequence.  No float atomics; nothing depends on chunk boundaries, grid size or scheduling.  psd = fl(acc *
 * fl(norm / n_avg)), peak = fl(max * fl(norm)).  A band is summed by 64 partial sums (partial l takes bins first + l, first + l
 * + 64, ... in ascending order) combined by a fixed halving tree (l with l + 32, then + 16, ... + 1).
 *
 * Plain C types only; device pointers and the HIP stream travel as void*.  Same conventions as lora_hip_filterbank.h: every
 * argument check comes before any device call.
 */
#ifndef LORA_HIP_SPECTRUM_H
#define LORA_HIP_SPECTRUM_H

#include <stddef.h>
#include <stdint.h>

#include "lora_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Limits (LORA_HIP_ERR_BAD_CONFIG outside them, before any device call). */
#define LORA_HIP_SPECTRUM_MIN_NFFT 64u     /* nfft: a power of two, 64 .. 4096 */
#define LORA_HIP_SPECTRUM_MAX_NFFT 4096u
#define LORA_HIP_SPECTRUM_MAX_AVG 1024u    /* 1 <= n_avg <= 1024 segments per row; 1 <= hop <= nfft */
#define LORA_HIP_SPECTRUM_MAX_BANDS 256u   /* 0 <= n_bands <= 256 */

#define LORA_HIP_SPECTRUM_WINDOW_HANN 0u
#define LORA_HIP_SPECTRUM_WINDOW_RECT 1u

#define LORA_HIP_SPECTRUM_FLAG_PEAK 1u     /* also keep the per-bin maximum over a row's segments (max hold) */

typedef struct lora_hip_spectrum_config {
    uint32_t        struct_size;
    double          samp_rate;   /* fs of the capture (Hz), > 0: only names the frequency axis */
    uint32_t        nfft;
    uint32_t        hop;         /* segment s starts at sample s * hop */
    uint32_t        n_avg;       /* segments per row */
    uint32_t        window;      /* LORA_HIP_SPECTRUM_WINDOW_* */
    uint32_t        flags;       /* LORA_HIP_SPECTRUM_FLAG_* */
    const uint32_t *bands;       /* n_bands pairs (first_bin, n_bins) in centred indices (may be NULL when n_bands is 0) */
    uint32_t        n_bands;
    int32_t         device;      /* HIP device ordinal */
} lora_hip_spectrum_config_t;

typedef struct lora_hip_spectrum lora_hip_spectrum_t;

/* LORA_HIP_ERR_ARG: cfg or out NULL, struct_size too small, bands NULL with n_bands > 0; LORA_HIP_ERR_BAD_CONFIG: a limit above,
 * nfft no power of two, a band empty or outside [0, nfft), an unknown window or flag bit, samp_rate <= 0;
 * LORA_HIP_ERR_NO_DEVICE: no such HIP device (no CPU fallback). */
lora_hip_status lora_hip_spectrum_create(const lora_hip_spectrum_config_t *cfg, lora_hip_spectrum_t **out);
void            lora_hip_spectrum_destroy(lora_hip_spectrum_t *h);
const char     *lora_hip_spectrum_last_error(const lora_hip_spectrum_t *h);

/* The window table (nfft fp32 values): *n receives nfft; w may be NULL to query it. */
lora_hip_status lora_hip_spectrum_window(const lora_hip_spectrum_t *h, float *w, size_t cap, size_t *n);

/* Rows the next call will emit for n_in input items (depends on the samples and segments carried over). */
size_t          lora_hip_spectrum_output_rows(const lora_hip_spectrum_t *h, size_t n_in);

/* Streaming, device-resident: d_in = n_in cf32 items continuing the stream.  *n_rows rows are written: row j of d_psd (and of
 * d_peak) starts at float index j * row_stride (row_stride >= nfft) and holds nfft floats, row j of d_band holds n_bands floats
 * at j * n_bands; *first_row is the absolute index of row 0 of this call.  d_peak must be NULL unless the handle has
 * LORA_HIP_SPECTRUM_FLAG_PEAK; d_band is NULL iff n_bands == 0 (LORA_HIP_ERR_ARG otherwise).  LORA_HIP_ERR_OVERFLOW, with
 * *n_rows set and nothing run (the stream is where it was), when n_in would yield more than max_rows.  One pass over the
 * input; synchronous on return. */
lora_hip_status lora_hip_spectrum_run_device(lora_hip_spectrum_t *h, const void *d_in, size_t n_in, float *d_psd, float *d_peak,
                                             float *d_band, size_t row_stride, size_t max_rows, size_t *n_rows, uint64_t *first_row,
                                             void *hip_stream);

/* The same for n_in items of format fmt (lora_hip_iq_format, lora_hip.h: the conversion, scale and the checks made before any
 * device call): the kernel converts each item as it stages it, the carried samples stay cf32.  Bit for bit the rows of
 * lora_hip_spectrum_run_device fed the converted items; the format may change from call to call. */
lora_hip_status lora_hip_spectrum_run_device_raw(lora_hip_spectrum_t *h, const void *d_in, size_t n_in, int fmt, float scale,
                                                 float *d_psd, float *d_peak, float *d_band, size_t row_stride, size_t max_rows,
                                                 size_t *n_rows, uint64_t *first_row, void *hip_stream);

/* Same with host buffers: in = n_in cf32 items, psd / peak / band host arrays laid out as above. */
lora_hip_status lora_hip_spectrum_work(lora_hip_spectrum_t *h, const float *in, size_t n_in, float *psd, float *peak, float *band,
                                       size_t row_stride, size_t max_rows, size_t *n_rows, uint64_t *first_row);

/* Same with n_in host items of format fmt: the raw bytes are uploaded and converted by the kernel. */
lora_hip_status lora_hip_spectrum_work_raw(lora_hip_spectrum_t *h, const void *in, size_t n_in, int fmt, float scale, float *psd,
                                           float *peak, float *band, size_t row_stride, size_t max_rows, size_t *n_rows,
                                           uint64_t *first_row);

/* Drops the carried samples and the row in progress; the next item is sample 0 of a new stream. */
lora_hip_status lora_hip_spectrum_reset(lora_hip_spectrum_t *h);

/* Kernel time of the last run (HIP events on the launch stream: the scan and, with bands, the band sums). */
float           lora_hip_spectrum_last_kernel_ms(const lora_hip_spectrum_t *h);

#ifdef __cplusplus
}
#endif
#endif /* LORA_HIP_SPECTRUM_H */
