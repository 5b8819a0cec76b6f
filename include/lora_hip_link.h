/*
 * lora_hip_link.h -- C ABI of the per-frame link metrics: signal power, noise power, RSSI, SNR, carrier frequency offset,
 * timing offset and the sync word of every published frame, measured on the device (gr_lora_amd/csrc/lora_link.hip).
 *
 * DEFINITION (float64 restatement: gr_lora_amd/linkmetrics.py).  Positions are relative to a frame's
 * header_pos (first header symbol); sps = samples per symbol, N = 2^sf, D = sps / N.  Six windows of sps items:
 *     window 0, 1 (preamble):  header_pos - (25 sps) / 4 + k sps     the last two unmodulated upchirps
 *     window 2, 3 (sync):      header_pos - (17 sps) / 4 + k sps     the two sync-word symbols
 *     window 4, 5 (SFD):       header_pos -  (9 sps) / 4 + k sps     the two whole downchirps
 * (integer division).  A window is valid iff it lies whole inside its stream; an invalid window is never read.  A window's
 * spectrum X[k], k in [-N/2, N/2) stored at index k mod N, is the pruned sps-point DFT (the N bins of
 * lora_hip_window_stats_device, no N/2 fold) of
 *     m[n] = v[n] * down[n] * w[n],     w[n] = 0.5 - 0.5 cos(2 pi (n + 0.5) / sps)      (Hann)
 * with down = the decoder's d_downchirp (table 0 of lora_hip_get_table; it carries the reference's factor 1 + 1j, |down|^2 = 2),
 * v = x for preamble and sync windows and conj(x) for SFD windows.  lora_hip_link_window_t is what the device forms from it;
 * lora_hip_link_combine is the per-frame combination, in double on the host.
 * Plain C types only; device pointers and the HIP stream travel as void*.  Same conventions as lora_hip.h: every argument
 * check comes before any device call.
 */
#ifndef LORA_HIP_LINK_H
#define LORA_HIP_LINK_H

#include <stddef.h>
#include <stdint.h>

#include "lora_hip.h"
#include "lora_hip_gateway.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LORA_HIP_LINK_WINDOWS 6u
#define LORA_HIP_LINK_LOBE 3          /* the lobe is peak_bin - 3 .. peak_bin + 3, indices mod N (the Hann main lobe and one bin either side) */
#define LORA_HIP_LINK_FLAG_PREAMBLE 1u /* both preamble windows were valid */
#define LORA_HIP_LINK_FLAG_SYNC 2u     /* both sync windows */
#define LORA_HIP_LINK_FLAG_SFD 4u      /* both SFD windows */
#define LORA_HIP_LINK_FLOOR_DB (-200.0) /* rssi_dbfs / snr_db of a zero power */

/* One window, written by one workgroup (24 bytes). */
typedef struct lora_hip_link_window {
    int32_t  peak_bin;     /* index (k mod N) of the first maximum of |X|^2                                          */
    float    frac;         /* a = |X[peak-1]|, b = |X[peak+1]|, alpha = max(a, b) / |X[peak]|, d = (2 alpha - 1) / (alpha + 1): +d if b >= a, else -d */
    float    lobe_power;   /* sum of |X|^2 over peak_bin - 3 .. peak_bin + 3 (mod N)                                 */
    float    total_power;  /* sum over all N bins                                                                    */
    float    peak_power;   /* |X[peak_bin]|^2                                                                        */
    uint32_t valid;        /* 0: the window lay outside its stream and was not read (every other field 0)            */
} lora_hip_link_window_t;

/* One frame (80 bytes).  With nb = (total - lobe) / (N - 7) the noise per bin and s = max(lobe - 7 nb, 0) of a window:
 * signal_power = mean of s / (0.75 sps^2), noise_power = mean of nb N / (0.75 sps^2) over the windows of the valid preamble and SFD
 * pairs, both in full-scale^2 inside the bandwidth (0.75 = 0.375, the Hann window's power gain, times |down|^2 = 2).  With
 * pos = peak_bin + frac wrapped into [-N/2, N/2), u and d the mean pos of the preamble and of the SFD windows:
 * cfo_bins = wrap((u - d) / 2), cfo_hz = cfo_bins bandwidth / N, timing_samples = wrap((u + d) / 2) D (positive: the windows
 * start late), sync_shift[k] = round(pos of sync window k - u) mod N.  A metric whose windows are missing is 0 (the levels:
 * LORA_HIP_LINK_FLOOR_DB) and its flag bit is clear. */
typedef struct lora_hip_link_metrics {
    uint32_t flags;            /* LORA_HIP_LINK_FLAG_*; 0: not measured (link metrics off)                           */
    uint32_t reserved0;
    double   signal_power, noise_power;
    double   rssi_dbfs, snr_db; /* 10 log10(signal_power), 10 log10(signal_power / noise_power), not below the floor */
    double   cfo_bins, cfo_hz, timing_samples;
    int32_t  sync_shift[2];
    uint64_t reserved;
} lora_hip_link_metrics_t;

typedef struct lora_hip_link_request {
    uint32_t stream;           /* index into the stream list                                                          */
    uint32_t reserved;
    int64_t  header_pos;       /* first header symbol, relative to the stream (any value: windows outside are invalid) */
} lora_hip_link_request_t;

/* Measures n frames at caller-given header positions in caller-resident cf32 IQ.  metrics_out[n]; windows_out, if not NULL,
 * gets the 6 n window records.  Synchronous on return.  LORA_HIP_ERR_ARG: h, d_iq, stream_off or stream_len NULL, n_streams 0,
 * n with req or metrics_out NULL, a stream outside the buffer, a request's stream >= n_streams. */
lora_hip_status lora_hip_link_measure_device(lora_hip_decoder_t *h, const void *d_iq, size_t total_items, const uint64_t *stream_off,
                                             const uint64_t *stream_len, uint32_t n_streams, const lora_hip_link_request_t *req, size_t n,
                                             lora_hip_link_metrics_t *metrics_out, lora_hip_link_window_t *windows_out, void *hip_stream);

/* The combination above: host only, no handle.  LORA_HIP_ERR_ARG: a NULL pointer, sps or nbins no power of two, nbins < 16 or > sps. */
lora_hip_status lora_hip_link_combine(const lora_hip_link_window_t *windows /* [6] */, uint32_t sps, uint32_t nbins, double bandwidth,
                                      lora_hip_link_metrics_t *out);

/* Turns the measurement on (on != 0) or off for a decoder handle: every frame published from then on is measured at the end
 * of the pass that decoded it (one launch per pass, on the pass's stream and IQ).  Off by default; when off nothing is built or
 * launched and the existing poll / drain entry points are unchanged (when on they drop the metrics). */
lora_hip_status lora_hip_link_enable(lora_hip_decoder_t *h, int on);
/* lora_hip_poll_frame / lora_hip_drain_frames with the metrics (flags == 0 for a frame published while link metrics were off). */
lora_hip_status lora_hip_link_poll_frame(lora_hip_decoder_t *h, uint8_t *buf, size_t cap, size_t *len, lora_hip_frame_info_t *info,
                                         lora_hip_link_metrics_t *metrics);
lora_hip_status lora_hip_link_drain_frames(lora_hip_decoder_t *h, uint8_t *buf, size_t cap, lora_hip_frame_info_t *infos,
                                           lora_hip_link_metrics_t *metrics, size_t max_frames, size_t *n_frames);
/* The same pair for a mux ... */
lora_hip_status lora_hip_link_mux_enable(lora_hip_mux_t *m, int on);
lora_hip_status lora_hip_link_mux_poll_frame(lora_hip_mux_t *m, uint8_t *buf, size_t cap, size_t *len, lora_hip_frame_info_t *info,
                                             lora_hip_link_metrics_t *metrics);
/* ... and for the gateway (every decoder's mux). */
lora_hip_status lora_hip_link_gateway_enable(lora_hip_gateway_t *g, int on);
lora_hip_status lora_hip_link_gateway_poll_frame(lora_hip_gateway_t *g, uint8_t *buf, size_t cap, size_t *len,
                                                 lora_hip_gateway_frame_info_t *info, lora_hip_link_metrics_t *metrics);
/* Counters since creation: window-kernel launches, frames measured, the kernel's time (HIP events), summed.  Any may be NULL. */
lora_hip_status lora_hip_link_stats(const lora_hip_decoder_t *h, uint64_t *launches, uint64_t *frames, double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* LORA_HIP_LINK_H */
