/*
 * lora_hip_tx.h -- C ABI of the transmit side: the LoRa frame encoder (host only) and a wide-band traffic synthesiser that
 * writes a capture of many concurrent emitters into device memory, where lora_hip_gateway_work_device and the other device
 * entry points read it.
 *
 * The capture on absolute sample indices m is, in the order the frames were added,
 *     y[m] = sum_e  a_e * c_e[m - start_e] * exp(2j*pi * frac(f_e / fs * m))      for start_e <= m < start_e + items_e
 * where c_e is the frame's unit-amplitude waveform at the capture's rate fs (preamble upchirps, two sync symbols, 2.25
 * downchirps, 8 header symbols, payload symbols): gr_lora_amd/synth.py build_wideband is the float64 statement of it and
 * tests/test_gpu_tx.py holds the device to it.  A sample no emitter covers is +0.0, +0.0 unless noise is on.
 * Plain C types only; device pointers and the HIP stream travel as void*.  Same conventions as lora_hip.h.
 */
#ifndef LORA_HIP_TX_H
#define LORA_HIP_TX_H

#include <stddef.h>
#include <stdint.h>

#include "lora_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LORA_HIP_TX_MAX_DECIMATION 1024u        /* samp_rate / bandwidth, an integer (any, not only powers of two)   */
#define LORA_HIP_TX_MAX_SYMBOL_ITEMS 4194304u   /* samp_rate / bandwidth * 2^sf at most (2^22)                        */
#define LORA_HIP_TX_MAX_PREAMBLE 1024u
#define LORA_HIP_TX_MAX_SHIFTS 2048u            /* header + payload symbols of the longest frame fit (SF6 reduced rate, CR4, 257 bytes: 1040) */

#define LORA_HIP_TX_FRAME_HDR_NIBBLES 1u        /* flags: hdr_nibbles replaces the valid header checksum             */
#define LORA_HIP_TX_FRAME_CRC_BYTES 2u          /* flags: crc_bytes replaces the valid payload CRC                   */

/* One emitter: one frame at one place in time and frequency. */
typedef struct lora_hip_tx_frame {
    uint32_t       struct_size;     /* sizeof(lora_hip_tx_frame_t)                                                    */
    uint32_t       bandwidth;       /* Hz; the stream's samp_rate must be an integer multiple of it                   */
    uint8_t        sf;              /* 6 .. 12; 6 with implicit only (the header block holds 5 codewords)             */
    uint8_t        implicit;
    uint8_t        cr;              /* 1 .. 4                                                                         */
    uint8_t        crc;             /* two CRC bytes follow the payload                                               */
    uint8_t        reduced_rate;
    uint8_t        reserved0[3];
    uint32_t       preamble_len;    /* upchirps in front of the sync symbols; 0 = 8                                   */
    int32_t        sync_shifts[2];  /* negative = the default 3N/16 and N/4 (N = 2^sf); taken mod N                   */
    uint32_t       flags;           /* LORA_HIP_TX_FRAME_*                                                            */
    uint8_t        hdr_nibbles[2];  /* with FRAME_HDR_NIBBLES: low nibble of PHY byte 1, high nibble of PHY byte 2    */
    uint8_t        crc_bytes[2];    /* with FRAME_CRC_BYTES: the two bytes behind the payload, as the decoder shows them */
    int64_t        start;           /* absolute index of the frame's first sample                                     */
    double         freq_hz;         /* centre of the frame, Hz from the capture's centre                              */
    float          amplitude;
    uint32_t       length;          /* payload bytes, 0 .. 255                                                        */
    const uint8_t *payload;
} lora_hip_tx_frame_t;

typedef struct lora_hip_tx_config {
    uint32_t struct_size;
    int32_t  device;
    double   samp_rate;             /* of the capture, Hz                                                             */
    double   noise_sigma;           /* 0 = none; else complex white Gaussian noise of this sigma per complex sample   */
    uint64_t seed;                  /* of the noise: a sample's noise is a function of (seed, absolute index) alone   */
    uint32_t flags;                 /* reserved, 0                                                                    */
    uint32_t reserved;
} lora_hip_tx_config_t;

typedef struct lora_hip_tx lora_hip_tx_t;

/* ---- host only: no device is needed ------------------------------------------------------------------------------------- */

/* The frame's symbols as cyclic advances in bins: shifts[0 .. 8) the header block, shifts[8 .. 8 + *n_pay) the payload blocks;
 * *n_hdr is 8.  shifts may be NULL to ask for the counts only.  Whitening, Hamming code, shuffle, interleaver, inverse gray
 * code and the bin convention are the inverse of the decoder's chain (gr_lora_amd/synth.py encode_shifts); by default the
 * header checksum and the payload CRC are the valid ones (lora_hip_check_frame accepts the decoded frame).  start, freq_hz,
 * amplitude, preamble_len and sync_shifts play no part here.
 * LORA_HIP_ERR_ARG: f / n_hdr / n_pay NULL, struct_size too small, payload NULL with length > 0; LORA_HIP_ERR_BAD_SF: sf outside
 * 6..12; LORA_HIP_ERR_BAD_CONFIG: cr outside 1..4, length > 255, sf 6 without implicit, unknown flags, a nibble above 15;
 * LORA_HIP_ERR_OVERFLOW: cap < 8 + *n_pay (the counts are still set). */
lora_hip_status lora_hip_tx_encode(const lora_hip_tx_frame_t *f, uint16_t *shifts, size_t cap, uint32_t *n_hdr, uint32_t *n_pay);

/* Items of the frame's waveform at samp_rate.  As lora_hip_tx_encode, and LORA_HIP_ERR_BAD_CONFIG when samp_rate / bandwidth is
 * no integer in 1 .. LORA_HIP_TX_MAX_DECIMATION, when that times 2^sf exceeds LORA_HIP_TX_MAX_SYMBOL_ITEMS, or when preamble_len
 * exceeds LORA_HIP_TX_MAX_PREAMBLE. */
lora_hip_status lora_hip_tx_frame_items(const lora_hip_tx_frame_t *f, float samp_rate, uint64_t *items);

/* ---- the stream ---------------------------------------------------------------------------------------------------------- */

/* LORA_HIP_ERR_ARG: cfg / out NULL, struct_size too small, device < 0; LORA_HIP_ERR_BAD_CONFIG: samp_rate or noise_sigma not
 * finite, samp_rate <= 0, noise_sigma < 0, flags != 0.  All before any device call; then LORA_HIP_ERR_NO_DEVICE without a
 * device.  There is no CPU path.  The stream starts at position 0. */
lora_hip_status lora_hip_tx_create(const lora_hip_tx_config_t *cfg, lora_hip_tx_t **out);
void            lora_hip_tx_destroy(lora_hip_tx_t *h);
const char     *lora_hip_tx_last_error(const lora_hip_tx_t *h);

/* Adds n frames (each struct_size == sizeof(lora_hip_tx_frame_t)); their order, after the frames added before, is the order of
 * the sum.  Encoded on the host, symbols uploaded.  The checks of lora_hip_tx_frame_items at the stream's rate, and
 * LORA_HIP_ERR_ARG for an amplitude or freq_hz that is not finite and for a start before lora_hip_tx_position.  When any frame
 * of the call is refused none of them is added and the stream is as before. */
lora_hip_status lora_hip_tx_add_frames(lora_hip_tx_t *h, const lora_hip_tx_frame_t *frames, size_t n);

/* The next n items as cf32 at d_out (8-byte aligned), in one kernel launch on hip_stream; the position advances by n and frames
 * that lie wholly behind it are retired.  The call returns when the items are written.  Any split of a capture into calls gives
 * the same bits. */
lora_hip_status lora_hip_tx_generate_device(lora_hip_tx_t *h, void *d_out, size_t n, void *hip_stream);

/* The same items as integers of format fmt (lora_hip_iq_format; d_out aligned to the item), packed by the same kernel: per
 * component rint(double(x) * full_scale), + 127.5 first for cu8, ties to even, clipped to the type - bit for bit
 * gr_lora_amd.iqformat.quantize of the cf32 items.  full_scale must be finite and positive.  fmt LORA_HIP_IQ_CF32 ignores it. */
lora_hip_status lora_hip_tx_generate_device_raw(lora_hip_tx_t *h, void *d_out, size_t n, int fmt, double full_scale, void *hip_stream);

/* The next n cf32 items into host memory (staged through a device buffer of the handle). */
lora_hip_status lora_hip_tx_generate(lora_hip_tx_t *h, float *out, size_t n);

int64_t lora_hip_tx_position(const lora_hip_tx_t *h);        /* absolute index of the next item                        */
size_t  lora_hip_tx_pending(const lora_hip_tx_t *h);         /* frames added and not yet emitted to their last sample  */
float   lora_hip_tx_last_kernel_ms(const lora_hip_tx_t *h);  /* the last generate call's kernel (HIP events)           */

#ifdef __cplusplus
}
#endif
#endif /* LORA_HIP_TX_H */
