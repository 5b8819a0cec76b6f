/*
 * lora_hip_soft.h -- C ABI of the soft-decision decoder for the low-SNR receive path (gr_lora_amd/csrc/lora_soft.inc.hip).
 *
 * lora_hip_decode_at_headers_device (lora_hip.h) decides every symbol by its arg-max bin; the block de-interleaver then spreads each
 * codeword over 4 + CR symbols and Hamming(8,4) corrects one bit at 4/8 and nothing at 4/5 and 4/6.  The calls here keep, per bit of
 * a symbol's word, a log-likelihood ratio taken from the whole dechirped spectrum and decide each codeword by correlation with the
 * 16 codewords of the code, at every CR: about 2 dB of decoding sensitivity, and error correction at 4/5 and 4/6.
 *
 * DEFINITION (float64 restatement: gr_lora_amd/softdecode.py).  sps = samples per symbol, N = 2^sf.
 *   symbol metric   m[k] = |X[k]|, X the N bins k in [-N/2, N/2) stored at index k mod N of the sps-point DFT of x * d_downchirp (the bins
 *                   of lora_hip_window_stats_device, no N/2 fold; d_downchirp: table 0 of lora_hip_get_table)
 *   bin, word       b(k) = (k - 1) mod N (LORA_HIP_DEMOD_FFT's bin).  Full rate: w = b ^ (b >> 1), ppm = sf bits.  Reduced rate:
 *                   b' = ((b + 2) / 4) mod (N / 4), w = b' ^ (b' >> 1), ppm = sf - 2 bits.  The eight header symbols are always reduced
 *   bit LLR         L[i] = max{m[k]: bit i of w(k) = 0} - max{m[k]: bit i of w(k) = 1}, i < ppm; positive: the bit is 0
 *   codeword LLRs   a block of n_w words (8: header, 4 + cr: payload) yields ppm codewords x: C_x[i] = L_i[(x - i) mod ppm], i < n_w
 *   de-shuffle      D_x[j] = C_x[S[j]] if S[j] < n_w else 0 (an erasure), S = {5,0,1,2,4,3,6,7}
 *   de-whitening    D_x[j] negated where bit j of the codeword's whitening byte is 1 (the tables of the integer chain, same indices)
 *   decision        score[s] = sum over j ascending of (bit j of ENC[s] ? -D[j] : D[j]) in fp32; the nibble is the smallest s whose score
 *                   is largest; margin = best - second best
 *   frame           header bytes from nibbles 0..4 (a cr field above 4 reads as 4, one of 0 gives no frame), payload_length = length +
 *                   2 has_crc, symbol count as decoder_impl.cc:842-847, bytes low nibble first over the spare header codewords and the
 *                   payload codewords; symbol k is the window at header_pos + k sps (no fine_sync)
 * Link metrics (lora_hip_link.h) are NOT measured for the frames published here, whatever lora_hip_link_enable says.
 * Plain C types only; device pointers and the HIP stream travel as void*.  Every argument check comes before any device call.
 */
#ifndef LORA_HIP_SOFT_H
#define LORA_HIP_SOFT_H

#include <stddef.h>
#include <stdint.h>

#include "lora_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LORA_HIP_SOFT_REQUIRE_HEADER_CHECKSUM 1u /* a header whose 5-bit checksum fails is not demodulated further (a false alarm would cost up to 257 bytes of noise) */

#define LORA_HIP_SOFT_FRAME 0u            /* a frame was published */
#define LORA_HIP_SOFT_HEADER_REJECTED 1u  /* LORA_HIP_SOFT_REQUIRE_HEADER_CHECKSUM and the checksum failed; no frame */
#define LORA_HIP_SOFT_CR_ZERO 2u          /* the header's cr field is 0; no frame */
#define LORA_HIP_SOFT_TRUNCATED 3u        /* header or payload runs past its stream (every symbol needs 2 sps items from its position, as in the hard path); no frame */

typedef struct lora_hip_soft_report {
    uint32_t status;              /* LORA_HIP_SOFT_FRAME ... */
    uint32_t cr;                  /* of the decoded header (after the rewrite of values above 4)                         */
    uint32_t payload_length;      /* length + 2 has_crc                                                                  */
    uint32_t payload_symbols;     /* 0 where no payload was demodulated                                                  */
    uint8_t  header_checksum_ok;  /* the header's 5-bit checksum (lora_hip_check_frame's rule)                           */
    uint8_t  has_crc;
    uint8_t  crc_ok;              /* lora_hip_check_frame's rule; 0 where no frame was published                         */
    uint8_t  reserved;
    uint32_t codewords;           /* codewords decided: 5 header + (sf - 7) spare + payload                              */
    uint32_t changed;             /* ... of them those whose nibble differs from the hard chain's on the same LLR signs   */
    float    min_margin;          /* smallest margin of a decided codeword (fp32, the device's own)                      */
    float    mean_abs_llr;        /* mean |L| over the windows demodulated; 0 where no frame was published               */
} lora_hip_soft_report_t;

/* Test and diagnostics entry: the bit LLRs of n windows of samples_per_symbol items at offsets[i] (host array, item indices into d_iq).
 * reduced[i] != 0: the reduced-rate word table (ppm = sf - 2), else the full one (ppm = sf); reduced == NULL: the handle's
 * reduced_rate for every window.  llr_out: the ppm floats of every window back to back (n * ppm where all windows are alike);
 * k_out / peak_out (optional): arg-max index k (first maximum) and its magnitude.  Host arrays.                                    */
lora_hip_status lora_hip_soft_symbols_device(lora_hip_decoder_t *h, const void *d_iq, size_t total_items, const int64_t *offsets, size_t n,
                                             const uint8_t *reduced, float *llr_out, int32_t *k_out, float *peak_out, void *hip_stream);

/* lora_hip_decode_at_headers_device with soft decisions: same arguments, same checks and errors (a pass is open: ERR_ARG; implicit header:
 * ERR_BAD_CONFIG; bad stream or header position: ERR_ARG).  SF 7..12 only: a handle at SF6, whose header block holds 4 codewords and not the 5 of
 * an explicit header, gets ERR_BAD_CONFIG before any device call.  Four launches: the LLRs of the 8 header windows of all n entries, their five
 * header codewords (the host reads n headers), the LLRs of all payload windows of all frames, the chain of all frames.  LLRs stay on the
 * device.  Frames go to the handle's queue in the order of pre, built like the hard path's: loratap bytes with SNR byte 0, info.stream,
 * info.header_pos, info.end_pos = header_pos + (8 + payload symbols taken) sps.  reports (optional): n records.                        */
lora_hip_status lora_hip_soft_decode_at_headers_device(lora_hip_decoder_t *h, const void *d_iq, size_t total_items, const uint64_t *stream_off,
                                                       const uint64_t *stream_len, uint32_t n_streams, const lora_hip_preamble_t *pre, size_t n,
                                                       uint32_t flags, lora_hip_soft_report_t *reports, void *hip_stream);

/* ---- CRC-aided repair (off by default; definition: gr_lora_amd/softdecode.py crc_repair) ----
 * Where a frame is published with a payload CRC that fails, the L least reliable codewords of its body may take their second-best nibble
 * (the smallest s != nibble with the largest score among the rest: what margin is measured against).
 *   eligible    the codewords that feed the frame body - spare header codewords first, then payload codewords - at indices
 *               c < 2 * payload_length.  The five header codewords are never touched
 *   candidates  the n_cand = min(L, eligible) of them with the smallest (margin, c), margins compared as values; candidate 0 is the least reliable
 *   syndrome    lora_hip_check_frame's crc_calc ^ crc_rx of the body; affine over GF(2) in the body bits, so candidate i taking its second
 *               nibble changes it by a fixed 16-bit e[i]
 *   pattern p   1 .. 2^n_cand - 1 matches iff the XOR of e[i] over its set bits equals the syndrome; penalty = the sum of margin[i] over the
 *               set bits, i ascending, fp32.  The matching pattern with the smallest (penalty, p) is applied to the published bytes
 * The 16-bit CRC also accepts wrong patterns: more than 2^L / 65536 of the time, because its last two payload bytes and the CRC bytes enter
 * by plain XOR and one wrong symbol puts the same bit error into several codewords of a block.  DESIGN.md 4.19.1 has the measured rate.     */
#define LORA_HIP_SOFT_REPAIR_NOT_ATTEMPTED 0u /* no frame published, or the frame has no CRC, or repair is off */
#define LORA_HIP_SOFT_REPAIR_CRC_HELD 1u      /* the CRC held: nothing to do, no other field is filled in      */
#define LORA_HIP_SOFT_REPAIR_REPAIRED 2u      /* a pattern matched and was applied                             */
#define LORA_HIP_SOFT_REPAIR_FAILED 3u        /* no pattern matched: every byte is as the decoder left it      */
#define LORA_HIP_SOFT_REPAIR_MAX_CANDIDATES 8u

typedef struct lora_hip_soft_repair {
    uint32_t status;      /* LORA_HIP_SOFT_REPAIR_NOT_ATTEMPTED ...                                   */
    uint32_t candidates;  /* n_cand                                                                   */
    uint32_t pattern;     /* bit i: candidate i took its second nibble; 0 unless REPAIRED             */
    uint32_t changed;     /* set bits of pattern                                                      */
    uint16_t syndrome;    /* the value before repair                                                  */
    uint16_t reserved;
    float    penalty;     /* of the pattern applied (fp32, the device's own); 0 unless REPAIRED       */
    uint16_t codeword[8]; /* the body codeword index c of each candidate, 0 past n_cand               */
} lora_hip_soft_repair_t;

/* candidates: 0 turns repair off (the default), 1 .. 8 turns it on with that L for later lora_hip_soft_decode_at_headers_device calls on this
 * handle; anything else: ERR_ARG.  With repair on that call queues one more launch behind the chain's; the published frame carries the
 * repaired bytes, reports[i].crc_ok is that of the published frame, and every other report field is the decision before repair.           */
lora_hip_status lora_hip_soft_crc_repair_enable(lora_hip_decoder_t *h, uint32_t candidates);

/* The records of the last lora_hip_soft_decode_at_headers_device call on this handle, one per entry of pre: n must be that call's n (ERR_ARG
 * otherwise; before any such call: 0).  With repair off every record is NOT_ATTEMPTED.                                                     */
lora_hip_status lora_hip_soft_crc_repair_results(lora_hip_decoder_t *h, lora_hip_soft_repair_t *out, size_t n);

/* Test and diagnostics entry: the repair kernel alone on n_frames frame bodies given as codewords.  length[f] <= 255: payload bytes in front
 * of the two CRC bytes; nibble / second (values below 16) / margin: the 2 * (length[f] + 2) body codewords of every frame, back to back;
 * candidates 1 .. 8.  bytes_out: the length[f] + 2 body bytes of every frame after repair, back to back; records_out: n_frames records.
 * Host arrays.                                                                                                                              */
lora_hip_status lora_hip_soft_crc_repair_codewords(lora_hip_decoder_t *h, size_t n_frames, const uint32_t *length, const uint8_t *nibble,
                                                   const uint8_t *second, const float *margin, uint32_t candidates, uint8_t *bytes_out,
                                                   lora_hip_soft_repair_t *records_out, void *hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* LORA_HIP_SOFT_H */
