// lora_spectrum.hip -- MI355X spectral scan: Welch power-spectrum rows and band powers of a wide-band capture.  C ABI and the
// definition in include/lora_hip_spectrum.h; float64 model of the same definition in gr_lora_amd/spectrum.py (welch_rows).
//
// Kernel (spec_kernel), one launch per call.  The unit of work is a ROW (n_avg segments): a workgroup takes the segments of
// one row that this call completes, in ascending order, and keeps the row's per-bin sums in registers, so a spectrum never
// goes to HBM.  The work split follows nfft, not the chunk: nfft / 4 threads per segment - one wavefront at 64 .. 256, a
// workgroup of 2 .. 16 waves at 512 .. 4096.
//   * staging: the row's samples live in an LDS ring of nfft cf32 slots (slot = offset inside the row mod nfft).  The first
//     segment of the unit fills it; every later one loads only its hop new items, so with hop < nfft the overlap is read once
//     per workgroup.  An integer item is converted by the load (lora_iq::load<F>); items from before this call come from the
//     handle's carried samples (cf32).
//   * transform: decimation in frequency, radix 4, in place in a second LDS buffer (one last radix-2 stage where log2 nfft is
//     odd).  The first stage reads the ring and applies the window as the item enters; twiddles e^{-2 pi j t / nfft} come from a
//     table built in double on the host and copied into LDS once per workgroup.  The result is left in digit-reversed order;
//     nothing is reordered until a row is stored.
//   * accumulation: thread t owns positions t, t + T, ...: acc = acc + (re re + im im) per segment, and the maximum with
//     LORA_HIP_SPECTRUM_FLAG_PEAK.  This file is compiled without floating-point contraction, so each of these is one rounding,
//     the same in every instantiation.
//   * a completed row is scaled, put into centred order through LDS and stored coalesced; a row still in progress at the end of
//     the call stores acc (position order) to the handle's state, and the unit that continues it in the next call starts from
//     there - the same sequence of additions whatever the chunking.  State is double-buffered: the unit that reads it and the
//     unit that writes it may be different workgroups of one launch.
// Band sums are a second small launch over the stored rows (band_kernel).  Design and measurements: DESIGN.md 4.15.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lora_hip_spectrum.h"
#include "lora_iq.h"

#pragma STDC FP_CONTRACT OFF

namespace {

constexpr int kMaxPer = 4;               // positions a thread owns: nfft / threads (1 at 64, 2 at 128, 4 from 256 on)
constexpr unsigned kBandBlocksMax = 1u << 16;

struct SpArgs {
    const void *in;          // new input items of format F
    const float2 *hist;      // the n_hist items before in[0] (cf32)
    const float *state_in;   // partial sums of the row in progress: acc[nfft], then max[nfft] (position order)
    float *state_out;
    float *psd;              // rows of row_stride floats
    float *peak;             // or nullptr
    long long n_abs;         // absolute index of in[0]
    long long n_in;
    long long seg0, seg1;    // absolute segments [seg0, seg1) are completed by this call
    long long row0;          // seg0 / n_avg: the row of unit 0 (and output row 0 unless it is left in progress)
    long long row_stride;
    int n_hist;
    int nfft, hop, n_avg;
    float scale;             // integer formats: the conversion's scale (lora_iq.h)
    float k_psd, k_peak;     // fl(norm / n_avg), fl(norm)
};

__device__ __forceinline__ float2 sp_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 sp_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 sp_cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }

// position p of the finished in-place transform holds bin k: one base-4 digit per radix-4 stage, most significant first in p,
// least significant first in k; the radix-2 stage's bit last in p
__device__ __forceinline__ int sp_bin_of(int p, int nfft)
{
    int k = 0, mult = 1, L = nfft, rem = p;
    while (L >= 4) {
        const int q = L >> 2;
        const int d = rem / q;
        rem -= d * q;
        k += d * mult;
        mult <<= 2;
        L = q;
    }
    if (L == 2) k += rem * mult;
    return k;
}

template <int F>
__global__ __launch_bounds__(1024) void spec_kernel(SpArgs A, const float *__restrict__ win, const float2 *__restrict__ twg)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int N = A.nfft, mask = N - 1, T = (int)blockDim.x, t = (int)threadIdx.x;
    float2 *ring = reinterpret_cast<float2 *>(smem);   // ring[(offset inside the unit) & mask]
    float2 *X = ring + N;                               // the transform, in place
    float2 *tw = X + N;                                 // tw[i] = e^{-2 pi j i / N}
    const long long row = A.row0 + blockIdx.x;
    const long long row_s0 = row * A.n_avg;
    const long long sb = row_s0 > A.seg0 ? row_s0 : A.seg0;
    const long long se = row_s0 + A.n_avg < A.seg1 ? row_s0 + A.n_avg : A.seg1;
    const bool resume = sb > row_s0, done = se == row_s0 + A.n_avg;
    const bool want_peak = A.peak != nullptr;
    const int per = N / T;                              // <= kMaxPer

    float acc[kMaxPer], pk[kMaxPer];
#pragma unroll
    for (int i = 0; i < kMaxPer; i++) {
        acc[i] = 0.0f; pk[i] = 0.0f;
        if (resume && i < per) {
            acc[i] = A.state_in[t + i * T];
            pk[i] = A.state_in[N + t + i * T];
        }
    }
    for (int i = t; i < N; i += T) tw[i] = twg[i];

    for (long long s = sb; s < se; s++) {
        // ---- staging: the items of segment s that the ring does not hold yet
        const int off = (int)(s - sb) * A.hop;                         // offset of the segment inside the unit
        const long long loc0 = s * A.hop - A.n_abs;                    // index of the segment's first item relative to in[0]
        const int n_first = s == sb ? 0 : N - A.hop;
        for (int n = n_first + t; n < N; n += T) {
            const long long i = loc0 + n;
            float2 v = make_float2(0.f, 0.f);
            if (i >= 0) {
                if (i < A.n_in) v = lora_iq::load<F>(A.in, i, A.scale);
            } else if (i >= -(long long)A.n_hist) {
                v = A.hist[A.n_hist + i];
            }
            ring[(off + n) & mask] = v;
        }
        __syncthreads();
        // ---- transform: radix-4 stages, the first one from the ring through the window
        int L = N, step = 1;                                           // step = N / L
        bool first = true;
        while (L >= 4) {
            const int q = L >> 2;
            for (int bf = t; bf < (N >> 2); bf += T) {
                const int j = bf & (q - 1);
                const int base = (bf - j) * 4 + j;                     // block (bf / q) * L + j
                float2 a, b, c, d;
                if (first) {
                    const float wa = win[base], wb = win[base + q], wc = win[base + 2 * q], wd = win[base + 3 * q];
                    a = ring[(off + base) & mask]; b = ring[(off + base + q) & mask];
                    c = ring[(off + base + 2 * q) & mask]; d = ring[(off + base + 3 * q) & mask];
                    a.x *= wa; a.y *= wa; b.x *= wb; b.y *= wb; c.x *= wc; c.y *= wc; d.x *= wd; d.y *= wd;
                } else {
                    a = X[base]; b = X[base + q]; c = X[base + 2 * q]; d = X[base + 3 * q];
                }
                const float2 apc = sp_add(a, c), amc = sp_sub(a, c), bpd = sp_add(b, d), bmd = sp_sub(b, d);
                const float2 y0 = sp_add(apc, bpd);
                const float2 y1 = make_float2(amc.x + bmd.y, amc.y - bmd.x);   // (a - c) - j (b - d)
                const float2 y2 = sp_sub(apc, bpd);
                const float2 y3 = make_float2(amc.x - bmd.y, amc.y + bmd.x);   // (a - c) + j (b - d)
                const int ti = j * step;
                X[base] = y0;
                X[base + q] = sp_cmul(y1, tw[ti]);
                X[base + 2 * q] = sp_cmul(y2, tw[2 * ti]);
                X[base + 3 * q] = sp_cmul(y3, tw[3 * ti]);
            }
            __syncthreads();
            first = false;
            L = q;
            step <<= 2;
        }
        if (L == 2) {
            for (int bf = t; bf < (N >> 1); bf += T) {
                const float2 a = X[2 * bf], b = X[2 * bf + 1];
                X[2 * bf] = sp_add(a, b);
                X[2 * bf + 1] = sp_sub(a, b);
            }
            __syncthreads();
        }
        // ---- accumulation (the next write of X comes after the next segment's staging barrier)
#pragma unroll
        for (int i = 0; i < kMaxPer; i++) {
            if (i < per) {
                const float2 v = X[t + i * T];
                const float p = v.x * v.x + v.y * v.y;
                acc[i] = acc[i] + p;
                pk[i] = fmaxf(pk[i], p);
            }
        }
    }

    if (!done) {
#pragma unroll
        for (int i = 0; i < kMaxPer; i++) {
            if (i < per) {
                A.state_out[t + i * T] = acc[i];
                A.state_out[N + t + i * T] = pk[i];
            }
        }
        return;
    }
    // ---- a completed row: centred order through LDS (X as 2 N floats), then coalesced stores
    float *o = reinterpret_cast<float *>(X);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kMaxPer; i++) {
        if (i < per) {
            const int ci = (sp_bin_of(t + i * T, N) + (N >> 1)) & mask;
            o[ci] = acc[i] * A.k_psd;
            o[N + ci] = pk[i] * A.k_peak;
        }
    }
    __syncthreads();
    const long long orow = (row - A.row0) * A.row_stride;
    for (int i = t; i < N; i += T) {
        A.psd[orow + i] = o[i];
        if (want_peak) A.peak[orow + i] = o[N + i];
    }
}

// band[r][b] = sum of psd[r][first .. first + n - 1]: one wavefront per (row, band), 64 strided partial sums and a halving tree
__global__ __launch_bounds__(64) void band_kernel(const float *__restrict__ psd, long long row_stride, const uint32_t *__restrict__ bands,
                                                  int n_bands, long long n_rows, float *__restrict__ out)
{
    const int lane = (int)threadIdx.x;
    const long long total = n_rows * n_bands;
    for (long long job = blockIdx.x; job < total; job += gridDim.x) {
        const long long r = job / n_bands;
        const int b = (int)(job - r * n_bands);
        const int first = (int)bands[2 * b], n = (int)bands[2 * b + 1];
        const float *p = psd + r * row_stride + first;
        float v = 0.0f;
        for (int i = lane; i < n; i += 64) v = v + p[i];
        for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_down(v, d, 64);
        if (lane == 0) out[job] = v;
    }
}

} // namespace

struct lora_hip_spectrum {
    lora_hip_spectrum_config_t cfg{};
    std::vector<uint32_t> bands;   // pairs
    std::vector<float> window;
    int nfft = 0, hop = 0, n_avg = 0, threads = 0;
    bool peak = false;
    float k_psd = 0.0f, k_peak = 0.0f;
    size_t lds = 0;
    int device = 0;
    long long n_abs = 0;           // input items consumed so far
    int cur = 0;                   // which half of d_state holds the row in progress
    float *d_win = nullptr, *d_state = nullptr;     // d_state: 2 halves of 2 nfft floats
    float2 *d_tw = nullptr, *d_hist = nullptr, *d_hist2 = nullptr;
    uint32_t *d_bands = nullptr;
    void *d_stage_in = nullptr;
    float *d_stage_psd = nullptr, *d_stage_peak = nullptr, *d_stage_band = nullptr;
    size_t stage_in_cap = 0, stage_rows_cap = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_ms = 0.0f;
    std::string err;
};

namespace {

lora_hip_status sfail(lora_hip_spectrum *h, lora_hip_status s, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    return s;
}
#define SP_TRY(h, call)                                                                                    \
    do {                                                                                                   \
        hipError_t e_ = (call);                                                                            \
        if (e_ != hipSuccess) return sfail((h), LORA_HIP_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// segments whose last sample is among the first n items of the stream
long long sp_segments(const lora_hip_spectrum *h, long long n) { return n >= h->nfft ? (n - h->nfft) / h->hop + 1 : 0; }

// carried samples once n items have been consumed: from the first sample of the first incomplete segment on (< nfft)
long long sp_carried(const lora_hip_spectrum *h, long long n) { return n - sp_segments(h, n) * h->hop; }

template <int F>
hipError_t sp_launch_as(unsigned units, int threads, size_t lds, hipStream_t st, const SpArgs &a, const float *win, const float2 *tw)
{
    hipLaunchKernelGGL((spec_kernel<F>), dim3(units), dim3(threads), lds, st, a, win, tw);
    return hipGetLastError();
}

hipError_t sp_launch(int fmt, unsigned units, int threads, size_t lds, hipStream_t st, const SpArgs &a, const float *win, const float2 *tw)
{
    switch (fmt) {
    case LORA_HIP_IQ_SC16: return sp_launch_as<LORA_HIP_IQ_SC16>(units, threads, lds, st, a, win, tw);
    case LORA_HIP_IQ_SC8: return sp_launch_as<LORA_HIP_IQ_SC8>(units, threads, lds, st, a, win, tw);
    case LORA_HIP_IQ_CU8: return sp_launch_as<LORA_HIP_IQ_CU8>(units, threads, lds, st, a, win, tw);
    default: return sp_launch_as<LORA_HIP_IQ_CF32>(units, threads, lds, st, a, win, tw);
    }
}

template <int F>
bool sp_allow_lds(size_t lds)
{
    return hipFuncSetAttribute((const void *)spec_kernel<F>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
}

lora_hip_status sp_check_raw(lora_hip_spectrum *h, const void *p, int fmt, float scale)
{
    if (!h) return LORA_HIP_ERR_ARG;
    if (!lora_iq::args_ok(p, fmt, scale)) return sfail(h, LORA_HIP_ERR_ARG, "unknown format %d, unusable scale %g, or input not aligned to its component", fmt, (double)scale);
    return LORA_HIP_OK;
}

// what a call of n_in items emits, and the pointer rules of the header; no device call
lora_hip_status sp_check_run(lora_hip_spectrum *h, const void *in, size_t n_in, const float *psd, const float *peak, const float *band, size_t row_stride,
                             size_t max_rows, size_t *n_rows, uint64_t *first_row)
{
    if (!h || !n_rows || !first_row || (n_in && !in)) return LORA_HIP_ERR_ARG;
    if (n_in > (size_t)1 << 40) return sfail(h, LORA_HIP_ERR_ARG, "n_in %zu: at most 2^40 items per call", n_in);
    if (peak && !h->peak) return sfail(h, LORA_HIP_ERR_ARG, "a peak buffer needs LORA_HIP_SPECTRUM_FLAG_PEAK");
    if ((band != nullptr) != !h->bands.empty()) return sfail(h, LORA_HIP_ERR_ARG, "the band buffer is NULL iff n_bands is 0");
    const long long s0 = sp_segments(h, h->n_abs), s1 = sp_segments(h, h->n_abs + (long long)n_in);
    const size_t nr = (size_t)(s1 / h->n_avg - s0 / h->n_avg);
    *n_rows = nr;
    *first_row = (uint64_t)(s0 / h->n_avg);
    if (nr > max_rows) return sfail(h, LORA_HIP_ERR_OVERFLOW, "max_rows %zu < %zu rows", max_rows, nr);
    if (nr && (!psd || (h->peak && !peak) || row_stride < (size_t)h->nfft))
        return sfail(h, LORA_HIP_ERR_ARG, "rows to write: psd%s must not be NULL and row_stride %zu must be at least nfft", h->peak ? " and peak" : "", row_stride);
    if (s1 > s0 && (s1 - 1) / h->n_avg - s0 / h->n_avg + 1 > 0x7fffffffll) return sfail(h, LORA_HIP_ERR_ARG, "n_in %zu touches more than 2^31 - 1 rows", n_in);
    return LORA_HIP_OK;
}

lora_hip_status sp_run_device(lora_hip_spectrum_t *h, const void *d_in, size_t n_in, int fmt, float scale, float *d_psd, float *d_peak, float *d_band,
                              size_t row_stride, size_t max_rows, size_t *n_rows, uint64_t *first_row, void *hip_stream)
{
    const lora_hip_status cs = sp_check_run(h, d_in, n_in, d_psd, d_peak, d_band, row_stride, max_rows, n_rows, first_row);
    if (cs != LORA_HIP_OK) return cs;
    hipStream_t st = (hipStream_t)hip_stream;
    SP_TRY(h, hipSetDevice(h->device));
    const long long n_new = h->n_abs + (long long)n_in;
    const long long s0 = sp_segments(h, h->n_abs), s1 = sp_segments(h, n_new);
    const int c_old = (int)sp_carried(h, h->n_abs), c_new = (int)sp_carried(h, n_new);
    const size_t nr = *n_rows;
    h->last_ms = 0.0f;
    bool wrote_state = false, wrote_hist = false;
    if (s1 > s0) {
        SpArgs a{};
        a.in = d_in; a.hist = h->d_hist;
        a.state_in = h->d_state + (size_t)h->cur * 2 * h->nfft;
        a.state_out = h->d_state + (size_t)(h->cur ^ 1) * 2 * h->nfft;
        a.psd = d_psd; a.peak = h->peak ? d_peak : nullptr;
        a.n_abs = h->n_abs; a.n_in = (long long)n_in; a.seg0 = s0; a.seg1 = s1; a.row0 = s0 / h->n_avg;
        a.row_stride = (long long)row_stride;
        a.n_hist = c_old; a.nfft = h->nfft; a.hop = h->hop; a.n_avg = h->n_avg;
        a.scale = lora_iq::scale_of(fmt, scale); a.k_psd = h->k_psd; a.k_peak = h->k_peak;
        const unsigned units = (unsigned)((s1 - 1) / h->n_avg - s0 / h->n_avg + 1);
        wrote_state = s1 % h->n_avg != 0;
        SP_TRY(h, hipEventRecord(h->ev0, st));
        SP_TRY(h, sp_launch(fmt, units, h->threads, h->lds, st, a, h->d_win, h->d_tw));
        if (nr && !h->bands.empty()) {
            const unsigned long long jobs = (unsigned long long)nr * h->bands.size() / 2;
            hipLaunchKernelGGL(band_kernel, dim3((unsigned)std::min<unsigned long long>(jobs, kBandBlocksMax)), dim3(64), 0, st, (const float *)d_psd,
                               (long long)row_stride, (const uint32_t *)h->d_bands, (int)(h->bands.size() / 2), (long long)nr, d_band);
            SP_TRY(h, hipGetLastError());
        }
        SP_TRY(h, hipEventRecord(h->ev1, st));
    }
    // the next call's carried samples: the last c_new items of (carried, input), on the device for any n_in
    if (c_new > 0 && n_in) {
        if ((size_t)c_new <= n_in) {
            const size_t from = n_in - (size_t)c_new;
            if (fmt != LORA_HIP_IQ_CF32)
                SP_TRY(h, lora_iq::unpack_launch((const unsigned char *)d_in + from * lora_iq::item_bytes(fmt), (size_t)c_new, fmt, scale, h->d_hist2, st));
            else
                SP_TRY(h, hipMemcpyAsync(h->d_hist2, (const float2 *)d_in + from, (size_t)c_new * sizeof(float2), hipMemcpyDeviceToDevice, st));
        } else {
            const size_t keep = (size_t)c_new - n_in;   // <= c_old: the newest carried items stay
            SP_TRY(h, hipMemcpyAsync(h->d_hist2, h->d_hist + ((size_t)c_old - keep), keep * sizeof(float2), hipMemcpyDeviceToDevice, st));
            if (fmt != LORA_HIP_IQ_CF32)
                SP_TRY(h, lora_iq::unpack_launch(d_in, n_in, fmt, scale, h->d_hist2 + keep, st));
            else
                SP_TRY(h, hipMemcpyAsync(h->d_hist2 + keep, d_in, n_in * sizeof(float2), hipMemcpyDeviceToDevice, st));
        }
        wrote_hist = true;
    }
    SP_TRY(h, hipStreamSynchronize(st));
    if (s1 > s0) SP_TRY(h, hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1));
    // every fallible call is behind us: the handle moves on in one piece (carried samples, row in progress, item count)
    if (wrote_hist) std::swap(h->d_hist, h->d_hist2);
    if (wrote_state) h->cur ^= 1;
    h->n_abs = n_new;
    return LORA_HIP_OK;
}

// (the staging area holds n_in items of any format: it is sized for cf32)
lora_hip_status sp_work(lora_hip_spectrum_t *h, const void *in, size_t n_in, int fmt, float scale, float *psd, float *peak, float *band, size_t row_stride,
                        size_t max_rows, size_t *n_rows, uint64_t *first_row)
{
    const lora_hip_status cs = sp_check_run(h, in, n_in, psd, peak, band, row_stride, max_rows, n_rows, first_row);
    if (cs != LORA_HIP_OK) return cs;
    SP_TRY(h, hipSetDevice(h->device));
    const size_t nr = *n_rows, N = (size_t)h->nfft, nb = h->bands.size() / 2;
    if (n_in > h->stage_in_cap) {
        if (h->d_stage_in) (void)hipFree(h->d_stage_in);
        h->d_stage_in = nullptr; h->stage_in_cap = 0;
        SP_TRY(h, hipMalloc(&h->d_stage_in, (n_in + n_in / 4 + 16) * sizeof(float2)));
        h->stage_in_cap = n_in + n_in / 4 + 16;
    }
    if (std::max<size_t>(nr, 1) > h->stage_rows_cap) {
        if (h->d_stage_psd) (void)hipFree(h->d_stage_psd);
        if (h->d_stage_peak) (void)hipFree(h->d_stage_peak);
        if (h->d_stage_band) (void)hipFree(h->d_stage_band);
        h->d_stage_psd = h->d_stage_peak = h->d_stage_band = nullptr; h->stage_rows_cap = 0;
        const size_t cap = nr + nr / 4 + 4;
        SP_TRY(h, hipMalloc((void **)&h->d_stage_psd, cap * N * sizeof(float)));
        if (h->peak) SP_TRY(h, hipMalloc((void **)&h->d_stage_peak, cap * N * sizeof(float)));
        if (nb) SP_TRY(h, hipMalloc((void **)&h->d_stage_band, cap * nb * sizeof(float)));
        h->stage_rows_cap = cap;
    }
    if (n_in) SP_TRY(h, hipMemcpy(h->d_stage_in, in, n_in * lora_iq::item_bytes(fmt), hipMemcpyHostToDevice));
    const lora_hip_status s = sp_run_device(h, h->d_stage_in, n_in, fmt, scale, h->d_stage_psd, h->d_stage_peak, h->d_stage_band, N, nr, n_rows, first_row, nullptr);
    if (s != LORA_HIP_OK) return s;
    if (nr) {
        SP_TRY(h, hipMemcpy2D(psd, row_stride * sizeof(float), h->d_stage_psd, N * sizeof(float), N * sizeof(float), nr, hipMemcpyDeviceToHost));
        if (h->peak) SP_TRY(h, hipMemcpy2D(peak, row_stride * sizeof(float), h->d_stage_peak, N * sizeof(float), N * sizeof(float), nr, hipMemcpyDeviceToHost));
        if (nb) SP_TRY(h, hipMemcpy(band, h->d_stage_band, nr * nb * sizeof(float), hipMemcpyDeviceToHost));
    }
    return LORA_HIP_OK;
}

} // namespace

extern "C" {

lora_hip_status lora_hip_spectrum_create(const lora_hip_spectrum_config_t *cfg, lora_hip_spectrum_t **out)
{
    if (!cfg || !out || cfg->struct_size < sizeof(lora_hip_spectrum_config_t)) return LORA_HIP_ERR_ARG;
    *out = nullptr;
    if (cfg->n_bands && !cfg->bands) return LORA_HIP_ERR_ARG;
    const uint32_t N = cfg->nfft;
    if (N < LORA_HIP_SPECTRUM_MIN_NFFT || N > LORA_HIP_SPECTRUM_MAX_NFFT || (N & (N - 1)) != 0 || cfg->hop < 1 || cfg->hop > N || cfg->n_avg < 1 ||
        cfg->n_avg > LORA_HIP_SPECTRUM_MAX_AVG || cfg->window > LORA_HIP_SPECTRUM_WINDOW_RECT || (cfg->flags & ~LORA_HIP_SPECTRUM_FLAG_PEAK) != 0 ||
        cfg->n_bands > LORA_HIP_SPECTRUM_MAX_BANDS || !(cfg->samp_rate > 0.0) || !std::isfinite(cfg->samp_rate))
        return LORA_HIP_ERR_BAD_CONFIG;
    for (uint32_t b = 0; b < cfg->n_bands; b++) {
        const uint32_t first = cfg->bands[2 * b], n = cfg->bands[2 * b + 1];
        if (n < 1 || first >= N || n > N - first) return LORA_HIP_ERR_BAD_CONFIG;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev) return LORA_HIP_ERR_NO_DEVICE;
    auto *h = new lora_hip_spectrum;
    h->cfg = *cfg;
    h->cfg.bands = nullptr;
    h->bands.assign(cfg->bands, cfg->bands + 2 * (size_t)cfg->n_bands);
    h->device = cfg->device;
    h->nfft = (int)N; h->hop = (int)cfg->hop; h->n_avg = (int)cfg->n_avg;
    h->peak = (cfg->flags & LORA_HIP_SPECTRUM_FLAG_PEAK) != 0;
    h->threads = std::max(64, (int)N / 4);
    h->lds = 3 * (size_t)N * sizeof(float2);
    h->window.resize(N);
    double sw2 = 0.0;
    for (uint32_t k = 0; k < N; k++) {
        h->window[k] = cfg->window == LORA_HIP_SPECTRUM_WINDOW_RECT ? 1.0f : (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (double)k / (double)N));
        sw2 += (double)h->window[k] * (double)h->window[k];
    }
    const double norm = 1.0 / ((double)N * sw2);
    h->k_psd = (float)(norm / (double)cfg->n_avg);
    h->k_peak = (float)norm;
    std::vector<float2> tw(N);
    for (uint32_t i = 0; i < N; i++) {
        const double a = -2.0 * M_PI * (double)i / (double)N;
        tw[i] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    lora_hip_status st = LORA_HIP_OK;
    do {
        if (hipSetDevice(h->device) != hipSuccess) { st = LORA_HIP_ERR_NO_DEVICE; break; }
        if (hipMalloc((void **)&h->d_win, N * sizeof(float)) != hipSuccess || hipMalloc((void **)&h->d_tw, N * sizeof(float2)) != hipSuccess ||
            hipMalloc((void **)&h->d_state, 4 * (size_t)N * sizeof(float)) != hipSuccess || hipMalloc((void **)&h->d_hist, N * sizeof(float2)) != hipSuccess ||
            hipMalloc((void **)&h->d_hist2, N * sizeof(float2)) != hipSuccess ||
            hipMalloc((void **)&h->d_bands, std::max<size_t>(h->bands.size(), 2) * sizeof(uint32_t)) != hipSuccess ||
            hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) { st = LORA_HIP_ERR_NOMEM; break; }
        if (hipMemcpy(h->d_win, h->window.data(), N * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(h->d_tw, tw.data(), N * sizeof(float2), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemset(h->d_state, 0, 4 * (size_t)N * sizeof(float)) != hipSuccess ||
            (!h->bands.empty() && hipMemcpy(h->d_bands, h->bands.data(), h->bands.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess)) {
            st = LORA_HIP_ERR_HIP; break;
        }
        // one attribute for the one kernel, whatever the handle: the largest nfft's three buffers
        const size_t lds_max = 3 * (size_t)LORA_HIP_SPECTRUM_MAX_NFFT * sizeof(float2);
        if (!sp_allow_lds<LORA_HIP_IQ_CF32>(lds_max) || !sp_allow_lds<LORA_HIP_IQ_SC16>(lds_max) || !sp_allow_lds<LORA_HIP_IQ_SC8>(lds_max) ||
            !sp_allow_lds<LORA_HIP_IQ_CU8>(lds_max)) { st = LORA_HIP_ERR_HIP; break; }
    } while (false);
    if (st != LORA_HIP_OK) { lora_hip_spectrum_destroy(h); return st; }
    *out = h;
    return LORA_HIP_OK;
}

void lora_hip_spectrum_destroy(lora_hip_spectrum_t *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->d_win) (void)hipFree(h->d_win);
    if (h->d_tw) (void)hipFree(h->d_tw);
    if (h->d_state) (void)hipFree(h->d_state);
    if (h->d_hist) (void)hipFree(h->d_hist);
    if (h->d_hist2) (void)hipFree(h->d_hist2);
    if (h->d_bands) (void)hipFree(h->d_bands);
    if (h->d_stage_in) (void)hipFree(h->d_stage_in);
    if (h->d_stage_psd) (void)hipFree(h->d_stage_psd);
    if (h->d_stage_peak) (void)hipFree(h->d_stage_peak);
    if (h->d_stage_band) (void)hipFree(h->d_stage_band);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    delete h;
}

const char *lora_hip_spectrum_last_error(const lora_hip_spectrum_t *h) { return h ? h->err.c_str() : "null handle"; }

lora_hip_status lora_hip_spectrum_window(const lora_hip_spectrum_t *h, float *w, size_t cap, size_t *n)
{
    if (!h || !n) return LORA_HIP_ERR_ARG;
    *n = h->window.size();
    if (!w) return LORA_HIP_OK;
    if (cap < h->window.size()) return LORA_HIP_ERR_OVERFLOW;
    std::memcpy(w, h->window.data(), h->window.size() * sizeof(float));
    return LORA_HIP_OK;
}

size_t lora_hip_spectrum_output_rows(const lora_hip_spectrum_t *h, size_t n_in)
{
    if (!h || n_in > (size_t)1 << 40) return 0;
    return (size_t)(sp_segments(h, h->n_abs + (long long)n_in) / h->n_avg - sp_segments(h, h->n_abs) / h->n_avg);
}

lora_hip_status lora_hip_spectrum_run_device(lora_hip_spectrum_t *h, const void *d_in, size_t n_in, float *d_psd, float *d_peak, float *d_band,
                                             size_t row_stride, size_t max_rows, size_t *n_rows, uint64_t *first_row, void *hip_stream)
{
    return sp_run_device(h, d_in, n_in, LORA_HIP_IQ_CF32, 0.0f, d_psd, d_peak, d_band, row_stride, max_rows, n_rows, first_row, hip_stream);
}

lora_hip_status lora_hip_spectrum_run_device_raw(lora_hip_spectrum_t *h, const void *d_in, size_t n_in, int fmt, float scale, float *d_psd, float *d_peak,
                                                 float *d_band, size_t row_stride, size_t max_rows, size_t *n_rows, uint64_t *first_row, void *hip_stream)
{
    const lora_hip_status s = sp_check_raw(h, d_in, fmt, scale);
    return s != LORA_HIP_OK ? s : sp_run_device(h, d_in, n_in, fmt, scale, d_psd, d_peak, d_band, row_stride, max_rows, n_rows, first_row, hip_stream);
}

lora_hip_status lora_hip_spectrum_work(lora_hip_spectrum_t *h, const float *in, size_t n_in, float *psd, float *peak, float *band, size_t row_stride,
                                       size_t max_rows, size_t *n_rows, uint64_t *first_row)
{
    return sp_work(h, in, n_in, LORA_HIP_IQ_CF32, 0.0f, psd, peak, band, row_stride, max_rows, n_rows, first_row);
}

lora_hip_status lora_hip_spectrum_work_raw(lora_hip_spectrum_t *h, const void *in, size_t n_in, int fmt, float scale, float *psd, float *peak, float *band,
                                           size_t row_stride, size_t max_rows, size_t *n_rows, uint64_t *first_row)
{
    const lora_hip_status s = sp_check_raw(h, in, fmt, scale);
    return s != LORA_HIP_OK ? s : sp_work(h, in, n_in, fmt, scale, psd, peak, band, row_stride, max_rows, n_rows, first_row);
}

lora_hip_status lora_hip_spectrum_reset(lora_hip_spectrum_t *h)
{
    if (!h) return LORA_HIP_ERR_ARG;
    h->n_abs = 0;   // (no carried samples, no row in progress: both are derived from the item count)
    return LORA_HIP_OK;
}

float lora_hip_spectrum_last_kernel_ms(const lora_hip_spectrum_t *h) { return h ? h->last_ms : 0.0f; }

} // extern "C"
