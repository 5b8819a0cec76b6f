// lora_link.hip -- per-frame link metrics (include/lora_hip_link.h): the window kernel.
//
// One 256-thread workgroup per (frame, window).  A window's spectrum is the pruned dechirp spectrum of get_shift_fft /
// detect_spectrum (lora_kernels.hip, lora_detect.inc.hip: the N bins k in [-N/2, N/2) of the sps-point DFT of x * d_downchirp, no
// N/2 fold) of the Hann-windowed symbol - the same generic polyphase FFT, any SF and decimation, D / G polyphase rows of N points
// in LDS and G passes over the symbol where they do not all fit (SF12 at D = 8), a body of its own so that the decoder's
// translation unit stays as it is.  From the spectrum the workgroup forms peak bin, the fractional peak position, the power of
// the peak's lobe and of all bins; the per-frame combination is the host's, in double (lora_hip_link_combine).  No atomics, no
// state shared between workgroups; 8 B per item read once, 24 B written.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lora_link.h"

namespace lora_hip {

namespace {

__device__ __forceinline__ float2 link_cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

__device__ __forceinline__ float link_wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sums over the workgroup in a fixed order; every thread gets the total.  red: kWG / 64 floats
__device__ __forceinline__ float link_block_sum(float v, float *red)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = link_wave_sum(v);
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// first maximum of the workgroup; red: 2 * kWG / 64 words
__device__ __forceinline__ void link_block_argmax_first(float &v, int &idx, float *red)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
    __syncthreads();
    if (lane == 0) { red[wave] = v; ((int *)red)[4 + wave] = idx; }
    __syncthreads();
    v = red[0]; idx = ((int *)red)[4];
#pragma unroll
    for (int w = 1; w < kWG / 64; w++) {
        const float ov = red[w];
        const int oi = ((int *)red)[4 + w];
        if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
}

static_assert(kWG == 256, "the reductions above combine four wavefronts");

} // namespace

__global__ __launch_bounds__(kWG) void link_windows_kernel(DevParams P, const float *__restrict__ hann, const float2 *__restrict__ iq,
                                                           const LinkWindowDesc *__restrict__ wins, uint32_t n, LinkWindowRec *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t s = blockIdx.x;
    if (s >= n) return;
    const LinkWindowDesc wd = wins[s];
    if (wd.valid == 0u) return; // (uniform: before any address of the IQ buffer is formed)
    float2 *work = reinterpret_cast<float2 *>(smem);
    float *red = reinterpret_cast<float *>(smem + P.lds_work_bytes); // 16 words: behind the FFT work area (walker_lds_bytes)
    const float2 *__restrict__ x = iq + wd.offset;
    const bool conj = wd.conj != 0u;

    const uint32_t N = P.nbins, D = P.decim, G = P.fft_groups, DG = D / G, logN = P.log_nbins;
    const uint32_t stride = P.fft_stride, pts = N * DG, smask = P.sps - 1u;
    float2 acc[kMaxBinsPerThread];
#pragma unroll
    for (int m = 0; m < kMaxBinsPerThread; m++) acc[m] = make_float2(0.0f, 0.0f);
    for (uint32_t g = 0; g < G; g++) {
        // polyphase rows r = g DG + rr of this pass: y_r[q] = v[q D + r] down[q D + r] w[q D + r]
        for (uint32_t idx = threadIdx.x; idx < pts; idx += kWG) {
            const uint32_t rr = idx % DG, q = idx / DG;
            const uint32_t i = q * D + g * DG + rr;
            float2 v = x[i];
            if (conj) v.y = -v.y;
            const float2 t = link_cmul(v, P.down[i]);
            const float w = hann[i];
            work[rr * stride + q] = make_float2(t.x * w, t.y * w);
        }
        __syncthreads();
        // N-point radix-2 DIF of every row, in place (bit-reversed output)
        for (uint32_t h = N >> 1; h >= 1u; h >>= 1) {
            const uint32_t tw_step = (N >> 1) / h;
            for (uint32_t b = threadIdx.x; b < (pts >> 1); b += kWG) {
                const uint32_t arr = b / (N >> 1), j = b % (N >> 1);
                const uint32_t off = j & (h - 1u), blk = j / h;
                const uint32_t i0 = arr * stride + blk * 2u * h + off, i1 = i0 + h;
                const float2 a = work[i0], c = work[i1];
                const float2 d = make_float2(a.x - c.x, a.y - c.y);
                work[i0] = make_float2(a.x + c.x, a.y + c.y);
                work[i1] = link_cmul(d, P.twN[off * tw_step]);
            }
            __syncthreads();
        }
        // X[k] += W_sps^{k r} FFT_N(y_r)[k mod N]
#pragma unroll
        for (int m = 0; m < kMaxBinsPerThread; m++) {
            const uint32_t j = threadIdx.x + (uint32_t)m * kWG;
            if (j < N) {
                const int32_t k = (j < N / 2u) ? (int32_t)j : (int32_t)j - (int32_t)N;
                const uint32_t jr = __brev(j) >> (32u - logN);
                for (uint32_t rr = 0; rr < DG; rr++) {
                    const uint32_t r = g * DG + rr;
                    const float2 t = link_cmul(work[rr * stride + jr], P.tws[(uint32_t)(k * (int32_t)r) & smask]);
                    acc[m].x += t.x; acc[m].y += t.y;
                }
            }
        }
        __syncthreads();
    }
    float bv = -1.0f, tot = 0.0f;
    int bi = 0;
#pragma unroll
    for (int m = 0; m < kMaxBinsPerThread; m++) {
        const uint32_t j = threadIdx.x + (uint32_t)m * kWG;
        if (j < N) {
            const float pw = acc[m].x * acc[m].x + acc[m].y * acc[m].y;
            tot += pw;
            if (pw > bv) { bv = pw; bi = (int)j; }
        }
    }
    tot = link_block_sum(tot, red);
    link_block_argmax_first(bv, bi, red);
    // the lobe around the peak (indices mod N) and the peak's two neighbours
    float lobe = 0.0f;
#pragma unroll
    for (int m = 0; m < kMaxBinsPerThread; m++) {
        const uint32_t j = threadIdx.x + (uint32_t)m * kWG;
        if (j < N) {
            const uint32_t d = (j - (uint32_t)bi) & (N - 1u); // distance above the peak, mod N
            if (d <= (uint32_t)kLinkLobe || d >= N - (uint32_t)kLinkLobe) {
                const float pw = acc[m].x * acc[m].x + acc[m].y * acc[m].y;
                lobe += pw;
                if (d == 1u) red[12] = pw;
                if (d == N - 1u) red[13] = pw;
            }
        }
    }
    lobe = link_block_sum(lobe, red); // (its barriers also publish red[12], red[13])
    if (threadIdx.x == 0) {
        const float a = sqrtf(red[13]), b = sqrtf(red[12]), pk = sqrtf(bv);
        float frac = 0.0f;
        if (pk > 0.0f) {
            const float alpha = fmaxf(a, b) / pk;
            const float dd = (2.0f * alpha - 1.0f) / (alpha + 1.0f);
            frac = (b >= a) ? dd : -dd;
        }
        LinkWindowRec r;
        r.peak_bin = bi; r.frac = frac; r.lobe_power = lobe; r.total_power = tot; r.peak_power = bv; r.valid = 1u;
        out[s] = r;
    }
}

int launch_link_windows(const DevParams &p, const float *d_hann, const float2 *iq, const LinkWindowDesc *d_wins, uint32_t n, LinkWindowRec *d_out, void *stream)
{
    if (n == 0) return 0;
    const uint32_t lds = walker_lds_bytes(p); // the FFT work area + at least 1280 B behind it: this kernel uses 64 of them
    if (lds > 64u * 1024u) {
        if (hipFuncSetAttribute((const void *)link_windows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -1;
    }
    hipLaunchKernelGGL(link_windows_kernel, dim3(n), dim3(kWG), lds, (hipStream_t)stream, p, d_hann, iq, d_wins, n, d_out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace lora_hip
