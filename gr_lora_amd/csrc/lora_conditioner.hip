// lora_conditioner.hip -- MI355X IQ conditioner: DC-offset removal and IQ-imbalance correction from block moments.  C ABI and the
// definition in include/lora_hip_conditioner.h; float64 model of the same definition in gr_lora_amd/conditioner.py (condition).
//
// Two kernels per call, launched back to back on the caller's stream; the second reads what the first wrote, in stream order.
//   cd_moments_kernel   one wavefront per complete block, kMomentBlocks of them to a workgroup.  Lane p runs chain p of the
//                       header's summation order: items p, p + 64, ... of the block, converted as they are loaded
//                       (lora_iq::load<F>), widened to double, five running sums from +0.  A row of 64 cf32 items is one 512-byte
//                       read of the wavefront.  The 64 totals are reduced by the header's halving tree with wavefront shuffles
//                       and lane 0 writes the block's record.  An item in front of this call's first comes from the handle's
//                       held items (cf32): only the call's first block can straddle the two.
//   cd_apply_kernel     a workgroup streams kApplyItems items of one block (the whole block where B is smaller).  Threads 0 .. 4
//                       form the block's window sums from the carried records and the new ones, ascending; thread 0 runs the ten
//                       fp64 operations, rounds the four parameters to fp32 and, in the block's first workgroup, writes them and
//                       the estimates next to the moments.  Then every thread converts two adjacent items per step: 16-byte
//                       loads (cf32) and 16-byte stores where the held count is even and the pointers are 16-byte aligned,
//                       item by item otherwise; both give the same bits.
//   cd_tail_kernel      flush: the held items with the newest parameters.
// A record is kRecDoubles doubles: the five moments, mI, mQ, r, q, then dI, dQ, a, b as four floats.  The records of a call sit
// behind the W - 1 carried ones in one buffer; the last W - 1 of both are copied to the front of a second buffer for the next
// call, and the two swap.  No workgroup waits for another.  fp64 '/' and sqrt are the correctly rounded ones hipcc emits by
// default, and contraction is off in this file (the pragma below), so every operator below is one IEEE operation.
// Design and measurements: DESIGN.md 4.18.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lora_hip_conditioner.h"
#include "lora_iq.h"

#pragma clang fp contract(off)

namespace {

constexpr int kRow = 64;                 // chains per block = lanes of a wavefront
constexpr int kMomentBlocks = 4;         // wavefronts (blocks) per workgroup of cd_moments_kernel
constexpr int kApplyThreads = 256;
constexpr uint32_t kApplyItems = 4096;   // items per workgroup of cd_apply_kernel, at most
constexpr int kRecDoubles = 12;          // S_I, S_Q, S_II, S_QQ, S_IQ, mI, mQ, r, q, (dI, dQ), (a, b), spare
constexpr int kRecEst = 5, kRecPar = 9;
constexpr int kLastDoubles = 6;          // newest block: mI, mQ, r, q, (dI, dQ), (a, b)

struct CdArgs {
    const void *in;          // new input items of format F
    const float2 *held;      // the n_held items in front of in[0] (cf32)
    double *rec;             // W - 1 carried records, then this call's
    double *last;            // the newest block's estimates and parameters
    float2 *out;
    long long n_in;
    long long n_blocks;
    int n_held;
    int B, W;
    int n_hist;              // how many of the carried records belong to the window
    int chunks;              // workgroups per block in cd_apply_kernel
    int items;               // items per workgroup there
    int vec;                 // 16-byte path allowed
    int flags;
    int fixed;
    float fx[4];
    float scale;
};

// item j of (held, in): j counts from the first held item
template <int F>
__device__ __forceinline__ float2 cd_item(const CdArgs &A, long long j)
{
    return j < A.n_held ? A.held[j] : lora_iq::load<F>(A.in, j - A.n_held, A.scale);
}

template <int F>
__global__ __launch_bounds__(kRow * kMomentBlocks) void cd_moments_kernel(CdArgs A)
{
    const int lane = (int)(threadIdx.x & (kRow - 1));
    const long long blk = (long long)blockIdx.x * kMomentBlocks + (long long)(threadIdx.x / kRow);
    if (blk >= A.n_blocks) return;                       // (the whole wavefront; nothing below synchronises the workgroup)
    const long long j0 = blk * A.B + lane;
    const int rows = A.B / kRow;                         // >= 4, a power of two
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int r = 0; r < rows; r += 4) {
        float2 v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = cd_item<F>(A, j0 + (long long)(r + k) * kRow);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double I = (double)v[k].x, Q = (double)v[k].y;
            s[0] = s[0] + I;
            s[1] = s[1] + Q;
            s[2] = s[2] + I * I;                         // (the products are exact, 24-bit factors: a fused step gives the same bits)
            s[3] = s[3] + Q * Q;
            s[4] = s[4] + I * Q;
        }
    }
#pragma unroll
    for (int st = kRow / 2; st >= 1; st >>= 1) {
#pragma unroll
        for (int c = 0; c < 5; c++) s[c] = s[c] + __shfl_down(s[c], st, kRow);   // (lanes >= st hold values nobody reads)
    }
    if (lane == 0) {
        double *rec = A.rec + ((long long)(A.W - 1) + blk) * kRecDoubles;
#pragma unroll
        for (int c = 0; c < 5; c++) rec[c] = s[c];
    }
}

__device__ __forceinline__ float2 cd_correct(float2 v, float dI, float dQ, float a, float b)
{
    const float zI = v.x - dI;
    const float u = v.y - dQ;
    const float p0 = a * zI, p1 = b * u;                 // (two roundings, then the sum's: contraction is off in this file)
    return make_float2(zI, p0 + p1);
}

template <int F>
__global__ __launch_bounds__(kApplyThreads) void cd_apply_kernel(CdArgs A)
{
    __shared__ double S[5];
    __shared__ float P[4];
    const int t = (int)threadIdx.x;
    const long long blk = (long long)(blockIdx.x / (unsigned)A.chunks);
    const int chunk = (int)(blockIdx.x % (unsigned)A.chunks);
    double *rec = A.rec + ((long long)(A.W - 1) + blk) * kRecDoubles;
    const bool newest = chunk == 0 && blk == A.n_blocks - 1;
    if (A.fixed) {
        if (t < 4) {
            P[t] = A.fx[t];
            if (chunk == 0) reinterpret_cast<float *>(rec + kRecPar)[t] = A.fx[t];
            if (newest) reinterpret_cast<float *>(A.last + 4)[t] = A.fx[t];
        }
    } else {
        const long long avail = (long long)A.n_hist + blk;                       // window blocks in front of this one
        const int nw = (int)(avail < (long long)(A.W - 1) ? avail : (long long)(A.W - 1)) + 1;
        if (t < 5) {
            const double *p = rec - (long long)(nw - 1) * kRecDoubles + t;
            double acc = 0.0;
            for (int i = 0; i < nw; i++) acc = acc + p[(long long)i * kRecDoubles];
            S[t] = acc;
        }
        __syncthreads();
        if (t == 0) {
            const double cnt = (double)nw * (double)A.B;
            const double mI = S[0] / cnt, mQ = S[1] / cnt;
            const double cII = S[2] / cnt - mI * mI;
            const double cQQ = S[3] / cnt - mQ * mQ;
            const double cIQ = S[4] / cnt - mI * mQ;
            const double r = cIQ / cII, q = cQQ / cII;
            const double e = q - r * r;
            double b = 1.0 / sqrt(e);
            double a = -r * b;
            if (!(cII > 0.0) || !(e > 0x1p-12)) { a = 0.0; b = 1.0; }
            const bool dc = (A.flags & LORA_HIP_CONDITIONER_FLAG_DC) != 0, iq = (A.flags & LORA_HIP_CONDITIONER_FLAG_IQ) != 0;
            P[0] = dc ? (float)mI : 0.0f;
            P[1] = dc ? (float)mQ : 0.0f;
            P[2] = iq ? (float)a : 0.0f;
            P[3] = iq ? (float)b : 1.0f;
            if (chunk == 0) {
                rec[kRecEst + 0] = mI; rec[kRecEst + 1] = mQ; rec[kRecEst + 2] = r; rec[kRecEst + 3] = q;
                float *pf = reinterpret_cast<float *>(rec + kRecPar);
                pf[0] = P[0]; pf[1] = P[1]; pf[2] = P[2]; pf[3] = P[3];
            }
            if (newest) {
                A.last[0] = mI; A.last[1] = mQ; A.last[2] = r; A.last[3] = q;
                float *pf = reinterpret_cast<float *>(A.last + 4);
                pf[0] = P[0]; pf[1] = P[1]; pf[2] = P[2]; pf[3] = P[3];
            }
        }
    }
    __syncthreads();
    const float dI = P[0], dQ = P[1], a = P[2], b = P[3];
    const long long j0 = blk * A.B + (long long)chunk * A.items;                  // counted from the first held item; even
    if (A.vec) {
        // n_held is even: the pair (j, j + 1), j even, lies in the held items or in the input, never across
        for (int i = 2 * t; i < A.items; i += 2 * kApplyThreads) {
            const long long j = j0 + i;
            float2 v0, v1;
            if (j < A.n_held) {
                const float4 w = *reinterpret_cast<const float4 *>(A.held + j);
                v0 = make_float2(w.x, w.y); v1 = make_float2(w.z, w.w);
            } else if constexpr (F == LORA_HIP_IQ_CF32) {
                const float4 w = *reinterpret_cast<const float4 *>(reinterpret_cast<const float2 *>(A.in) + (j - A.n_held));
                v0 = make_float2(w.x, w.y); v1 = make_float2(w.z, w.w);
            } else {
                v0 = lora_iq::load<F>(A.in, j - A.n_held, A.scale);
                v1 = lora_iq::load<F>(A.in, j - A.n_held + 1, A.scale);
            }
            const float2 y0 = cd_correct(v0, dI, dQ, a, b), y1 = cd_correct(v1, dI, dQ, a, b);
            *reinterpret_cast<float4 *>(A.out + j) = make_float4(y0.x, y0.y, y1.x, y1.y);
        }
    } else {
        for (int i = t; i < A.items; i += kApplyThreads) {
            const long long j = j0 + i;
            A.out[j] = cd_correct(cd_item<F>(A, j), dI, dQ, a, b);
        }
    }
}

// flush: out[i] = the held item i with the newest parameters (or the fixed ones)
__global__ __launch_bounds__(kApplyThreads) void cd_tail_kernel(const float2 *held, int n, const double *last, int fixed, float f0, float f1, float f2, float f3,
                                                               float2 *out)
{
    const float *pf = reinterpret_cast<const float *>(last + 4);
    const float dI = fixed ? f0 : pf[0], dQ = fixed ? f1 : pf[1], a = fixed ? f2 : pf[2], b = fixed ? f3 : pf[3];
    const int i = (int)(blockIdx.x * kApplyThreads + threadIdx.x);
    if (i < n) out[i] = cd_correct(held[i], dI, dQ, a, b);
}

} // namespace

struct lora_hip_conditioner {
    uint32_t B = 4096, W = 16, flags = 3;
    int device = 0;
    uint32_t n_held = 0;        // items of the partial block
    uint32_t n_hist = 0;        // carried records that belong to the window: min(W - 1, blocks since the window started)
    uint64_t n_emitted = 0;     // items written so far
    uint64_t n_blocks = 0;      // blocks completed so far
    bool fixed = false;
    float fx[4] = {0.0f, 0.0f, 0.0f, 1.0f};
    float2 *d_held = nullptr;   // B items
    double *d_rec = nullptr, *d_rec2 = nullptr;   // W - 1 + rec_cap records each; d_rec2 holds the last call's after the swap
    size_t rec_cap = 0;
    size_t last_blocks = 0;     // records of the last call, in d_rec2 behind the first W - 1
    double *d_last = nullptr;
    void *d_stage_in = nullptr;
    float2 *d_stage_out = nullptr;
    size_t stage_in_cap = 0, stage_out_cap = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_ms = 0.0f;
    std::string err;
};

namespace {

lora_hip_status cfail(lora_hip_conditioner *h, lora_hip_status s, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    return s;
}
#define CD_TRY(h, call)                                                                                    \
    do {                                                                                                   \
        hipError_t e_ = (call);                                                                            \
        if (e_ != hipSuccess) return cfail((h), LORA_HIP_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

constexpr size_t kMaxItemsPerCall = (size_t)1 << 40;

void cd_last_init(double *v)
{
    std::memset(v, 0, kLastDoubles * sizeof(double));
    const float id[4] = {0.0f, 0.0f, 0.0f, 1.0f};
    std::memcpy(v + 4, id, sizeof id);
}

uint32_t cd_apply_items(uint32_t B) { return std::min(B, kApplyItems); }

template <int F>
hipError_t cd_launch_as(hipStream_t st, const CdArgs &a)
{
    const unsigned g1 = (unsigned)((a.n_blocks + kMomentBlocks - 1) / kMomentBlocks);
    if (!a.fixed) hipLaunchKernelGGL((cd_moments_kernel<F>), dim3(g1), dim3(kRow * kMomentBlocks), 0, st, a);
    hipLaunchKernelGGL((cd_apply_kernel<F>), dim3((unsigned)(a.n_blocks * a.chunks)), dim3(kApplyThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t cd_launch(int fmt, hipStream_t st, const CdArgs &a)
{
    switch (fmt) {
    case LORA_HIP_IQ_SC16: return cd_launch_as<LORA_HIP_IQ_SC16>(st, a);
    case LORA_HIP_IQ_SC8: return cd_launch_as<LORA_HIP_IQ_SC8>(st, a);
    case LORA_HIP_IQ_CU8: return cd_launch_as<LORA_HIP_IQ_CU8>(st, a);
    default: return cd_launch_as<LORA_HIP_IQ_CF32>(st, a);
    }
}

lora_hip_status cd_check_raw(lora_hip_conditioner *h, const void *p, int fmt, float scale)
{
    if (!h) return LORA_HIP_ERR_ARG;
    if (!lora_iq::args_ok(p, fmt, scale)) return cfail(h, LORA_HIP_ERR_ARG, "unknown format %d, unusable scale %g, or input not aligned to its component", fmt, (double)scale);
    return LORA_HIP_OK;
}

// what a call of n_in items emits, and the pointer rules of the header; no device call
lora_hip_status cd_check_run(lora_hip_conditioner *h, const void *in, size_t n_in, size_t item_bytes, const void *out, size_t max_out, size_t *n_out,
                             uint64_t *first_out)
{
    if (!h || !n_out || !first_out || (n_in && !in)) return LORA_HIP_ERR_ARG;
    if (n_in > kMaxItemsPerCall) return cfail(h, LORA_HIP_ERR_ARG, "n_in %zu: at most 2^40 items per call", n_in);
    const size_t nr = ((size_t)h->n_held + n_in) / h->B * h->B;
    *n_out = nr;
    *first_out = h->n_emitted;
    if (nr > max_out) return cfail(h, LORA_HIP_ERR_OVERFLOW, "max_out %zu < %zu outputs", max_out, nr);
    if (nr && !out) return cfail(h, LORA_HIP_ERR_ARG, "outputs to write: out must not be NULL");
    if (((uintptr_t)out & 7u) != 0) return cfail(h, LORA_HIP_ERR_ARG, "out must be aligned to 8 bytes");
    if (nr && n_in) {
        const uintptr_t i0 = (uintptr_t)in, i1 = i0 + n_in * item_bytes, o0 = (uintptr_t)out, o1 = o0 + nr * sizeof(float2);
        if (i0 < o1 && o0 < i1) return cfail(h, LORA_HIP_ERR_ARG, "d_out overlaps d_in");
    }
    if (nr / cd_apply_items(h->B) > 0x7fffffffull) return cfail(h, LORA_HIP_ERR_ARG, "n_in %zu yields more than 2^31 - 1 workgroups", n_in);
    return LORA_HIP_OK;
}

// room for n more records behind the carried ones, in both buffers; the carried ones move along
lora_hip_status cd_reserve_records(lora_hip_conditioner *h, size_t n, hipStream_t st)
{
    if (n <= h->rec_cap) return LORA_HIP_OK;
    const size_t cap = n + n / 4 + 16, keep = (size_t)h->W - 1;
    double *a = nullptr, *b = nullptr;
    if (hipMalloc((void **)&a, (keep + cap) * kRecDoubles * sizeof(double)) != hipSuccess || hipMalloc((void **)&b, (keep + cap) * kRecDoubles * sizeof(double)) != hipSuccess) {
        if (a) (void)hipFree(a);
        return cfail(h, LORA_HIP_ERR_NOMEM, "no device memory for %zu block records", cap);
    }
    hipError_t e = hipStreamSynchronize(st);
    if (e == hipSuccess && keep) e = hipMemcpy(a, h->d_rec, keep * kRecDoubles * sizeof(double), hipMemcpyDeviceToDevice);
    if (e != hipSuccess) {
        (void)hipFree(a); (void)hipFree(b);
        return cfail(h, LORA_HIP_ERR_HIP, "moving the carried records: %s", hipGetErrorString(e));
    }
    (void)hipFree(h->d_rec); (void)hipFree(h->d_rec2);
    h->d_rec = a; h->d_rec2 = b; h->rec_cap = cap;
    h->last_blocks = 0;                                   // (the last call's records went with the old buffer)
    return LORA_HIP_OK;
}

lora_hip_status cd_run_device(lora_hip_conditioner_t *h, const void *d_in, size_t n_in, int fmt, float scale, void *d_out, size_t max_out, size_t *n_out,
                              uint64_t *first_out, void *hip_stream)
{
    const lora_hip_status cs = cd_check_run(h, d_in, n_in, lora_iq::item_bytes(fmt), d_out, max_out, n_out, first_out);
    if (cs != LORA_HIP_OK) return cs;
    hipStream_t st = (hipStream_t)hip_stream;
    CD_TRY(h, hipSetDevice(h->device));
    const size_t nr = *n_out, nb = nr / h->B, keep = (size_t)h->W - 1;
    const size_t held_after = (size_t)h->n_held + n_in - nr;
    h->last_ms = 0.0f;
    if (nb) {
        const lora_hip_status rs = cd_reserve_records(h, nb, st);
        if (rs != LORA_HIP_OK) return rs;
        CdArgs a{};
        a.in = d_in; a.held = h->d_held; a.rec = h->d_rec; a.last = h->d_last; a.out = (float2 *)d_out;
        a.n_in = (long long)n_in; a.n_blocks = (long long)nb; a.n_held = (int)h->n_held;
        a.B = (int)h->B; a.W = (int)h->W; a.n_hist = (int)h->n_hist;
        a.items = (int)cd_apply_items(h->B); a.chunks = (int)(h->B / (uint32_t)a.items);
        const uintptr_t in_align = fmt == LORA_HIP_IQ_CF32 ? 15u : 0u;
        a.vec = (h->n_held % 2 == 0) && ((uintptr_t)d_out & 15u) == 0 && ((uintptr_t)d_in & in_align) == 0;
        a.flags = (int)h->flags; a.fixed = h->fixed ? 1 : 0;
        std::memcpy(a.fx, h->fx, sizeof a.fx);
        a.scale = lora_iq::scale_of(fmt, scale);
        if (h->fixed) CD_TRY(h, hipMemsetAsync(h->d_rec + keep * kRecDoubles, 0, nb * kRecDoubles * sizeof(double), st));
        CD_TRY(h, hipEventRecord(h->ev0, st));
        CD_TRY(h, cd_launch(fmt, st, a));
        CD_TRY(h, hipEventRecord(h->ev1, st));
        // the next call's carried records: the last W - 1 of (carried, new), to the front of the other buffer
        if (keep) CD_TRY(h, hipMemcpyAsync(h->d_rec2, h->d_rec + nb * kRecDoubles, keep * kRecDoubles * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    // the next call's held items: behind the kernels in stream order, so the buffer they read may be written
    if (held_after) {
        const size_t from = nb ? n_in - held_after : 0, n_new = nb ? held_after : n_in;
        float2 *dst = h->d_held + (nb ? 0 : h->n_held);
        if (n_new) {
            if (fmt != LORA_HIP_IQ_CF32)
                CD_TRY(h, lora_iq::unpack_launch((const unsigned char *)d_in + from * lora_iq::item_bytes(fmt), n_new, fmt, scale, dst, st));
            else
                CD_TRY(h, hipMemcpyAsync(dst, (const float2 *)d_in + from, n_new * sizeof(float2), hipMemcpyDeviceToDevice, st));
        }
    }
    CD_TRY(h, hipStreamSynchronize(st));
    if (nb) CD_TRY(h, hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1));
    // every fallible call is behind us: the handle moves on in one piece
    if (nb) {
        std::swap(h->d_rec, h->d_rec2);
        h->n_hist = h->fixed ? 0u : (uint32_t)std::min<size_t>(keep, (size_t)h->n_hist + nb);
    }
    h->last_blocks = nb;
    h->n_held = (uint32_t)held_after;
    h->n_emitted += nr;
    h->n_blocks += nb;
    return LORA_HIP_OK;
}

lora_hip_status cd_grow_stage_out(lora_hip_conditioner *h, size_t nr)
{
    if (nr <= h->stage_out_cap) return LORA_HIP_OK;
    if (h->d_stage_out) (void)hipFree(h->d_stage_out);
    h->d_stage_out = nullptr; h->stage_out_cap = 0;
    CD_TRY(h, hipMalloc((void **)&h->d_stage_out, (nr + nr / 4 + 16) * sizeof(float2)));
    h->stage_out_cap = nr + nr / 4 + 16;
    return LORA_HIP_OK;
}

// (the staging area holds n_in items of any format: it is sized for cf32)
lora_hip_status cd_work(lora_hip_conditioner_t *h, const void *in, size_t n_in, int fmt, float scale, float *out, size_t max_out, size_t *n_out, uint64_t *first_out)
{
    const lora_hip_status cs = cd_check_run(h, in, n_in, lora_iq::item_bytes(fmt), out, max_out, n_out, first_out);
    if (cs != LORA_HIP_OK) return cs;
    const size_t nr = *n_out;
    CD_TRY(h, hipSetDevice(h->device));
    if (n_in > h->stage_in_cap) {
        if (h->d_stage_in) (void)hipFree(h->d_stage_in);
        h->d_stage_in = nullptr; h->stage_in_cap = 0;
        CD_TRY(h, hipMalloc(&h->d_stage_in, (n_in + n_in / 4 + 16) * sizeof(float2)));
        h->stage_in_cap = n_in + n_in / 4 + 16;
    }
    const lora_hip_status gs = cd_grow_stage_out(h, nr);
    if (gs != LORA_HIP_OK) return gs;
    if (n_in) CD_TRY(h, hipMemcpy(h->d_stage_in, in, n_in * lora_iq::item_bytes(fmt), hipMemcpyHostToDevice));
    const lora_hip_status s = cd_run_device(h, h->d_stage_in, n_in, fmt, scale, h->d_stage_out, nr, n_out, first_out, nullptr);
    if (s != LORA_HIP_OK) return s;
    if (nr) CD_TRY(h, hipMemcpy(out, h->d_stage_out, nr * sizeof(float2), hipMemcpyDeviceToHost));
    return LORA_HIP_OK;
}

} // namespace

extern "C" {

lora_hip_status lora_hip_conditioner_create(const lora_hip_conditioner_config_t *cfg, lora_hip_conditioner_t **out)
{
    if (!cfg || !out || cfg->struct_size < sizeof(lora_hip_conditioner_config_t)) return LORA_HIP_ERR_ARG;
    *out = nullptr;
    const uint32_t B = cfg->block ? cfg->block : 4096u, W = cfg->window ? cfg->window : 16u;
    if (B < LORA_HIP_CONDITIONER_MIN_BLOCK || B > LORA_HIP_CONDITIONER_MAX_BLOCK || (B & (B - 1)) != 0 || W > LORA_HIP_CONDITIONER_MAX_WINDOW ||
        (cfg->flags & ~(LORA_HIP_CONDITIONER_FLAG_DC | LORA_HIP_CONDITIONER_FLAG_IQ)) != 0)
        return LORA_HIP_ERR_BAD_CONFIG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev) return LORA_HIP_ERR_NO_DEVICE;
    auto *h = new lora_hip_conditioner;
    h->B = B; h->W = W; h->flags = cfg->flags; h->device = cfg->device;
    h->rec_cap = 64;
    const size_t rec_bytes = ((size_t)W - 1 + h->rec_cap) * kRecDoubles * sizeof(double);
    double last[kLastDoubles];
    cd_last_init(last);
    lora_hip_status st = LORA_HIP_OK;
    do {
        if (hipSetDevice(h->device) != hipSuccess) { st = LORA_HIP_ERR_NO_DEVICE; break; }
        if (hipMalloc((void **)&h->d_held, (size_t)B * sizeof(float2)) != hipSuccess || hipMalloc((void **)&h->d_rec, rec_bytes) != hipSuccess ||
            hipMalloc((void **)&h->d_rec2, rec_bytes) != hipSuccess || hipMalloc((void **)&h->d_last, sizeof last) != hipSuccess ||
            hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) {
            st = LORA_HIP_ERR_NOMEM; break;
        }
        if (hipMemset(h->d_held, 0, (size_t)B * sizeof(float2)) != hipSuccess || hipMemset(h->d_rec, 0, rec_bytes) != hipSuccess ||
            hipMemset(h->d_rec2, 0, rec_bytes) != hipSuccess || hipMemcpy(h->d_last, last, sizeof last, hipMemcpyHostToDevice) != hipSuccess) { st = LORA_HIP_ERR_HIP; break; }
    } while (false);
    if (st != LORA_HIP_OK) { lora_hip_conditioner_destroy(h); return st; }
    *out = h;
    return LORA_HIP_OK;
}

void lora_hip_conditioner_destroy(lora_hip_conditioner_t *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->d_held) (void)hipFree(h->d_held);
    if (h->d_rec) (void)hipFree(h->d_rec);
    if (h->d_rec2) (void)hipFree(h->d_rec2);
    if (h->d_last) (void)hipFree(h->d_last);
    if (h->d_stage_in) (void)hipFree(h->d_stage_in);
    if (h->d_stage_out) (void)hipFree(h->d_stage_out);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    delete h;
}

const char *lora_hip_conditioner_last_error(const lora_hip_conditioner_t *h) { return h ? h->err.c_str() : "null handle"; }

size_t lora_hip_conditioner_output_items(const lora_hip_conditioner_t *h, size_t n_in)
{
    if (!h || n_in > kMaxItemsPerCall) return 0;
    return ((size_t)h->n_held + n_in) / h->B * h->B;
}

lora_hip_status lora_hip_conditioner_get_plan(const lora_hip_conditioner_t *h, uint32_t *block, uint32_t *window, uint32_t *blocks_per_group, uint32_t *items_per_group)
{
    if (!h) return LORA_HIP_ERR_ARG;
    if (block) *block = h->B;
    if (window) *window = h->W;
    if (blocks_per_group) *blocks_per_group = kMomentBlocks;
    if (items_per_group) *items_per_group = cd_apply_items(h->B);
    return LORA_HIP_OK;
}

lora_hip_status lora_hip_conditioner_run_device(lora_hip_conditioner_t *h, const void *d_in, size_t n_in, void *d_out, size_t max_out, size_t *n_out,
                                                uint64_t *first_out, void *hip_stream)
{
    return cd_run_device(h, d_in, n_in, LORA_HIP_IQ_CF32, 0.0f, d_out, max_out, n_out, first_out, hip_stream);
}

lora_hip_status lora_hip_conditioner_run_device_raw(lora_hip_conditioner_t *h, const void *d_in, size_t n_in, int fmt, float scale, void *d_out, size_t max_out,
                                                    size_t *n_out, uint64_t *first_out, void *hip_stream)
{
    const lora_hip_status s = cd_check_raw(h, d_in, fmt, scale);
    return s != LORA_HIP_OK ? s : cd_run_device(h, d_in, n_in, fmt, scale, d_out, max_out, n_out, first_out, hip_stream);
}

lora_hip_status lora_hip_conditioner_work(lora_hip_conditioner_t *h, const float *in, size_t n_in, float *out, size_t max_out, size_t *n_out, uint64_t *first_out)
{
    return cd_work(h, in, n_in, LORA_HIP_IQ_CF32, 0.0f, out, max_out, n_out, first_out);
}

lora_hip_status lora_hip_conditioner_work_raw(lora_hip_conditioner_t *h, const void *in, size_t n_in, int fmt, float scale, float *out, size_t max_out,
                                              size_t *n_out, uint64_t *first_out)
{
    const lora_hip_status s = cd_check_raw(h, in, fmt, scale);
    return s != LORA_HIP_OK ? s : cd_work(h, in, n_in, fmt, scale, out, max_out, n_out, first_out);
}

lora_hip_status lora_hip_conditioner_flush_device(lora_hip_conditioner_t *h, void *d_out, size_t max_out, size_t *n_out, uint64_t *first_out, void *hip_stream)
{
    if (!h || !n_out || !first_out) return LORA_HIP_ERR_ARG;
    const size_t n = h->n_held;
    *n_out = n;
    *first_out = h->n_emitted;
    if (n > max_out) return cfail(h, LORA_HIP_ERR_OVERFLOW, "max_out %zu < %zu held items", max_out, n);
    if (n && !d_out) return cfail(h, LORA_HIP_ERR_ARG, "held items to write: out must not be NULL");
    if (((uintptr_t)d_out & 7u) != 0) return cfail(h, LORA_HIP_ERR_ARG, "out must be aligned to 8 bytes");
    if (!n) return LORA_HIP_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    CD_TRY(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(cd_tail_kernel, dim3((unsigned)((n + kApplyThreads - 1) / kApplyThreads)), dim3(kApplyThreads), 0, st, h->d_held, (int)n, h->d_last,
                       h->fixed ? 1 : 0, h->fx[0], h->fx[1], h->fx[2], h->fx[3], (float2 *)d_out);
    CD_TRY(h, hipGetLastError());
    CD_TRY(h, hipStreamSynchronize(st));
    h->n_held = 0;
    h->n_emitted += n;
    return LORA_HIP_OK;
}

lora_hip_status lora_hip_conditioner_flush(lora_hip_conditioner_t *h, float *out, size_t max_out, size_t *n_out, uint64_t *first_out)
{
    if (!h || !n_out || !first_out) return LORA_HIP_ERR_ARG;
    const size_t n = h->n_held;
    *n_out = n;
    *first_out = h->n_emitted;
    if (n > max_out) return cfail(h, LORA_HIP_ERR_OVERFLOW, "max_out %zu < %zu held items", max_out, n);
    if (n && !out) return cfail(h, LORA_HIP_ERR_ARG, "held items to write: out must not be NULL");
    if (!n) return LORA_HIP_OK;
    CD_TRY(h, hipSetDevice(h->device));
    const lora_hip_status gs = cd_grow_stage_out(h, n);
    if (gs != LORA_HIP_OK) return gs;
    const lora_hip_status s = lora_hip_conditioner_flush_device(h, h->d_stage_out, n, n_out, first_out, nullptr);
    if (s != LORA_HIP_OK) return s;
    CD_TRY(h, hipMemcpy(out, h->d_stage_out, n * sizeof(float2), hipMemcpyDeviceToHost));
    return LORA_HIP_OK;
}

lora_hip_status lora_hip_conditioner_reset(lora_hip_conditioner_t *h)
{
    if (!h) return LORA_HIP_ERR_ARG;
    double last[kLastDoubles];
    cd_last_init(last);
    CD_TRY(h, hipSetDevice(h->device));
    CD_TRY(h, hipMemcpy(h->d_last, last, sizeof last, hipMemcpyHostToDevice));
    h->n_held = 0; h->n_hist = 0; h->n_emitted = 0; h->n_blocks = 0; h->last_blocks = 0;
    return LORA_HIP_OK;
}

lora_hip_status lora_hip_conditioner_set_fixed(lora_hip_conditioner_t *h, float d_i, float d_q, float a, float b)
{
    if (!h) return LORA_HIP_ERR_ARG;
    if (!std::isfinite(d_i) || !std::isfinite(d_q) || !std::isfinite(a) || !std::isfinite(b)) return cfail(h, LORA_HIP_ERR_ARG, "the four constants must be finite");
    h->fixed = true;
    h->fx[0] = d_i; h->fx[1] = d_q; h->fx[2] = a; h->fx[3] = b;
    h->n_hist = 0;
    return LORA_HIP_OK;
}

lora_hip_status lora_hip_conditioner_set_adaptive(lora_hip_conditioner_t *h)
{
    if (!h) return LORA_HIP_ERR_ARG;
    if (h->fixed) h->n_hist = 0;
    h->fixed = false;
    return LORA_HIP_OK;
}

lora_hip_status lora_hip_conditioner_block_records(lora_hip_conditioner_t *h, double *moments, float *params, size_t cap, size_t *n, float *newest_params,
                                                   double *newest_estimates)
{
    if (!h || !n) return LORA_HIP_ERR_ARG;
    const size_t nb = h->last_blocks;
    *n = nb;
    if ((moments || params) && cap < nb) return cfail(h, LORA_HIP_ERR_OVERFLOW, "room for %zu records < %zu", cap, nb);
    if (!(((moments || params) && nb) || newest_params || newest_estimates)) return LORA_HIP_OK;
    CD_TRY(h, hipSetDevice(h->device));
    if ((moments || params) && nb) {
        std::vector<double> rec(nb * kRecDoubles);
        CD_TRY(h, hipMemcpy(rec.data(), h->d_rec2 + ((size_t)h->W - 1) * kRecDoubles, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < nb; i++) {
            if (moments) std::memcpy(moments + 5 * i, &rec[i * kRecDoubles], 5 * sizeof(double));
            if (params) std::memcpy(params + 4 * i, &rec[i * kRecDoubles + kRecPar], 4 * sizeof(float));
        }
    }
    if (newest_params || newest_estimates) {
        double last[kLastDoubles];
        CD_TRY(h, hipMemcpy(last, h->d_last, sizeof last, hipMemcpyDeviceToHost));
        if (newest_params) std::memcpy(newest_params, h->fixed ? (const void *)h->fx : (const void *)(last + 4), 4 * sizeof(float));
        if (newest_estimates) std::memcpy(newest_estimates, last, 4 * sizeof(double));
    }
    return LORA_HIP_OK;
}

float lora_hip_conditioner_last_kernel_ms(const lora_hip_conditioner_t *h) { return h ? h->last_ms : 0.0f; }

} // extern "C"
