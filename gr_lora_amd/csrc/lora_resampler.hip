// lora_resampler.hip -- MI355X rational resampler: rate fs_in -> fs_in * L / M by a Kaiser-windowed-sinc polyphase filter.  C ABI
// and the definition in include/lora_hip_resampler.h; float64 model of the same definition in gr_lora_amd/resampler.py (resample).
//
// Kernel (rs_kernel), one launch per call.  A workgroup of T threads takes G consecutive tiles of T outputs (rs_plan):
//   * the phase table - L rows of Q taps, row p holds h[p + j L] at column j, zero where p + j L >= ntaps - is copied from
//     global memory into LDS once per workgroup (at most 70 KB; G tiles share the copy).  Every lane has its own phase, so the
//     lanes of a wavefront read column j of different rows: the row stride is Q | 1, odd, which spreads rows p .. p + 31 over
//     the 32 banks a 4-byte LDS read sees (a stride that is a multiple of 32 would put them all on one).
//   * a tile's input span, x[n0(first) - Q + 1 .. n0(last)], is staged into LDS beside the table as cf32; an integer item is
//     converted by the load (lora_iq::load<F>), an index in front of this call's first item comes from the handle's carried
//     items (cf32), an index below 0 of the stream is zero.  Every global read is guarded by n_in.
//   * thread t then runs output t's chain: re = fma(h, x.re, re), im = fma(h, x.im, im) for j = 0 .. Q - 1, from +0, written as
//     fmaf so that every instantiation rounds alike, and stores one cf32 (guarded by the output count).
// The handle's carried items are brought up to date by copies (or lora_iq's unpack) on the same stream into a second buffer,
// and the handle moves on only after everything has succeeded.  Design and measurements: DESIGN.md 4.16.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/lora_hip_resampler.h"
#include "lora_iq.h"

namespace {

constexpr size_t kLdsPreferred = 80u * 1024u;    // two workgroups per CU
constexpr size_t kLdsMax = 160u * 1024u;         // what a gfx950 workgroup can have
constexpr uint32_t kMaxTilesPerGroup = 32;

struct RsArgs {
    const void *in;        // new input items of format F
    const float2 *hist;    // the Q - 1 items before in[0] (cf32); only the last n_valid of them belong to the stream
    const float *tab;      // L rows of S floats
    float2 *out;
    long long n_in, n_out;
    long long base;        // n0 of output 0 relative to in[0] (>= 0)
    int p0;                // p of output 0
    int n_valid;
    int L, M, Q, S, T, G;
    int tab_floats;        // L * S rounded up to even: the input span starts 8-byte aligned behind it
    float scale;           // integer formats: the conversion's scale (lora_iq.h)
};

template <int F>
__global__ __launch_bounds__(256) void rs_kernel(RsArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *tab = reinterpret_cast<float *>(smem);
    float2 *xs = reinterpret_cast<float2 *>(smem + (size_t)A.tab_floats * sizeof(float));
    const int t = (int)threadIdx.x, T = A.T, L = A.L, M = A.M, Q = A.Q;
    const long long tile0 = (long long)blockIdx.x * A.G;
    for (int i = t; i < L * A.S; i += T) tab[i] = A.tab[i];
    for (int g = 0; g < A.G; g++) {
        const long long k0 = (tile0 + g) * T;               // first output of the tile
        if (k0 >= A.n_out) break;                            // (the same for every thread of the workgroup)
        const int cnt = (int)(A.n_out - k0 < T ? A.n_out - k0 : T);
        const long long t0 = A.p0 + k0 * M;
        const long long dn0 = t0 / L;
        const int pt0 = (int)(t0 - dn0 * L);
        const int span = (pt0 + (cnt - 1) * M) / L + Q;     // <= ((T - 1) M + L - 1) / L + Q, what rs_plan made room for
        const long long first = A.base + dn0 - (Q - 1);     // of the span, relative to in[0]
        __syncthreads();                                     // the previous tile has been read
        for (int i = t; i < span; i += T) {
            const long long r = first + i;
            float2 v = make_float2(0.f, 0.f);
            if (r >= 0) {
                if (r < A.n_in) v = lora_iq::load<F>(A.in, r, A.scale);
            } else if (r >= -(long long)A.n_valid) {
                v = A.hist[(Q - 1) + r];
            }
            xs[i] = v;
        }
        __syncthreads();
        if (t < cnt) {
            const int tt = pt0 + t * M;
            const int dn = tt / L;
            const float *hr = tab + (tt - dn * L) * A.S;
            const float2 *xp = xs + dn + (Q - 1);            // x[n0]; x[n0 - j] is xp[-j], down to xs[dn] >= xs[0]
            float re = 0.0f, im = 0.0f;
            for (int j = 0; j < Q; j++) {
                const float h = hr[j];
                const float2 v = xp[-j];
                re = fmaf(h, v.x, re);
                im = fmaf(h, v.y, im);
            }
            A.out[k0 + t] = make_float2(re, im);
        }
    }
}

// modified Bessel function I0 by its power series, sum_k ((x / 2)^k / k!)^2: all terms positive, summed in extended precision
double rs_i0(double x)
{
    const long double q = (long double)x * (long double)x / 4.0L;
    long double term = 1.0L, sum = 1.0L;
    for (int k = 1; k < 1000; k++) {
        term *= q / ((long double)k * (long double)k);
        sum += term;
        if (term < sum * 1e-22L) break;
    }
    return (double)sum;
}

// the prototype of the header's definition
std::vector<float> rs_design(uint32_t L, uint32_t M, uint32_t Z, double beta, double c)
{
    const uint32_t R = std::max(L, M);
    const size_t ntaps = 2 * (size_t)Z * R + 1;
    std::vector<float> h(ntaps);
    const double alpha = (double)(ntaps - 1) / 2.0, i0b = rs_i0(beta), gain = (double)L * (c / (double)R);
    for (size_t k = 0; k < ntaps; k++) {
        const double r = ((double)k - alpha) / alpha;
        const double w = rs_i0(beta * std::sqrt(1.0 - r * r)) / i0b;
        const double tt = ((double)k - (double)(Z * R)) * c / (double)R;
        const double y = M_PI * tt;
        const double s = tt == 0.0 ? 1.0 : std::sin(y) / y;
        h[k] = (float)(gain * s * w);
    }
    return h;
}

struct RsPlan {
    uint32_t T = 0, G = 0, S = 0, tab_floats = 0;
    size_t lds = 0;
};

// The tile follows from (L, M, Q): the table takes L * (Q | 1) floats and a tile of T outputs spans ((T - 1) M + L - 1) / L + Q
// input items.  T is the largest of 256, 128, 64 that leaves room for two workgroups per CU; deep decimation with a long filter
// does not fit that and takes T = 64 in whatever one workgroup can have.  G makes the table copy (L S floats) cost no more than
// the tiles' own traffic (16 bytes per output), up to 32.
bool rs_plan(uint32_t L, uint32_t M, uint32_t Q, RsPlan *pl)
{
    pl->S = Q | 1u;
    pl->tab_floats = (L * pl->S + 1u) & ~1u;
    const size_t tab_bytes = (size_t)pl->tab_floats * sizeof(float);
    auto lds_of = [&](uint32_t T) { return tab_bytes + ((size_t)((T - 1) * M + L - 1) / L + Q) * sizeof(float2); };
    pl->T = 0;
    for (uint32_t T : {256u, 128u, 64u})
        if (lds_of(T) <= kLdsPreferred) { pl->T = T; break; }
    if (!pl->T) {
        if (lds_of(64) > kLdsMax) return false;
        pl->T = 64;
    }
    pl->lds = lds_of(pl->T);
    pl->G = (uint32_t)std::min<size_t>(std::max<size_t>((tab_bytes + pl->T * 16 - 1) / (pl->T * 16), 1), kMaxTilesPerGroup);
    return true;
}

} // namespace

struct lora_hip_resampler {
    uint32_t L = 1, M = 1, Q = 1, Z = 16;
    double beta = 8.0, cutoff = 0.8;
    RsPlan plan;
    std::vector<float> taps;
    int device = 0;
    long long n_abs = 0;        // input items consumed so far
    long long n0 = 0, p = 0;    // of the next output: it needs x[n0 - Q + 1 .. n0]
    uint64_t m_abs = 0;         // outputs emitted so far
    int n_valid = 0;            // how many of the carried items belong to the stream: min(Q - 1, n_abs)
    float *d_tab = nullptr;
    float2 *d_hist = nullptr, *d_hist2 = nullptr;
    void *d_stage_in = nullptr;
    float2 *d_stage_out = nullptr;
    size_t stage_in_cap = 0, stage_out_cap = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_ms = 0.0f;
    std::string err;
};

namespace {

lora_hip_status rfail(lora_hip_resampler *h, lora_hip_status s, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    return s;
}
#define RS_TRY(h, call)                                                                                    \
    do {                                                                                                   \
        hipError_t e_ = (call);                                                                            \
        if (e_ != hipSuccess) return rfail((h), LORA_HIP_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

constexpr size_t kMaxItemsPerCall = (size_t)1 << 40;

// outputs whose n0 lies among the items consumed once n_in more have arrived: every k >= 0 with (p + k M) div L < d
long long rs_count(const lora_hip_resampler *h, long long n_in)
{
    const long long d = h->n_abs + n_in - h->n0;   // (at most n_in: n0 >= n_abs)
    return d <= 0 ? 0 : (d * h->L - h->p + h->M - 1) / h->M;
}

template <int F>
hipError_t rs_launch_as(unsigned groups, int threads, size_t lds, hipStream_t st, const RsArgs &a)
{
    hipLaunchKernelGGL((rs_kernel<F>), dim3(groups), dim3(threads), lds, st, a);
    return hipGetLastError();
}

hipError_t rs_launch(int fmt, unsigned groups, int threads, size_t lds, hipStream_t st, const RsArgs &a)
{
    switch (fmt) {
    case LORA_HIP_IQ_SC16: return rs_launch_as<LORA_HIP_IQ_SC16>(groups, threads, lds, st, a);
    case LORA_HIP_IQ_SC8: return rs_launch_as<LORA_HIP_IQ_SC8>(groups, threads, lds, st, a);
    case LORA_HIP_IQ_CU8: return rs_launch_as<LORA_HIP_IQ_CU8>(groups, threads, lds, st, a);
    default: return rs_launch_as<LORA_HIP_IQ_CF32>(groups, threads, lds, st, a);
    }
}

template <int F>
bool rs_allow_lds(size_t lds)
{
    return hipFuncSetAttribute((const void *)rs_kernel<F>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
}

lora_hip_status rs_check_raw(lora_hip_resampler *h, const void *p, int fmt, float scale)
{
    if (!h) return LORA_HIP_ERR_ARG;
    if (!lora_iq::args_ok(p, fmt, scale)) return rfail(h, LORA_HIP_ERR_ARG, "unknown format %d, unusable scale %g, or input not aligned to its component", fmt, (double)scale);
    return LORA_HIP_OK;
}

// what a call of n_in items emits, and the pointer rules of the header; no device call
lora_hip_status rs_check_run(lora_hip_resampler *h, const void *in, size_t n_in, const void *out, size_t max_out, size_t *n_out, uint64_t *first_out)
{
    if (!h || !n_out || !first_out || (n_in && !in)) return LORA_HIP_ERR_ARG;
    if (n_in > kMaxItemsPerCall) return rfail(h, LORA_HIP_ERR_ARG, "n_in %zu: at most 2^40 items per call", n_in);
    const size_t nr = (size_t)rs_count(h, (long long)n_in);
    *n_out = nr;
    *first_out = h->m_abs;
    if (nr > max_out) return rfail(h, LORA_HIP_ERR_OVERFLOW, "max_out %zu < %zu outputs", max_out, nr);
    if (nr && !out) return rfail(h, LORA_HIP_ERR_ARG, "outputs to write: out must not be NULL");
    if (((uintptr_t)out & 7u) != 0) return rfail(h, LORA_HIP_ERR_ARG, "out must be aligned to 8 bytes");
    const size_t per_group = (size_t)h->plan.T * h->plan.G;
    if ((nr + per_group - 1) / per_group > 0x7fffffffull) return rfail(h, LORA_HIP_ERR_ARG, "n_in %zu yields more than 2^31 - 1 workgroups of outputs", n_in);
    return LORA_HIP_OK;
}

lora_hip_status rs_run_device(lora_hip_resampler_t *h, const void *d_in, size_t n_in, int fmt, float scale, void *d_out, size_t max_out, size_t *n_out,
                              uint64_t *first_out, void *hip_stream)
{
    const lora_hip_status cs = rs_check_run(h, d_in, n_in, d_out, max_out, n_out, first_out);
    if (cs != LORA_HIP_OK) return cs;
    hipStream_t st = (hipStream_t)hip_stream;
    RS_TRY(h, hipSetDevice(h->device));
    const size_t nr = *n_out, keep_max = (size_t)h->Q - 1;
    h->last_ms = 0.0f;
    if (nr) {
        RsArgs a{};
        a.in = d_in; a.hist = h->d_hist; a.tab = h->d_tab; a.out = (float2 *)d_out;
        a.n_in = (long long)n_in; a.n_out = (long long)nr;
        a.base = h->n0 - h->n_abs; a.p0 = (int)h->p; a.n_valid = h->n_valid;
        a.L = (int)h->L; a.M = (int)h->M; a.Q = (int)h->Q; a.S = (int)h->plan.S; a.T = (int)h->plan.T; a.G = (int)h->plan.G;
        a.tab_floats = (int)h->plan.tab_floats;
        a.scale = lora_iq::scale_of(fmt, scale);
        const size_t per_group = (size_t)h->plan.T * h->plan.G;
        RS_TRY(h, hipEventRecord(h->ev0, st));
        RS_TRY(h, rs_launch(fmt, (unsigned)((nr + per_group - 1) / per_group), (int)h->plan.T, h->plan.lds, st, a));
        RS_TRY(h, hipEventRecord(h->ev1, st));
    }
    // the next call's carried items: the last Q - 1 of (carried, input), on the device for any n_in
    if (n_in) {
        if (n_in >= keep_max) {
            const size_t from = n_in - keep_max;
            if (fmt != LORA_HIP_IQ_CF32)
                RS_TRY(h, lora_iq::unpack_launch((const unsigned char *)d_in + from * lora_iq::item_bytes(fmt), keep_max, fmt, scale, h->d_hist2, st));
            else
                RS_TRY(h, hipMemcpyAsync(h->d_hist2, (const float2 *)d_in + from, keep_max * sizeof(float2), hipMemcpyDeviceToDevice, st));
        } else {
            const size_t keep = keep_max - n_in;   // the newest carried items shift to the front
            RS_TRY(h, hipMemcpyAsync(h->d_hist2, h->d_hist + n_in, keep * sizeof(float2), hipMemcpyDeviceToDevice, st));
            if (fmt != LORA_HIP_IQ_CF32)
                RS_TRY(h, lora_iq::unpack_launch(d_in, n_in, fmt, scale, h->d_hist2 + keep, st));
            else
                RS_TRY(h, hipMemcpyAsync(h->d_hist2 + keep, d_in, n_in * sizeof(float2), hipMemcpyDeviceToDevice, st));
        }
    }
    RS_TRY(h, hipStreamSynchronize(st));
    if (nr) RS_TRY(h, hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1));
    // every fallible call is behind us: the handle moves on in one piece
    if (n_in) std::swap(h->d_hist, h->d_hist2);
    h->n_valid = (int)std::min<long long>((long long)keep_max, (long long)h->n_valid + (long long)n_in);
    const long long adv = h->p + (long long)nr * h->M;   // (nr M < 2^59)
    h->n0 += adv / h->L;
    h->p = adv % h->L;
    h->m_abs += nr;
    h->n_abs += (long long)n_in;
    return LORA_HIP_OK;
}

// (the staging area holds n_in items of any format: it is sized for cf32)
lora_hip_status rs_work(lora_hip_resampler_t *h, const void *in, size_t n_in, int fmt, float scale, float *out, size_t max_out, size_t *n_out, uint64_t *first_out)
{
    const lora_hip_status cs = rs_check_run(h, in, n_in, out, max_out, n_out, first_out);
    if (cs != LORA_HIP_OK) return cs;
    RS_TRY(h, hipSetDevice(h->device));
    const size_t nr = *n_out;
    if (n_in > h->stage_in_cap) {
        if (h->d_stage_in) (void)hipFree(h->d_stage_in);
        h->d_stage_in = nullptr; h->stage_in_cap = 0;
        RS_TRY(h, hipMalloc(&h->d_stage_in, (n_in + n_in / 4 + 16) * sizeof(float2)));
        h->stage_in_cap = n_in + n_in / 4 + 16;
    }
    if (nr > h->stage_out_cap) {
        if (h->d_stage_out) (void)hipFree(h->d_stage_out);
        h->d_stage_out = nullptr; h->stage_out_cap = 0;
        RS_TRY(h, hipMalloc((void **)&h->d_stage_out, (nr + nr / 4 + 16) * sizeof(float2)));
        h->stage_out_cap = nr + nr / 4 + 16;
    }
    if (n_in) RS_TRY(h, hipMemcpy(h->d_stage_in, in, n_in * lora_iq::item_bytes(fmt), hipMemcpyHostToDevice));
    const lora_hip_status s = rs_run_device(h, h->d_stage_in, n_in, fmt, scale, h->d_stage_out, nr, n_out, first_out, nullptr);
    if (s != LORA_HIP_OK) return s;
    if (nr) RS_TRY(h, hipMemcpy(out, h->d_stage_out, nr * sizeof(float2), hipMemcpyDeviceToHost));
    return LORA_HIP_OK;
}

} // namespace

extern "C" {

lora_hip_status lora_hip_resampler_create(const lora_hip_resampler_config_t *cfg, lora_hip_resampler_t **out)
{
    if (!cfg || !out || cfg->struct_size < sizeof(lora_hip_resampler_config_t)) return LORA_HIP_ERR_ARG;
    *out = nullptr;
    const uint32_t Z = cfg->zero_crossings ? cfg->zero_crossings : 16u;
    const double beta = cfg->beta == 0.0 ? 8.0 : cfg->beta;
    const double c = cfg->cutoff;
    if (cfg->interpolation < 1 || cfg->interpolation > LORA_HIP_RESAMPLER_MAX_RATIO || cfg->decimation < 1 || cfg->decimation > LORA_HIP_RESAMPLER_MAX_RATIO ||
        Z < LORA_HIP_RESAMPLER_MIN_ZERO_CROSSINGS || Z > LORA_HIP_RESAMPLER_MAX_ZERO_CROSSINGS || !(beta >= 0.0 && beta <= (double)LORA_HIP_RESAMPLER_MAX_BETA) ||
        !(c > 0.0 && c <= 1.0) || cfg->flags != 0)
        return LORA_HIP_ERR_BAD_CONFIG;
    const uint32_t g = std::gcd(cfg->interpolation, cfg->decimation);
    const uint32_t L = cfg->interpolation / g, M = cfg->decimation / g, R = std::max(L, M);
    const size_t ntaps = 2 * (size_t)Z * R + 1;
    const size_t Q = (ntaps + L - 1) / L;
    RsPlan plan;
    if (ntaps > LORA_HIP_RESAMPLER_MAX_TAPS || Q > LORA_HIP_RESAMPLER_MAX_Q || !rs_plan(L, M, (uint32_t)Q, &plan)) return LORA_HIP_ERR_BAD_CONFIG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev) return LORA_HIP_ERR_NO_DEVICE;
    auto *h = new lora_hip_resampler;
    h->L = L; h->M = M; h->Q = (uint32_t)Q; h->Z = Z; h->beta = beta; h->cutoff = c;
    h->plan = plan;
    h->device = cfg->device;
    h->taps = rs_design(L, M, Z, beta, c);
    std::vector<float> tab((size_t)plan.tab_floats, 0.0f);
    for (uint32_t p = 0; p < L; p++)
        for (uint32_t j = 0; j < Q; j++)
            if ((size_t)p + (size_t)j * L < ntaps) tab[(size_t)p * plan.S + j] = h->taps[(size_t)p + (size_t)j * L];
    lora_hip_status st = LORA_HIP_OK;
    do {
        if (hipSetDevice(h->device) != hipSuccess) { st = LORA_HIP_ERR_NO_DEVICE; break; }
        if (hipMalloc((void **)&h->d_tab, tab.size() * sizeof(float)) != hipSuccess || hipMalloc((void **)&h->d_hist, Q * sizeof(float2)) != hipSuccess ||
            hipMalloc((void **)&h->d_hist2, Q * sizeof(float2)) != hipSuccess || hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) {
            st = LORA_HIP_ERR_NOMEM; break;
        }
        if (hipMemcpy(h->d_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemset(h->d_hist, 0, Q * sizeof(float2)) != hipSuccess || hipMemset(h->d_hist2, 0, Q * sizeof(float2)) != hipSuccess) { st = LORA_HIP_ERR_HIP; break; }
        // one attribute for the one kernel, whatever the handle
        if (!rs_allow_lds<LORA_HIP_IQ_CF32>(kLdsMax) || !rs_allow_lds<LORA_HIP_IQ_SC16>(kLdsMax) || !rs_allow_lds<LORA_HIP_IQ_SC8>(kLdsMax) ||
            !rs_allow_lds<LORA_HIP_IQ_CU8>(kLdsMax)) { st = LORA_HIP_ERR_HIP; break; }
    } while (false);
    if (st != LORA_HIP_OK) { lora_hip_resampler_destroy(h); return st; }
    *out = h;
    return LORA_HIP_OK;
}

void lora_hip_resampler_destroy(lora_hip_resampler_t *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->d_tab) (void)hipFree(h->d_tab);
    if (h->d_hist) (void)hipFree(h->d_hist);
    if (h->d_hist2) (void)hipFree(h->d_hist2);
    if (h->d_stage_in) (void)hipFree(h->d_stage_in);
    if (h->d_stage_out) (void)hipFree(h->d_stage_out);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    delete h;
}

const char *lora_hip_resampler_last_error(const lora_hip_resampler_t *h) { return h ? h->err.c_str() : "null handle"; }

lora_hip_status lora_hip_resampler_taps(const lora_hip_resampler_t *h, float *taps, size_t cap, size_t *n)
{
    if (!h || !n) return LORA_HIP_ERR_ARG;
    *n = h->taps.size();
    if (!taps) return LORA_HIP_OK;
    if (cap < h->taps.size()) return LORA_HIP_ERR_OVERFLOW;
    std::memcpy(taps, h->taps.data(), h->taps.size() * sizeof(float));
    return LORA_HIP_OK;
}

lora_hip_status lora_hip_resampler_ratio(const lora_hip_resampler_t *h, uint32_t *interpolation, uint32_t *decimation, uint32_t *q)
{
    if (!h) return LORA_HIP_ERR_ARG;
    if (interpolation) *interpolation = h->L;
    if (decimation) *decimation = h->M;
    if (q) *q = h->Q;
    return LORA_HIP_OK;
}

double lora_hip_resampler_delay(const lora_hip_resampler_t *h) { return h ? (double)h->Z * (double)std::max(h->L, h->M) / (double)h->M : 0.0; }

lora_hip_status lora_hip_resampler_get_plan(const lora_hip_resampler_t *h, uint32_t *tile, uint32_t *tiles_per_group, uint32_t *row_stride, size_t *lds_bytes)
{
    if (!h) return LORA_HIP_ERR_ARG;
    if (tile) *tile = h->plan.T;
    if (tiles_per_group) *tiles_per_group = h->plan.G;
    if (row_stride) *row_stride = h->plan.S;
    if (lds_bytes) *lds_bytes = h->plan.lds;
    return LORA_HIP_OK;
}

size_t lora_hip_resampler_output_items(const lora_hip_resampler_t *h, size_t n_in)
{
    if (!h || n_in > kMaxItemsPerCall) return 0;
    return (size_t)rs_count(h, (long long)n_in);
}

lora_hip_status lora_hip_resampler_run_device(lora_hip_resampler_t *h, const void *d_in, size_t n_in, void *d_out, size_t max_out, size_t *n_out,
                                              uint64_t *first_out, void *hip_stream)
{
    return rs_run_device(h, d_in, n_in, LORA_HIP_IQ_CF32, 0.0f, d_out, max_out, n_out, first_out, hip_stream);
}

lora_hip_status lora_hip_resampler_run_device_raw(lora_hip_resampler_t *h, const void *d_in, size_t n_in, int fmt, float scale, void *d_out, size_t max_out,
                                                  size_t *n_out, uint64_t *first_out, void *hip_stream)
{
    const lora_hip_status s = rs_check_raw(h, d_in, fmt, scale);
    return s != LORA_HIP_OK ? s : rs_run_device(h, d_in, n_in, fmt, scale, d_out, max_out, n_out, first_out, hip_stream);
}

lora_hip_status lora_hip_resampler_work(lora_hip_resampler_t *h, const float *in, size_t n_in, float *out, size_t max_out, size_t *n_out, uint64_t *first_out)
{
    return rs_work(h, in, n_in, LORA_HIP_IQ_CF32, 0.0f, out, max_out, n_out, first_out);
}

lora_hip_status lora_hip_resampler_work_raw(lora_hip_resampler_t *h, const void *in, size_t n_in, int fmt, float scale, float *out, size_t max_out,
                                            size_t *n_out, uint64_t *first_out)
{
    const lora_hip_status s = rs_check_raw(h, in, fmt, scale);
    return s != LORA_HIP_OK ? s : rs_work(h, in, n_in, fmt, scale, out, max_out, n_out, first_out);
}

lora_hip_status lora_hip_resampler_reset(lora_hip_resampler_t *h)
{
    if (!h) return LORA_HIP_ERR_ARG;
    h->n_abs = 0; h->n0 = 0; h->p = 0; h->m_abs = 0;
    h->n_valid = 0;   // (the carried items stay where they are and are read as zeros: no device call)
    return LORA_HIP_OK;
}

float lora_hip_resampler_last_kernel_ms(const lora_hip_resampler_t *h) { return h ? h->last_ms : 0.0f; }

} // extern "C"
