// lora_filterbank.hip -- MI355X polyphase DFT filter bank: the channeliser for channels on a uniform grid (a gateway's band
// plan).  C ABI in include/lora_hip_filterbank.h; float64 model of the same steps in tools/filterbank_model.py.
//
// Row kappa is the channeliser's output (lora_channelizer.hip) at f = f0 + kappa fs / M with the same taps h:
//     y_kappa[m] = sum_n h[n] x[mD - n] e^{-j 2 pi f (mD - n) / fs},   x[n < 0] = 0.
// With n = qM + r the grid part of the oscillator, e^{-j 2 pi kappa (mD - r) / M}, no longer depends on q:
//     1. premix    x'[n] = x[n] e^{-j 2 pi f0 n / fs}
//     2. branches  v_r[m] = sum_q h[qM + r] x'[mD - qM - r]                    (h zero-padded to Q M taps)
//     3. DFT       y_kappa[m] = sum_s e^{-j 2 pi kappa s / M} v_{(mD - s) mod M}[m]
// Step 3's cyclic shift by mD mod M is integer arithmetic on the absolute sample index (int64), so the grid part never drifts.
//
// Kernel (pfb_kernel), one launch per call.  A workgroup (8 waves) takes T consecutive output times:
//   * stages the tile's input span, (T-1) D + QM items, into LDS, premixed: x[n] * W[i] with W[i] = e^{-j 2 pi f0 i / fs}
//     for the offset i inside the tile (evaluated in double, then sincospif); the tile's base phasor e^{-j 2 pi f0 n0 / fs}
//     is evaluated in double and applied to the OUTPUTS (everything after the premix is linear), as in fir_mix_kernel;
//   * walks the tile in chunks of Cw (<= 64) outputs, G chunks at a time.  Branch phase: a wave takes one (branch r, chunk)
//     task, a lane one output time; the taps h[qM + r] are wave-uniform scalar loads, the samples one ds_read_b64 each
//     (lane stride D, spread over the banks by one padding slot per 16 samples).  The branch sum is stored already
//     shifted, at u[(mD - r) mod M], so the DFT reads every branch at the same index in every lane;
//   * DFT phase: a wave takes CB = 8 selected channels of one chunk: per s one conflict-free LDS read and 8 complex
//     products with scalar twiddles tw[s][c] = e^{-j 2 pi kappa_c s / M} from a table built on the host; rows are written
//     coalesced (64 consecutive outputs of one row per wave-instruction).
// The work is small (per input sample about 4 QM / D + 8 M n_sel / D flop) and shared by every channel; the design is in
// DESIGN.md 4.10.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lora_hip_filterbank.h"
#include "lora_iq.h"

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kCB = 8;                        // selected channels per DFT task
constexpr size_t kLdsMax = 160u * 1024u;      // LDS per CU (gfx950)
constexpr long long kTargetTileIn = 4096;     // input items a tile advances, at least (halo re-reads: (QM - 1) / this)

// the channeliser's design (lora_channelizer.hip, firdes_low_pass): firdes::low_pass(gain, fs, cutoff, transition, WIN_HAMMING)
std::vector<float> pfb_low_pass(double gain, double fs, double cutoff, double transition)
{
    int ntaps = (int)(53.0 * fs / (22.0 * transition));
    if ((ntaps & 1) == 0) ntaps++;
    const int M = (ntaps - 1) / 2;
    const double fwT0 = 2.0 * M_PI * cutoff / fs;
    std::vector<float> taps(ntaps);
    std::vector<float> w(ntaps);
    for (int n = 0; n < ntaps; n++) w[n] = (float)(0.54 - 0.46 * std::cos(2.0 * M_PI * n / (ntaps - 1)));
    for (int n = -M; n <= M; n++) {
        if (n == 0) taps[n + M] = (float)(fwT0 / M_PI * w[n + M]);
        else taps[n + M] = (float)(std::sin(n * fwT0) / (n * M_PI) * w[n + M]);
    }
    double fmax = taps[M];
    for (int n = 1; n <= M; n++) fmax += 2.0 * taps[n + M];
    const double g = gain / fmax;
    for (int n = 0; n < ntaps; n++) taps[n] = (float)(taps[n] * g);
    return taps;
}

struct PfbArgs {
    const float2 *in;      // new input items (pfb_kernel<., F>: of format F, aligned to its component)
    const float2 *hist;    // the nhist items before in[0]
    float2 *out;           // n_sel rows of out_stride
    double tps;            // f0 / fs (turns per sample)
    long long n_abs;       // absolute index of in[0]
    long long n_in;
    long long first;       // local index of the first output's newest input (decimation phase)
    long long n_out;
    long long out_stride;
    int M, Q, D;           // grid size, taps per branch, decimation
    int nhist;             // items in hist (= real tap count - 1)
    int n_sel, cpad;       // selected channels; twiddle row length (n_sel rounded up to kCB)
    int base_mod;          // (n_abs + first) mod M: the grid rotator's shift of output 0
    int cw, g, nc;         // outputs per chunk (<= 64), chunks per phase, chunks per tile (a multiple of g)
    int xs_slots;          // LDS slots of the staged span
    float scale;           // integer formats: the conversion's scale (lora_iq.h)
};

static_assert(LORA_HIP_FILTERBANK_MAX_DST * kCB <= 64, "run_device_rows: one lane per (destination, row of a channel group)");
typedef __attribute__((address_space(1))) unsigned long long pfb_gu64; // (global stores for run_device_rows' destinations)

__device__ __host__ __forceinline__ int pfb_slot(int i) { return i + (i >> 4); }

__device__ __forceinline__ float2 pfb_cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// kRows = false (run_device): row r at A.out + r A.out_stride.  kRows = true (run_device_rows): A.out is a device table of
// n_dst * n_sel row base pointers (float2 *) and A.out_stride is n_dst; each output goes to rows[d n_sel + r] for every d,
// the same value from the same registers.
// F = the format of A.in (lora_hip_iq_format): the staging load converts an integer item, rounded to fp32 before the premix; the
// history is always cf32.  Nothing else depends on F.
template <bool kRows, int F>
__global__ __launch_bounds__(kThreads) void pfb_kernel(PfbArgs A, const float *__restrict__ taps, const float2 *__restrict__ tw)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *xs = reinterpret_cast<float2 *>(smem);            // xs[slot(i)] = x'[p0 + i] / base
    float2 *u = xs + A.xs_slots;                              // u[(gi M + s) cw + lane]: shifted branch sums of G chunks
    const int M = A.M, Q = A.Q, D = A.D, L = Q * M, cw = A.cw;
    const int T = cw * A.nc;
    const long long m_tile = (long long)blockIdx.x * T;
    const long long p0 = A.first + m_tile * D - (L - 1);     // local input index of xs[0]
    const int span = (T - 1) * D + L;
    for (int i = threadIdx.x; i < span; i += kThreads) {
        const long long n = p0 + i;
        float2 v = make_float2(0.f, 0.f);
        if (n >= 0) {
            if (n < A.n_in) {
                if constexpr (F == LORA_HIP_IQ_CF32) v = A.in[n];
                else v = lora_iq::load<F>(A.in, n, A.scale);
            }
        }
        else if (n >= -(long long)A.nhist) v = A.hist[A.nhist + n];
        const double t = A.tps * (double)i;
        float s, c;
        sincospif(-2.0f * (float)(t - floor(t)), &s, &c);
        xs[pfb_slot(i)] = pfb_cmul(v, make_float2(c, s));
    }
    float2 base; // e^{-j 2 pi f0 (n_abs + p0) / fs}, in double
    {
        const double turns = A.tps * (double)(A.n_abs + p0);
        double s, c;
        sincospi(-2.0 * (turns - floor(turns)), &s, &c);
        base = make_float2((float)c, (float)s);
    }
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const bool act = lane < cw;
    const int n_cg = A.cpad / kCB;
    const int n_dst = kRows ? (int)A.out_stride : 0;
    __syncthreads();
    for (int k0 = 0; k0 < A.nc; k0 += A.g) {
        // branch phase: tasks (r, gi) over the waves
        for (int task = wave; task < M * A.g; task += kWaves) {
            const int r = task % M, gi = task / M;
            const int j = (k0 + gi) * cw + lane;              // output inside the tile
            if (act) {
                const int i0 = (L - 1) + j * D - r;           // xs index of x'[mD - r]
                float2 a0 = make_float2(0.f, 0.f), a1 = make_float2(0.f, 0.f);
                int q = 0;
#pragma unroll 2
                for (; q + 1 < Q; q += 2) {
                    const float h0 = taps[q * M + r], h1 = taps[(q + 1) * M + r];
                    const float2 v0 = xs[pfb_slot(i0 - q * M)], v1 = xs[pfb_slot(i0 - (q + 1) * M)];
                    a0.x = fmaf(h0, v0.x, a0.x); a0.y = fmaf(h0, v0.y, a0.y);
                    a1.x = fmaf(h1, v1.x, a1.x); a1.y = fmaf(h1, v1.y, a1.y);
                }
                if (q < Q) {
                    const float h0 = taps[q * M + r];
                    const float2 v0 = xs[pfb_slot(i0 - q * M)];
                    a0.x = fmaf(h0, v0.x, a0.x); a0.y = fmaf(h0, v0.y, a0.y);
                }
                // output m = m_tile + j sits at absolute input index n_abs + first + m D: shift (base_mod + m D) mod M
                const long long m = m_tile + j;
                int s = (int)((A.base_mod + (m % M) * (long long)(D % M)) % M) - r;
                if (s < 0) s += M;
                u[(gi * M + s) * cw + lane] = make_float2(a0.x + a1.x, a0.y + a1.y);
            }
        }
        __syncthreads();
        // DFT phase: tasks (channel group, gi) over the waves
        for (int task = wave; task < n_cg * A.g; task += kWaves) {
            const int cg = task % n_cg, gi = task / n_cg;
            unsigned long long mine = 0; // rows mode: lane l holds row cg kCB + (l % kCB) of destination l / kCB (read back per store)
            if constexpr (kRows) {
                const int rd = lane / kCB, rc = cg * kCB + lane % kCB;
                if (rd < n_dst && rc < A.n_sel) mine = reinterpret_cast<const unsigned long long *>(A.out)[(size_t)rd * A.n_sel + rc];
            }
            if (act) {
                float2 acc[kCB];
#pragma unroll
                for (int c = 0; c < kCB; c++) acc[c] = make_float2(0.f, 0.f);
                const float2 *__restrict__ ur = u + gi * M * cw + lane;
                const float2 *__restrict__ twg = tw + cg * kCB;
                for (int s = 0; s < M; s++) {
                    const float2 v = ur[s * cw];
#pragma unroll
                    for (int c = 0; c < kCB; c++) {
                        const float2 w = twg[s * A.cpad + c];
                        acc[c].x = fmaf(w.x, v.x, acc[c].x); acc[c].x = fmaf(-w.y, v.y, acc[c].x);
                        acc[c].y = fmaf(w.x, v.y, acc[c].y); acc[c].y = fmaf(w.y, v.x, acc[c].y);
                    }
                }
                const long long m = m_tile + (long long)(k0 + gi) * cw + lane;
                if (m < A.n_out) {
#pragma unroll
                    for (int c = 0; c < kCB; c++) {
                        const int row = cg * kCB + c;
                        if (row < A.n_sel) {
                            if constexpr (kRows) {
                                const float2 y = pfb_cmul(acc[c], base);
                                for (int d = 0; d < n_dst; d++) {
                                    const unsigned long long p = (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)mine, d * kCB + c) |
                                                                 (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(mine >> 32), d * kCB + c) << 32;
                                    reinterpret_cast<pfb_gu64 *>(p)[m] = __builtin_bit_cast(unsigned long long, y);
                                }
                            } else {
                                A.out[(size_t)row * A.out_stride + m] = pfb_cmul(acc[c], base);
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
}

size_t pfb_lds_bytes(int M, int D, int L, int cw, int g, int nc)
{
    const int span = (cw * nc - 1) * D + L;
    return ((size_t)pfb_slot(span - 1) + 1 + (size_t)g * M * cw) * sizeof(float2);
}

} // namespace

struct lora_hip_filterbank {
    lora_hip_filterbank_config_t cfg{};
    std::vector<int32_t> channels;
    std::vector<float> taps;       // the channeliser's d_lpf
    int M = 0, Q = 0, D = 0;
    int cw = 64, g = 1, nc = 1, cpad = 0, xs_slots = 0;
    size_t lds = 0;
    int device = 0;
    long long n_abs = 0;           // input items consumed so far
    float *d_taps = nullptr;
    float2 *d_tw = nullptr, *d_hist = nullptr, *d_hist2 = nullptr, *d_stage_in = nullptr, *d_stage_out = nullptr;
    float2 **d_rows = nullptr;     // run_device_rows' pointer table (LORA_HIP_FILTERBANK_MAX_DST * n_channels entries)
    std::vector<float2 *> rows;    // ... and its host copy (alive until the upload is done)
    size_t stage_in_cap = 0, stage_out_cap = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_ms = 0.0f;
    std::string err;
};

namespace {

lora_hip_status ffail(lora_hip_filterbank *h, lora_hip_status s, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    return s;
}
#define FB_TRY(h, call)                                                                                    \
    do {                                                                                                   \
        hipError_t e_ = (call);                                                                            \
        if (e_ != hipSuccess) return ffail((h), LORA_HIP_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// Tile shape: G chunks per phase so that the M G branch tasks spread evenly over the 8 waves; chunks of cw <= 64 outputs, as
// wide as the LDS allows; nc chunks per tile, enough that a tile advances kTargetTileIn input items where the LDS allows.
bool pfb_plan(lora_hip_filterbank *h)
{
    const int M = h->M, D = h->D, L = h->Q * h->M;
    int g = 1;
    while (g < 16 && (M * g) % kWaves != 0 && M * g < 4 * kWaves) g++;
    int cw = 64;
    while (cw > 1 && pfb_lds_bytes(M, D, L, cw, g, g) > kLdsMax) cw /= 2;
    while (g > 1 && pfb_lds_bytes(M, D, L, cw, g, g) > kLdsMax) g--;
    if (pfb_lds_bytes(M, D, L, cw, g, g) > kLdsMax) return false;
    int nc = g;
    while (nc < 64 * g && (long long)cw * nc * D < std::max<long long>(kTargetTileIn, 4ll * L) &&
           pfb_lds_bytes(M, D, L, cw, g, nc + g) <= kLdsMax)
        nc += g;
    h->cw = cw; h->g = g; h->nc = nc;
    h->xs_slots = pfb_slot((cw * nc - 1) * D + L - 1) + 1;
    h->lds = pfb_lds_bytes(M, D, L, cw, g, nc);
    return true;
}

template <bool kRows, int F>
hipError_t pfb_launch_as(unsigned tiles, size_t lds, hipStream_t st, const PfbArgs &a, const float *taps, const float2 *tw)
{
    hipLaunchKernelGGL((pfb_kernel<kRows, F>), dim3(tiles), dim3(kThreads), lds, st, a, taps, tw);
    return hipGetLastError();
}

template <bool kRows>
hipError_t pfb_launch(int fmt, unsigned tiles, size_t lds, hipStream_t st, const PfbArgs &a, const float *taps, const float2 *tw)
{
    switch (fmt) {
    case LORA_HIP_IQ_SC16: return pfb_launch_as<kRows, LORA_HIP_IQ_SC16>(tiles, lds, st, a, taps, tw);
    case LORA_HIP_IQ_SC8: return pfb_launch_as<kRows, LORA_HIP_IQ_SC8>(tiles, lds, st, a, taps, tw);
    case LORA_HIP_IQ_CU8: return pfb_launch_as<kRows, LORA_HIP_IQ_CU8>(tiles, lds, st, a, taps, tw);
    default: return pfb_launch_as<kRows, LORA_HIP_IQ_CF32>(tiles, lds, st, a, taps, tw);
    }
}

template <bool kRows, int F>
bool pfb_allow_lds()
{
    return hipFuncSetAttribute((const void *)pfb_kernel<kRows, F>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax) == hipSuccess;
}

template <bool kRows>
bool pfb_allow_lds_all()
{
    return pfb_allow_lds<kRows, LORA_HIP_IQ_CF32>() && pfb_allow_lds<kRows, LORA_HIP_IQ_SC16>() && pfb_allow_lds<kRows, LORA_HIP_IQ_SC8>() &&
           pfb_allow_lds<kRows, LORA_HIP_IQ_CU8>();
}

// integer input: the next call's history is the last nh items of (history, input), the input converted - on the device for any n_in
lora_hip_status pfb_hist_raw(lora_hip_filterbank *h, const void *d_in, size_t n_in, int fmt, float scale, hipStream_t st)
{
    const size_t nh = h->taps.size() - 1, ib = lora_iq::item_bytes(fmt);
    if (!nh || !n_in) return LORA_HIP_OK;
    if (n_in >= nh) {
        FB_TRY(h, lora_iq::unpack_launch((const unsigned char *)d_in + (n_in - nh) * ib, nh, fmt, scale, h->d_hist, st));
    } else {
        const size_t keep = nh - n_in;
        FB_TRY(h, hipMemcpyAsync(h->d_hist2, h->d_hist + n_in, keep * sizeof(float2), hipMemcpyDeviceToDevice, st));
        FB_TRY(h, lora_iq::unpack_launch(d_in, n_in, fmt, scale, h->d_hist2 + keep, st));
        std::swap(h->d_hist, h->d_hist2);
    }
    return LORA_HIP_OK;
}

lora_hip_status fb_run_device(lora_hip_filterbank_t *h, const void *d_in, size_t n_in, int fmt, float scale, void *d_out, size_t out_stride, size_t *n_out,
                              void *hip_stream);
lora_hip_status fb_run_device_rows(lora_hip_filterbank_t *h, const void *d_in, size_t n_in, int fmt, float scale, void *const *row_ptrs, uint32_t n_dst,
                                   size_t max_out, size_t *n_out, void *hip_stream);
lora_hip_status fb_work(lora_hip_filterbank_t *h, const void *in, size_t n_in, int fmt, float scale, float *out, size_t out_stride, size_t *n_out);

// the raw entry points' own checks (include/lora_hip.h, lora_hip_iq_format)
lora_hip_status fb_check_raw(lora_hip_filterbank *h, const void *p, int fmt, float scale)
{
    if (!h) return LORA_HIP_ERR_ARG;
    if (!lora_iq::args_ok(p, fmt, scale)) return ffail(h, LORA_HIP_ERR_ARG, "unknown format %d, unusable scale %g, or input not aligned to its component", fmt, (double)scale);
    return LORA_HIP_OK;
}

} // namespace

extern "C" {

lora_hip_status lora_hip_filterbank_create(const lora_hip_filterbank_config_t *cfg, lora_hip_filterbank_t **out)
{
    if (!cfg || !out || cfg->struct_size < sizeof(lora_hip_filterbank_config_t)) return LORA_HIP_ERR_ARG;
    *out = nullptr;
    if (!cfg->channels) return LORA_HIP_ERR_ARG;
    const uint32_t M = cfg->n_grid;
    if (M < 1 || M > LORA_HIP_FILTERBANK_MAX_GRID || cfg->decimation < 1 || cfg->decimation > LORA_HIP_FILTERBANK_MAX_DECIMATION ||
        cfg->n_channels < 1 || cfg->n_channels > M || !(cfg->samp_rate > 0.0) || !std::isfinite(cfg->samp_rate) ||
        !std::isfinite(cfg->grid_offset_hz) || cfg->flags != 0 || cfg->cutoff_hz < 0.0f || cfg->transition_hz < 0.0f)
        return LORA_HIP_ERR_BAD_CONFIG;
    const int lo = -(int)(M / 2), hi = (int)((M + 1) / 2) - 1;
    std::vector<char> seen(M, 0);
    for (uint32_t c = 0; c < cfg->n_channels; c++) {
        const int32_t k = cfg->channels[c];
        if (k < lo || k > hi || seen[(size_t)(k - lo)]) return LORA_HIP_ERR_BAD_CONFIG;
        seen[(size_t)(k - lo)] = 1;
    }
    const double cutoff = cfg->cutoff_hz > 0.0f ? (double)cfg->cutoff_hz : (double)(cfg->bandwidth / 2u) + 15000.0;
    const double transition = cfg->transition_hz > 0.0f ? (double)cfg->transition_hz : 10000.0;
    const double ntaps = 53.0 * cfg->samp_rate / (22.0 * transition);
    if (!(ntaps >= 2.0) || ntaps >= (double)LORA_HIP_FILTERBANK_MAX_TAPS) return LORA_HIP_ERR_BAD_CONFIG; // (below 2: one tap, its window 0 / 0)
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev) return LORA_HIP_ERR_NO_DEVICE;
    auto *h = new lora_hip_filterbank;
    h->cfg = *cfg;
    h->cfg.channels = nullptr;
    h->channels.assign(cfg->channels, cfg->channels + cfg->n_channels);
    h->device = cfg->device;
    h->taps = pfb_low_pass(1.0, cfg->samp_rate, cutoff, transition);
    h->M = (int)M;
    h->D = (int)cfg->decimation;
    h->Q = ((int)h->taps.size() + h->M - 1) / h->M;
    if (!pfb_plan(h)) { delete h; return LORA_HIP_ERR_BAD_CONFIG; }
    const int L = h->Q * h->M;
    std::vector<float> padded(h->taps);
    padded.resize((size_t)L, 0.0f);
    const int nsel = (int)h->channels.size();
    h->cpad = (nsel + kCB - 1) / kCB * kCB;
    std::vector<float2> tw((size_t)M * h->cpad, make_float2(0.f, 0.f)); // tw[s][c] = e^{-j 2 pi kappa_c s / M}, exact index kappa s mod M
    for (uint32_t s = 0; s < M; s++)
        for (int c = 0; c < nsel; c++) {
            const long long e = (((long long)h->channels[c] * s) % (long long)M + M) % M;
            const double a = -2.0 * M_PI * (double)e / (double)M;
            tw[(size_t)s * h->cpad + c] = make_float2((float)std::cos(a), (float)std::sin(a));
        }
    const size_t nh = h->taps.size() - 1;
    lora_hip_status st = LORA_HIP_OK;
    do {
        if (hipSetDevice(h->device) != hipSuccess) { st = LORA_HIP_ERR_NO_DEVICE; break; }
        if (hipMalloc((void **)&h->d_taps, (size_t)L * sizeof(float)) != hipSuccess ||
            hipMalloc((void **)&h->d_tw, tw.size() * sizeof(float2)) != hipSuccess ||
            hipMalloc((void **)&h->d_hist, std::max<size_t>(nh, 1) * sizeof(float2)) != hipSuccess ||
            hipMalloc((void **)&h->d_hist2, std::max<size_t>(nh, 1) * sizeof(float2)) != hipSuccess ||
            hipMalloc((void **)&h->d_rows, (size_t)LORA_HIP_FILTERBANK_MAX_DST * nsel * sizeof(float2 *)) != hipSuccess ||
            hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) { st = LORA_HIP_ERR_NOMEM; break; }
        if (hipMemcpy(h->d_taps, padded.data(), (size_t)L * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(h->d_tw, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemset(h->d_hist, 0, std::max<size_t>(nh, 1) * sizeof(float2)) != hipSuccess) { st = LORA_HIP_ERR_HIP; break; }
        // one attribute for the one kernel, whatever the handle: the largest tile any handle may plan
        if (!pfb_allow_lds_all<false>() || !pfb_allow_lds_all<true>()) { st = LORA_HIP_ERR_HIP; break; }
    } while (false);
    if (st != LORA_HIP_OK) { lora_hip_filterbank_destroy(h); return st; }
    *out = h;
    return LORA_HIP_OK;
}

void lora_hip_filterbank_destroy(lora_hip_filterbank_t *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->d_taps) (void)hipFree(h->d_taps);
    if (h->d_tw) (void)hipFree(h->d_tw);
    if (h->d_hist) (void)hipFree(h->d_hist);
    if (h->d_hist2) (void)hipFree(h->d_hist2);
    if (h->d_rows) (void)hipFree(h->d_rows);
    if (h->d_stage_in) (void)hipFree(h->d_stage_in);
    if (h->d_stage_out) (void)hipFree(h->d_stage_out);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    delete h;
}

const char *lora_hip_filterbank_last_error(const lora_hip_filterbank_t *h) { return h ? h->err.c_str() : "null handle"; }

lora_hip_status lora_hip_filterbank_taps(const lora_hip_filterbank_t *h, float *taps, size_t cap, size_t *n)
{
    if (!h || !n) return LORA_HIP_ERR_ARG;
    *n = h->taps.size();
    if (!taps) return LORA_HIP_OK;
    if (cap < h->taps.size()) return LORA_HIP_ERR_OVERFLOW;
    std::memcpy(taps, h->taps.data(), h->taps.size() * sizeof(float));
    return LORA_HIP_OK;
}

size_t lora_hip_filterbank_output_items(const lora_hip_filterbank_t *h, size_t n_in)
{
    if (!h) return 0;
    const long long D = h->D;
    const long long first = (D - (h->n_abs % D)) % D; // outputs sit at absolute input indices that are multiples of D
    return (long long)n_in > first ? (size_t)(((long long)n_in - first + D - 1) / D) : 0;
}

lora_hip_status lora_hip_filterbank_run_device(lora_hip_filterbank_t *h, const void *d_in, size_t n_in, void *d_out,
                                               size_t out_stride, size_t *n_out, void *hip_stream)
{
    return fb_run_device(h, d_in, n_in, LORA_HIP_IQ_CF32, 0.0f, d_out, out_stride, n_out, hip_stream);
}

lora_hip_status lora_hip_filterbank_run_device_raw(lora_hip_filterbank_t *h, const void *d_in, size_t n_in, int fmt, float scale, void *d_out,
                                                   size_t out_stride, size_t *n_out, void *hip_stream)
{
    const lora_hip_status s = fb_check_raw(h, d_in, fmt, scale);
    return s != LORA_HIP_OK ? s : fb_run_device(h, d_in, n_in, fmt, scale, d_out, out_stride, n_out, hip_stream);
}

lora_hip_status lora_hip_filterbank_run_device_rows(lora_hip_filterbank_t *h, const void *d_in, size_t n_in, void *const *row_ptrs, uint32_t n_dst,
                                                    size_t max_out, size_t *n_out, void *hip_stream)
{
    return fb_run_device_rows(h, d_in, n_in, LORA_HIP_IQ_CF32, 0.0f, row_ptrs, n_dst, max_out, n_out, hip_stream);
}

lora_hip_status lora_hip_filterbank_run_device_rows_raw(lora_hip_filterbank_t *h, const void *d_in, size_t n_in, int fmt, float scale,
                                                        void *const *row_ptrs, uint32_t n_dst, size_t max_out, size_t *n_out, void *hip_stream)
{
    const lora_hip_status s = fb_check_raw(h, d_in, fmt, scale);
    return s != LORA_HIP_OK ? s : fb_run_device_rows(h, d_in, n_in, fmt, scale, row_ptrs, n_dst, max_out, n_out, hip_stream);
}

lora_hip_status lora_hip_filterbank_work(lora_hip_filterbank_t *h, const float *in, size_t n_in, float *out, size_t out_stride, size_t *n_out)
{
    return fb_work(h, in, n_in, LORA_HIP_IQ_CF32, 0.0f, out, out_stride, n_out);
}

lora_hip_status lora_hip_filterbank_work_raw(lora_hip_filterbank_t *h, const void *in, size_t n_in, int fmt, float scale, float *out, size_t out_stride,
                                             size_t *n_out)
{
    const lora_hip_status s = fb_check_raw(h, in, fmt, scale);
    return s != LORA_HIP_OK ? s : fb_work(h, in, n_in, fmt, scale, out, out_stride, n_out);
}

lora_hip_status lora_hip_filterbank_get_plan(const lora_hip_filterbank_t *h, uint32_t *cw, uint32_t *g, uint32_t *nc, uint32_t *q, size_t *lds_bytes)
{
    if (!h) return LORA_HIP_ERR_ARG;
    if (cw) *cw = (uint32_t)h->cw;
    if (g) *g = (uint32_t)h->g;
    if (nc) *nc = (uint32_t)h->nc;
    if (q) *q = (uint32_t)h->Q;
    if (lds_bytes) *lds_bytes = h->lds;
    return LORA_HIP_OK;
}

float lora_hip_filterbank_last_kernel_ms(const lora_hip_filterbank_t *h) { return h ? h->last_ms : 0.0f; }

} // extern "C"

namespace {

lora_hip_status fb_run_device(lora_hip_filterbank_t *h, const void *d_in, size_t n_in, int fmt, float scale, void *d_out, size_t out_stride, size_t *n_out,
                              void *hip_stream)
{
    if (!h || !n_out || (n_in && (!d_in || !d_out))) return LORA_HIP_ERR_ARG;
    const size_t no = lora_hip_filterbank_output_items(h, n_in);
    *n_out = no;
    if (no > out_stride) return ffail(h, LORA_HIP_ERR_OVERFLOW, "out_stride %zu < %zu output items", out_stride, no);
    hipStream_t st = (hipStream_t)hip_stream;
    FB_TRY(h, hipSetDevice(h->device));
    const int nh = (int)h->taps.size() - 1; // the history is the real tap count - 1 items (the padded taps are zero)
    const long long D = h->D, M = h->M;
    h->last_ms = 0.0f;
    if (no) {
        PfbArgs a{};
        a.in = (const float2 *)d_in; a.hist = h->d_hist; a.out = (float2 *)d_out;
        a.tps = h->cfg.grid_offset_hz / h->cfg.samp_rate;
        a.n_abs = h->n_abs; a.n_in = (long long)n_in; a.first = (D - (h->n_abs % D)) % D; a.n_out = (long long)no;
        a.out_stride = (long long)out_stride;
        a.M = h->M; a.Q = h->Q; a.D = h->D; a.nhist = nh; a.n_sel = (int)h->channels.size(); a.cpad = h->cpad;
        a.base_mod = (int)((h->n_abs + a.first) % M);
        a.cw = h->cw; a.g = h->g; a.nc = h->nc; a.xs_slots = h->xs_slots; a.scale = lora_iq::scale_of(fmt, scale);
        const long long T = (long long)h->cw * h->nc;
        const unsigned tiles = (unsigned)(((long long)no + T - 1) / T);
        FB_TRY(h, hipEventRecord(h->ev0, st));
        FB_TRY(h, pfb_launch<false>(fmt, tiles, h->lds, st, a, (const float *)h->d_taps, (const float2 *)h->d_tw));
        FB_TRY(h, hipEventRecord(h->ev1, st));
    }
    // the next call's history: the last nh input items seen so far
    if (fmt != LORA_HIP_IQ_CF32) {
        const lora_hip_status s = pfb_hist_raw(h, d_in, n_in, fmt, scale, st);
        if (s != LORA_HIP_OK) return s;
    } else if (nh > 0) {
        if (n_in >= (size_t)nh) {
            FB_TRY(h, hipMemcpyAsync(h->d_hist, (const float2 *)d_in + (n_in - (size_t)nh), (size_t)nh * sizeof(float2), hipMemcpyDeviceToDevice, st));
        } else if (n_in) {
            const size_t keep = (size_t)nh - n_in;
            std::vector<float2> tmp((size_t)nh);
            FB_TRY(h, hipStreamSynchronize(st));
            FB_TRY(h, hipMemcpy(tmp.data(), h->d_hist + n_in, keep * sizeof(float2), hipMemcpyDeviceToHost));
            FB_TRY(h, hipMemcpy(tmp.data() + keep, d_in, n_in * sizeof(float2), hipMemcpyDeviceToHost));
            FB_TRY(h, hipMemcpy(h->d_hist, tmp.data(), tmp.size() * sizeof(float2), hipMemcpyHostToDevice));
        }
    }
    FB_TRY(h, hipStreamSynchronize(st));
    if (no) FB_TRY(h, hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1));
    h->n_abs += (long long)n_in;
    return LORA_HIP_OK;
}

lora_hip_status fb_run_device_rows(lora_hip_filterbank_t *h, const void *d_in, size_t n_in, int fmt, float scale, void *const *row_ptrs, uint32_t n_dst,
                                   size_t max_out, size_t *n_out, void *hip_stream)
{
    if (!h || !n_out || (n_in && (!d_in || !row_ptrs)) || n_dst < 1 || n_dst > LORA_HIP_FILTERBANK_MAX_DST) return LORA_HIP_ERR_ARG;
    const size_t nsel = h->channels.size();
    if (n_in)
        for (size_t i = 0; i < (size_t)n_dst * nsel; i++)
            if (!row_ptrs[i] || ((uintptr_t)row_ptrs[i] & 7u)) return ffail(h, LORA_HIP_ERR_ARG, "row pointer %zu is NULL or not 8-byte aligned", i);
    const size_t no = lora_hip_filterbank_output_items(h, n_in);
    *n_out = no;
    if (no > max_out) return ffail(h, LORA_HIP_ERR_OVERFLOW, "max_out %zu < %zu output items", max_out, no);
    hipStream_t st = (hipStream_t)hip_stream;
    FB_TRY(h, hipSetDevice(h->device));
    const int nh = (int)h->taps.size() - 1;
    const long long D = h->D, M = h->M;
    h->last_ms = 0.0f;
    if (no) {
        h->rows.assign((float2 *const *)row_ptrs, (float2 *const *)row_ptrs + (size_t)n_dst * nsel);
        FB_TRY(h, hipMemcpyAsync(h->d_rows, h->rows.data(), h->rows.size() * sizeof(float2 *), hipMemcpyHostToDevice, st));
        PfbArgs a{};
        a.in = (const float2 *)d_in; a.hist = h->d_hist; a.out = (float2 *)h->d_rows;
        a.tps = h->cfg.grid_offset_hz / h->cfg.samp_rate;
        a.n_abs = h->n_abs; a.n_in = (long long)n_in; a.first = (D - (h->n_abs % D)) % D; a.n_out = (long long)no;
        a.out_stride = (long long)n_dst;
        a.M = h->M; a.Q = h->Q; a.D = h->D; a.nhist = nh; a.n_sel = (int)nsel; a.cpad = h->cpad;
        a.base_mod = (int)((h->n_abs + a.first) % M);
        a.cw = h->cw; a.g = h->g; a.nc = h->nc; a.xs_slots = h->xs_slots; a.scale = lora_iq::scale_of(fmt, scale);
        const long long T = (long long)h->cw * h->nc;
        const unsigned tiles = (unsigned)(((long long)no + T - 1) / T);
        FB_TRY(h, hipEventRecord(h->ev0, st));
        FB_TRY(h, pfb_launch<true>(fmt, tiles, h->lds, st, a, (const float *)h->d_taps, (const float2 *)h->d_tw));
        FB_TRY(h, hipEventRecord(h->ev1, st));
    }
    // the next call's history, on the device whatever n_in: the last nh items of (history, input)
    if (fmt != LORA_HIP_IQ_CF32) {
        const lora_hip_status s = pfb_hist_raw(h, d_in, n_in, fmt, scale, st);
        if (s != LORA_HIP_OK) return s;
    } else if (nh > 0 && n_in) {
        if (n_in >= (size_t)nh) {
            FB_TRY(h, hipMemcpyAsync(h->d_hist, (const float2 *)d_in + (n_in - (size_t)nh), (size_t)nh * sizeof(float2), hipMemcpyDeviceToDevice, st));
        } else {
            const size_t keep = (size_t)nh - n_in;
            FB_TRY(h, hipMemcpyAsync(h->d_hist2, h->d_hist + n_in, keep * sizeof(float2), hipMemcpyDeviceToDevice, st));
            FB_TRY(h, hipMemcpyAsync(h->d_hist2 + keep, d_in, n_in * sizeof(float2), hipMemcpyDeviceToDevice, st));
            std::swap(h->d_hist, h->d_hist2);
        }
    }
    FB_TRY(h, hipStreamSynchronize(st));
    if (no) FB_TRY(h, hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1));
    h->n_abs += (long long)n_in;
    return LORA_HIP_OK;
}

// (the staging area holds n_in items of any format: it is sized for cf32)
lora_hip_status fb_work(lora_hip_filterbank_t *h, const void *in, size_t n_in, int fmt, float scale, float *out, size_t out_stride, size_t *n_out)
{
    if (!h || !n_out || (n_in && (!in || !out))) return LORA_HIP_ERR_ARG;
    const size_t no = lora_hip_filterbank_output_items(h, n_in);
    if (no > out_stride) { *n_out = no; return ffail(h, LORA_HIP_ERR_OVERFLOW, "out_stride %zu < %zu output items", out_stride, no); }
    FB_TRY(h, hipSetDevice(h->device));
    const size_t nc = h->channels.size();
    if (n_in > h->stage_in_cap) {
        if (h->d_stage_in) (void)hipFree(h->d_stage_in);
        h->d_stage_in = nullptr; h->stage_in_cap = 0;
        FB_TRY(h, hipMalloc((void **)&h->d_stage_in, (n_in + n_in / 4 + 16) * sizeof(float2)));
        h->stage_in_cap = n_in + n_in / 4 + 16;
    }
    const size_t ostride = std::max<size_t>(no, 1);
    const size_t need_out = nc * ostride;
    if (need_out > h->stage_out_cap) {
        if (h->d_stage_out) (void)hipFree(h->d_stage_out);
        h->d_stage_out = nullptr; h->stage_out_cap = 0;
        FB_TRY(h, hipMalloc((void **)&h->d_stage_out, (need_out + need_out / 4 + 16) * sizeof(float2)));
        h->stage_out_cap = need_out + need_out / 4 + 16;
    }
    if (n_in) FB_TRY(h, hipMemcpy(h->d_stage_in, in, n_in * lora_iq::item_bytes(fmt), hipMemcpyHostToDevice));
    lora_hip_status s = fb_run_device(h, h->d_stage_in, n_in, fmt, scale, h->d_stage_out, ostride, n_out, nullptr);
    if (s != LORA_HIP_OK) return s;
    if (no) FB_TRY(h, hipMemcpy2D(out, out_stride * sizeof(float2), h->d_stage_out, ostride * sizeof(float2), no * sizeof(float2), nc, hipMemcpyDeviceToHost));
    return LORA_HIP_OK;
}

} // namespace
