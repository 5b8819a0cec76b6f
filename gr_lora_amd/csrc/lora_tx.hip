// lora_tx.hip -- the transmit side (include/lora_hip_tx.h): the frame encoder (host), the traffic synthesiser's stream handle and
// tx_kernel, which writes a wide-band capture of many concurrent emitters into device memory.
//
// tx_kernel: one launch per generate call, one workgroup per tile of kTile consecutive output items, lanes on consecutive items
// (a wave's store is 64 consecutive items: 512 B of cf32).  The host gives each tile the emitters that overlap it as a range of
// a list of descriptor indices in ascending order of addition (runs of tiles with one set share one range); descriptor and list
// are indexed by values every lane of the workgroup shares.  Per (item, emitter):
//   position in the frame -> symbol and offset in it by a reciprocal multiply in double with a one-step fix-up (exact: the
//       position is below 2^34), minding that the symbols behind the quarter downchirp start at (preamble + 4) * sps + sps / 4;
//   i = (offset + shift * D) mod sps; the chirp's phase in turns is exactly i * (i - sps) / (2 * D * sps) (synth.base_upchirp),
//       negated for a downchirp: the numerator is an integer below 2^42, reduced mod 2 * D * sps by rint / fma in double, which
//       is exact integer arithmetic at these sizes;
//   the oscillator's turn is frac(f / fs * m) in double on the absolute index m, one rounded multiply as numpy makes it;
//   the summed turn, reduced to [-1/2, 1/2], is split into an fp32 head and an fp32 tail: one sincospif of the head, the tail
//       applied as a first-order rotation (it is below 2^-25 turns), so the phasor is good to sincospif's own error;
//   acc = fma(amplitude, phasor, acc) per component.
// The order of the sum is the order of the list, whatever the tiling, and every factor is a function of (emitter, m) alone: any
// split of a capture into calls gives the same bits.  An item no emitter covers stays +0.0, +0.0.
// Noise: Philox-4x32-10 keyed by the seed, counter = the absolute index, Box-Muller on two of the four words - no state.
// Integer output (sc16 / sc8 / cu8) is packed in the same kernel's store: rint(double(x) * full_scale [+ 127.5]), clipped.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lora_hip_tx.h"
#include "lora_frame_check.h"
#include "lora_iq.h"
#include "whitening_data.inc"

namespace {

constexpr int kThreads = 256;
constexpr int kPerLane = 8;
constexpr int kTile = kThreads * kPerLane;

struct TxDesc {
    long long start, len, body; // first absolute item, items, frame position of the first symbol behind the quarter downchirp
    double tps, inv_sps, den, inv_den; // f / fs; 1 / sps; 2 * D * sps and its reciprocal
    float amp;
    int sps, D, pre;        // items per symbol, fs / bw, preamble upchirps
    int sync0, sync1;       // shifts of the two sync symbols
    unsigned shift_off;     // first of the frame's shifts (header block, then payload) in the shift arena
    int pad;
};

struct TxArgs {
    const TxDesc *desc;
    const uint2 *tile_rng;      // per tile: first entry and count in tile_emit
    const unsigned *tile_emit;  // descriptor indices, ascending
    const unsigned short *shifts;
    void *out;
    long long pos, n;           // absolute index of item 0, items
    double full_scale;
    float noise_scale;          // sigma / sqrt(2); 0 = none
    unsigned key0, key1;
};

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned k0, unsigned k1, unsigned &o0, unsigned &o1)
{
    unsigned c2 = 0u, c3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o0 = c0; o1 = c1;
}

// x * y rounded once to double.  __dmul_rn is a plain x * y to the compiler, which contracts it into an add or subtract behind it
// (v_fma_f64: the product is then never rounded); the pragma takes the contract flag off this multiply alone.
__device__ __forceinline__ double mul_rn(double x, double y)
{
#pragma clang fp contract(off)
    return x * y;
}

template <int F>
__device__ __forceinline__ void tx_store(void *out, long long idx, float2 v, double fs)
{
    if constexpr (F == LORA_HIP_IQ_CF32) {
        reinterpret_cast<float2 *>(out)[idx] = v;
    } else {
        constexpr double lo = F == LORA_HIP_IQ_SC16 ? -32768.0 : F == LORA_HIP_IQ_SC8 ? -128.0 : 0.0;
        constexpr double hi = F == LORA_HIP_IQ_SC16 ? 32767.0 : F == LORA_HIP_IQ_SC8 ? 127.0 : 255.0;
        double a = mul_rn((double)v.x, fs), b = mul_rn((double)v.y, fs);
        if constexpr (F == LORA_HIP_IQ_CU8) { a = __dadd_rn(a, 127.5); b = __dadd_rn(b, 127.5); }
        const int ia = (int)fmin(fmax(rint(a), lo), hi), ib = (int)fmin(fmax(rint(b), lo), hi);
        if constexpr (F == LORA_HIP_IQ_SC16)
            reinterpret_cast<unsigned *>(out)[idx] = ((unsigned)ia & 0xffffu) | ((unsigned)ib << 16);
        else
            reinterpret_cast<unsigned short *>(out)[idx] = (unsigned short)(((unsigned)ia & 0xffu) | (((unsigned)ib & 0xffu) << 8));
    }
}

template <int F>
__global__ __launch_bounds__(kThreads) void tx_kernel(TxArgs a)
{
    const long long t0 = (long long)blockIdx.x * kTile + threadIdx.x; // item of this lane's first sample; the others kThreads apart
    const uint2 rng = a.tile_rng[blockIdx.x];
    float2 acc[kPerLane];
#pragma unroll
    for (int j = 0; j < kPerLane; j++) acc[j] = make_float2(0.0f, 0.0f);
    for (unsigned e = 0; e < rng.y; e++) {
        const TxDesc d = a.desc[a.tile_emit[rng.x + e]];
        const long long p0 = a.pos + t0 - d.start;
#pragma unroll
        for (int j = 0; j < kPerLane; j++) {
            const long long p = p0 + j * kThreads;
            if (p < 0 || p >= d.len) continue;
            const bool body = p >= d.body;
            const long long q = body ? p - d.body : p;
            int k = (int)((double)q * d.inv_sps);
            long long r = q - (long long)k * d.sps;
            if (r < 0) { k--; r += d.sps; }
            else if (r >= d.sps) { k++; r -= d.sps; }
            int shift;
            bool down = false;
            if (body) {
                shift = a.shifts[d.shift_off + (unsigned)k];
            } else {
                down = k >= d.pre + 2;
                shift = k == d.pre ? d.sync0 : k == d.pre + 1 ? d.sync1 : 0;
            }
            int i = (int)r + shift * d.D;
            if (i >= d.sps) i -= d.sps;
            const double num = (double)i * (double)(i - d.sps);      // exact, |num| <= 2^42
            const double rem = fma(-rint(num * d.inv_den), d.den, num); // num mod den, exact, in [-den/2, den/2]
            const double tc = down ? -(rem * d.inv_den) : rem * d.inv_den;
            const double x = mul_rn(d.tps, (double)(p + d.start));
            double t = (x - floor(x)) + tc;
            t -= rint(t);
            const float th = (float)t, tl = (float)(t - (double)th);
            float s, c;
            sincospif(2.0f * th, &s, &c);
            const float dl = 6.28318530717958647692f * tl;
            const float s2 = fmaf(c, dl, s), c2 = fmaf(-s, dl, c);
            acc[j].x = fmaf(d.amp, c2, acc[j].x);
            acc[j].y = fmaf(d.amp, s2, acc[j].y);
        }
    }
#pragma unroll
    for (int j = 0; j < kPerLane; j++) {
        const long long idx = t0 + j * kThreads;
        if (idx >= a.n) continue;
        float2 v = acc[j];
        if (a.noise_scale != 0.0f) {
            const unsigned long long m = (unsigned long long)(a.pos + idx);
            unsigned w0, w1;
            philox4x32_10((unsigned)m, (unsigned)(m >> 32), a.key0, a.key1, w0, w1);
            const float u = fmaf((float)w0, 2.3283064365386963e-10f, 1.1641532182693481e-10f); // (w0 + 1/2) 2^-32, in (0, 1]
            const float rad = a.noise_scale * sqrtf(-2.0f * logf(fminf(u, 1.0f)));
            float gs, gc;
            sincospif((float)w1 * 4.6566128730773926e-10f, &gs, &gc); // 2 pi w1 2^-32
            v.x = fmaf(rad, gc, v.x);
            v.y = fmaf(rad, gs, v.y);
        }
        tx_store<F>(a.out, idx, v, a.full_scale);
    }
}

// ---- the encoder (gr_lora_amd/synth.py encode_shifts, step by step) -----------------------------------------------------

uint8_t hamming_encode(uint32_t nib)
{
    const uint32_t b0 = nib & 1u, b1 = (nib >> 1) & 1u, b2 = (nib >> 2) & 1u, b3 = (nib >> 3) & 1u;
    const uint32_t p1 = b1 ^ b2 ^ b3, p2 = b0 ^ b1 ^ b2, p3 = b0 ^ b1 ^ b3, p4 = b0 ^ b2 ^ b3;
    return (uint8_t)(p1 | (b0 << 1) | (b1 << 2) | (b2 << 3) | (p2 << 4) | (b3 << 5) | (p3 << 6) | (p4 << 7));
}

// inverse of the receiver's deshuffle (out bit j = in bit pat[j])
uint8_t shuffle_tx(uint32_t pre)
{
    static const int pat[8] = {5, 0, 1, 2, 4, 3, 6, 7};
    uint32_t cw = 0;
    for (int j = 0; j < 8; j++) cw |= ((pre >> j) & 1u) << pat[j];
    return (uint8_t)cw;
}

uint32_t rotr(uint32_t v, uint32_t count, uint32_t size)
{
    count %= size;
    const uint32_t mask = (1u << size) - 1u;
    v &= mask;
    return ((v >> count) | (v << (size - count))) & mask;
}

uint32_t gray_inverse(uint32_t w)
{
    uint32_t b = 0;
    for (; w; w >>= 1) b ^= w;
    return b;
}

// lib/decoder_impl.cc:842-847 in float like the reference (synth.payload_symbol_count); volatile keeps every step a rounded float
uint32_t payload_blocks(uint32_t length_with_crc, uint32_t sf, uint32_t cr, bool reduced_rate)
{
    volatile float spb = (float)(cr + 4u);
    volatile float bits = (float)length_with_crc * 8.0f;
    volatile float ratio = spb / 4.0f;
    volatile float prod = bits * ratio;
    volatile float symbols_needed = prod / (float)(sf - (reduced_rate ? 2u : 0u));
    volatile float blocks = symbols_needed / spb;
    return (uint32_t)std::ceil(blocks);
}

lora_hip_status check_frame_fields(const lora_hip_tx_frame_t *f)
{
    if (!f || f->struct_size < sizeof(lora_hip_tx_frame_t) || (f->length && !f->payload)) return LORA_HIP_ERR_ARG;
    if (f->sf < 6 || f->sf > 12) return LORA_HIP_ERR_BAD_SF;
    if (f->cr < 1 || f->cr > 4 || f->length > 255u || (f->sf < 7 && !f->implicit) ||
        (f->flags & ~(LORA_HIP_TX_FRAME_HDR_NIBBLES | LORA_HIP_TX_FRAME_CRC_BYTES)) ||
        ((f->flags & LORA_HIP_TX_FRAME_HDR_NIBBLES) && (f->hdr_nibbles[0] > 15 || f->hdr_nibbles[1] > 15)))
        return LORA_HIP_ERR_BAD_CONFIG;
    return LORA_HIP_OK;
}

// fields checked by the caller
void encode(const lora_hip_tx_frame_t *f, std::vector<uint16_t> &out)
{
    const uint32_t sf = f->sf, cr = f->cr, N = 1u << sf, len = f->length;
    const bool crc = f->crc != 0, implicit = f->implicit != 0, rr = f->reduced_rate != 0;
    std::vector<uint8_t> body(f->payload, f->payload + len);
    if (crc) {
        if (f->flags & LORA_HIP_TX_FRAME_CRC_BYTES) {
            body.push_back(f->crc_bytes[0]);
            body.push_back(f->crc_bytes[1]);
        } else { // the CRC field is not whitened on air but de-whitened like data by the decoder: its bytes carry the whitening
            const uint16_t c = lora_frame::payload_crc16(f->payload, len);
            body.push_back((uint8_t)((c & 0xffu) ^ lora_frame::whiten_at(len)));
            body.push_back((uint8_t)((c >> 8) ^ lora_frame::whiten_at(len + 1u)));
        }
    }
    const unsigned char *prng = cr <= 2 ? LORA_WHITEN_CR56 : LORA_WHITEN_CR78;
    const size_t prng_len = cr <= 2 ? LORA_WHITEN_CR56_LEN : LORA_WHITEN_CR78_LEN;
    const uint32_t ppm_h = sf - 2u, ppm_p = rr ? sf - 2u : sf;
    const uint32_t n_blocks = payload_blocks((uint32_t)body.size(), sf, cr, rr);
    const size_t n_slots = (implicit ? ppm_h : ppm_h - 5u) + (size_t)n_blocks * ppm_p;
    std::vector<uint8_t> cw; // the first block's codewords, then the payload blocks'
    if (!implicit) {
        uint32_t n0 = 0, n1 = 0;
        if (f->flags & LORA_HIP_TX_FRAME_HDR_NIBBLES) { n0 = f->hdr_nibbles[0]; n1 = f->hdr_nibbles[1]; }
        else { const uint32_t c = lora_frame::header_checksum(len, cr, crc ? 1u : 0u); n0 = c >> 4; n1 = c & 15u; }
        const uint32_t hn[5] = {len >> 4, len & 15u, (cr << 1) | (crc ? 1u : 0u), n0, n1};
        for (uint32_t n : hn) cw.push_back(shuffle_tx(hamming_encode(n)));
    }
    for (size_t i = 0; i < n_slots; i++) {
        const uint32_t nib = i < 2 * body.size() ? ((i & 1u) ? body[i / 2] >> 4 : body[i / 2] & 15u) : 0u; // low nibble first
        const uint32_t w = i < prng_len ? prng[i] : 0u;
        cw.push_back(shuffle_tx(hamming_encode(nib) ^ w));
    }
    auto block = [&](const uint8_t *c, uint32_t ppm, uint32_t width, uint32_t mult) {
        for (uint32_t i = 0; i < width; i++) {
            uint32_t wp = 0;
            for (uint32_t x = 0; x < ppm; x++) wp |= (((uint32_t)c[x] >> i) & 1u) << x;
            out.push_back((uint16_t)((mult * gray_inverse(rotr(wp, i, ppm)) + 1u) % N));
        }
    };
    out.clear();
    block(cw.data(), ppm_h, 8u, 4u);
    for (uint32_t b = 0; b < n_blocks; b++) block(cw.data() + ppm_h + (size_t)b * ppm_p, ppm_p, cr + 4u, rr ? 4u : 1u);
}

// D = samp_rate / bandwidth when that is an integer the kernel takes, else 0
uint32_t decimation_of(double samp_rate, const lora_hip_tx_frame_t *f)
{
    if (!f->bandwidth || !(samp_rate > 0.0)) return 0;
    const double d = samp_rate / (double)f->bandwidth;
    if (d < 1.0 || d > (double)LORA_HIP_TX_MAX_DECIMATION || d != std::floor(d) || d * (double)f->bandwidth != samp_rate) return 0;
    const uint32_t D = (uint32_t)d;
    return ((uint64_t)D << f->sf) <= LORA_HIP_TX_MAX_SYMBOL_ITEMS ? D : 0;
}

uint64_t frame_items(uint32_t sps, uint32_t pre, size_t n_shifts) { return ((uint64_t)pre + 4u + n_shifts) * sps + sps / 4u; }

struct Frame {
    TxDesc d;
    std::vector<uint16_t> shifts;
};

} // namespace

struct lora_hip_tx {
    lora_hip_tx_config_t cfg{};
    int device = 0;
    long long pos = 0;
    std::vector<Frame> frames;   // pending, in order of addition
    unsigned short *d_shifts = nullptr;
    size_t shifts_cap = 0, shifts_used = 0, shifts_live = 0;
    TxDesc *d_desc = nullptr;
    size_t desc_cap = 0;
    uint2 *d_rng = nullptr;
    size_t rng_cap = 0;
    unsigned *d_emit = nullptr;
    size_t emit_cap = 0;
    float2 *d_stage = nullptr;
    size_t stage_cap = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_ms = 0.0f;
    std::string err;
    std::vector<TxDesc> h_desc;
    std::vector<uint2> h_rng;
    std::vector<unsigned> h_emit;
};

namespace {

lora_hip_status tfail(lora_hip_tx *h, lora_hip_status s, const char *fmt, ...)
{
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    h->err = buf;
    return s;
}

#define TX_TRY(h, call)                                                                                                    \
    do {                                                                                                                   \
        const hipError_t e_ = (call);                                                                                      \
        if (e_ != hipSuccess) return tfail((h), LORA_HIP_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_));                   \
    } while (0)

template <typename T>
lora_hip_status grow(lora_hip_tx *h, T *&p, size_t &cap, size_t need)
{
    if (need <= cap) return LORA_HIP_OK;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    const size_t want = need + need / 2 + 64;
    if (hipMalloc((void **)&p, want * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); return tfail(h, LORA_HIP_ERR_NOMEM, "hipMalloc of %zu bytes", want * sizeof(T)); }
    cap = want;
    return LORA_HIP_OK;
}

// the shift arena holds every pending frame's shifts; (re)built from the host copies when it is too small or mostly dead
lora_hip_status arena_rebuild(lora_hip_tx *h, size_t extra)
{
    size_t live = 0;
    for (const Frame &f : h->frames) live += f.shifts.size();
    std::vector<uint16_t> all;
    all.reserve(live);
    const lora_hip_status s = grow(h, h->d_shifts, h->shifts_cap, std::max<size_t>(2 * (live + extra), 4096));
    if (s != LORA_HIP_OK) return s;
    for (Frame &f : h->frames) {
        f.d.shift_off = (unsigned)all.size();
        all.insert(all.end(), f.shifts.begin(), f.shifts.end());
    }
    if (!all.empty()) TX_TRY(h, hipMemcpy(h->d_shifts, all.data(), all.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    h->shifts_used = h->shifts_live = live;
    return LORA_HIP_OK;
}

template <int F>
hipError_t tx_launch_as(unsigned tiles, hipStream_t st, const TxArgs &a)
{
    hipLaunchKernelGGL(tx_kernel<F>, dim3(tiles), dim3(kThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t tx_launch(int fmt, unsigned tiles, hipStream_t st, const TxArgs &a)
{
    switch (fmt) {
    case LORA_HIP_IQ_SC16: return tx_launch_as<LORA_HIP_IQ_SC16>(tiles, st, a);
    case LORA_HIP_IQ_SC8: return tx_launch_as<LORA_HIP_IQ_SC8>(tiles, st, a);
    case LORA_HIP_IQ_CU8: return tx_launch_as<LORA_HIP_IQ_CU8>(tiles, st, a);
    default: return tx_launch_as<LORA_HIP_IQ_CF32>(tiles, st, a);
    }
}

lora_hip_status tx_generate(lora_hip_tx *h, void *d_out, size_t n, int fmt, double full_scale, void *hip_stream)
{
    if (!h) return LORA_HIP_ERR_ARG;
    const size_t ib = lora_iq::item_bytes(fmt);
    if (!ib) return tfail(h, LORA_HIP_ERR_ARG, "unknown format %d", fmt);
    if (fmt != LORA_HIP_IQ_CF32 && !(std::isfinite(full_scale) && full_scale > 0.0)) return tfail(h, LORA_HIP_ERR_ARG, "full_scale %g must be finite and positive", full_scale);
    if (n && (!d_out || ((uintptr_t)d_out & (ib - 1)))) return tfail(h, LORA_HIP_ERR_ARG, "output NULL or not aligned to its %zu-byte item", ib);
    if (n > (size_t)0x7fffffffull * kTile / 2 || (long long)n > INT64_MAX / 4 - h->pos) return tfail(h, LORA_HIP_ERR_ARG, "%zu items in one call", n);
    h->last_ms = 0.0f;
    if (!n) return LORA_HIP_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    TX_TRY(h, hipSetDevice(h->device));
    const long long pos = h->pos, end = pos + (long long)n;
    const size_t tiles = (n + kTile - 1) / kTile;
    // the emitters of this call, and per tile the range of the list that holds those overlapping it
    h->h_desc.clear();
    struct Ev { size_t tile; unsigned id; bool add; };
    std::vector<Ev> evs;
    for (const Frame &f : h->frames) {
        if (f.d.start >= end || f.d.start + f.d.len <= pos) continue;
        const unsigned id = (unsigned)h->h_desc.size();
        h->h_desc.push_back(f.d);
        const long long a = std::max(f.d.start, pos) - pos, b = std::min(f.d.start + f.d.len, end) - 1 - pos;
        evs.push_back({(size_t)(a / kTile), id, true});
        evs.push_back({(size_t)(b / kTile) + 1, id, false});
    }
    std::stable_sort(evs.begin(), evs.end(), [](const Ev &x, const Ev &y) { return x.tile < y.tile; });
    h->h_rng.assign(tiles, make_uint2(0u, 0u));
    h->h_emit.clear();
    std::vector<unsigned> active;
    size_t t = 0, ei = 0;
    uint2 cur = make_uint2(0u, 0u);
    while (t < tiles) {
        bool changed = false;
        for (; ei < evs.size() && evs[ei].tile <= t; ei++) {
            auto it = std::lower_bound(active.begin(), active.end(), evs[ei].id);
            if (evs[ei].add) active.insert(it, evs[ei].id);
            else active.erase(it);
            changed = true;
        }
        if (changed) {
            cur = make_uint2((unsigned)h->h_emit.size(), (unsigned)active.size());
            h->h_emit.insert(h->h_emit.end(), active.begin(), active.end());
        }
        const size_t until = ei < evs.size() ? std::min(evs[ei].tile, tiles) : tiles;
        for (; t < until; t++) h->h_rng[t] = cur;
    }
    lora_hip_status s;
    if ((s = grow(h, h->d_desc, h->desc_cap, std::max<size_t>(h->h_desc.size(), 1))) != LORA_HIP_OK) return s;
    if ((s = grow(h, h->d_rng, h->rng_cap, tiles)) != LORA_HIP_OK) return s;
    if ((s = grow(h, h->d_emit, h->emit_cap, std::max<size_t>(h->h_emit.size(), 1))) != LORA_HIP_OK) return s;
    if (!h->h_desc.empty()) TX_TRY(h, hipMemcpyAsync(h->d_desc, h->h_desc.data(), h->h_desc.size() * sizeof(TxDesc), hipMemcpyHostToDevice, st));
    TX_TRY(h, hipMemcpyAsync(h->d_rng, h->h_rng.data(), tiles * sizeof(uint2), hipMemcpyHostToDevice, st));
    if (!h->h_emit.empty()) TX_TRY(h, hipMemcpyAsync(h->d_emit, h->h_emit.data(), h->h_emit.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
    TxArgs a{};
    a.desc = h->d_desc; a.tile_rng = h->d_rng; a.tile_emit = h->d_emit; a.shifts = h->d_shifts; a.out = d_out;
    a.pos = pos; a.n = (long long)n; a.full_scale = full_scale;
    a.noise_scale = (float)(h->cfg.noise_sigma / std::sqrt(2.0));
    a.key0 = (unsigned)h->cfg.seed; a.key1 = (unsigned)(h->cfg.seed >> 32);
    TX_TRY(h, hipEventRecord(h->ev0, st));
    TX_TRY(h, tx_launch(fmt, (unsigned)tiles, st, a));
    TX_TRY(h, hipEventRecord(h->ev1, st));
    TX_TRY(h, hipStreamSynchronize(st));
    TX_TRY(h, hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1));
    h->pos = end;
    // frames wholly behind the position are retired
    size_t keep = 0;
    for (size_t i = 0; i < h->frames.size(); i++) {
        if (h->frames[i].d.start + h->frames[i].d.len <= end) { h->shifts_live -= h->frames[i].shifts.size(); continue; }
        if (keep != i) h->frames[keep] = std::move(h->frames[i]);
        keep++;
    }
    h->frames.resize(keep);
    if (h->frames.empty()) h->shifts_used = h->shifts_live = 0;
    return LORA_HIP_OK;
}

} // namespace

extern "C" {

lora_hip_status lora_hip_tx_encode(const lora_hip_tx_frame_t *f, uint16_t *shifts, size_t cap, uint32_t *n_hdr, uint32_t *n_pay)
{
    if (!n_hdr || !n_pay) return LORA_HIP_ERR_ARG;
    const lora_hip_status s = check_frame_fields(f);
    if (s != LORA_HIP_OK) return s;
    std::vector<uint16_t> out;
    encode(f, out);
    *n_hdr = 8u;
    *n_pay = (uint32_t)out.size() - 8u;
    if (!shifts) return LORA_HIP_OK;
    if (cap < out.size()) return LORA_HIP_ERR_OVERFLOW;
    std::memcpy(shifts, out.data(), out.size() * sizeof(uint16_t));
    return LORA_HIP_OK;
}

lora_hip_status lora_hip_tx_frame_items(const lora_hip_tx_frame_t *f, float samp_rate, uint64_t *items)
{
    if (!items) return LORA_HIP_ERR_ARG;
    const lora_hip_status s = check_frame_fields(f);
    if (s != LORA_HIP_OK) return s;
    const uint32_t D = decimation_of((double)samp_rate, f);
    if (!D || f->preamble_len > LORA_HIP_TX_MAX_PREAMBLE) return LORA_HIP_ERR_BAD_CONFIG;
    std::vector<uint16_t> out;
    encode(f, out);
    *items = frame_items(D << f->sf, f->preamble_len ? f->preamble_len : 8u, out.size());
    return LORA_HIP_OK;
}

lora_hip_status lora_hip_tx_create(const lora_hip_tx_config_t *cfg, lora_hip_tx_t **out)
{
    if (!cfg || !out || cfg->struct_size < sizeof(lora_hip_tx_config_t)) return LORA_HIP_ERR_ARG;
    *out = nullptr;
    if (cfg->device < 0) return LORA_HIP_ERR_ARG;
    if (!std::isfinite(cfg->samp_rate) || !(cfg->samp_rate > 0.0) || !std::isfinite(cfg->noise_sigma) || cfg->noise_sigma < 0.0 || cfg->flags != 0)
        return LORA_HIP_ERR_BAD_CONFIG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device >= ndev) { (void)hipGetLastError(); return LORA_HIP_ERR_NO_DEVICE; }
    auto *h = new lora_hip_tx;
    h->cfg = *cfg;
    h->device = cfg->device;
    lora_hip_status st = LORA_HIP_OK;
    if (hipSetDevice(h->device) != hipSuccess) st = LORA_HIP_ERR_NO_DEVICE;
    else if (hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) st = LORA_HIP_ERR_HIP;
    else st = arena_rebuild(h, 0);
    if (st != LORA_HIP_OK) { lora_hip_tx_destroy(h); return st; }
    *out = h;
    return LORA_HIP_OK;
}

void lora_hip_tx_destroy(lora_hip_tx_t *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->d_shifts) (void)hipFree(h->d_shifts);
    if (h->d_desc) (void)hipFree(h->d_desc);
    if (h->d_rng) (void)hipFree(h->d_rng);
    if (h->d_emit) (void)hipFree(h->d_emit);
    if (h->d_stage) (void)hipFree(h->d_stage);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    delete h;
}

const char *lora_hip_tx_last_error(const lora_hip_tx_t *h) { return h ? h->err.c_str() : "null handle"; }

lora_hip_status lora_hip_tx_add_frames(lora_hip_tx_t *h, const lora_hip_tx_frame_t *frames, size_t n)
{
    if (!h || (n && !frames)) return LORA_HIP_ERR_ARG;
    std::vector<Frame> add(n);
    size_t extra = 0;
    for (size_t i = 0; i < n; i++) {
        const lora_hip_tx_frame_t *f = &frames[i];
        if (f->struct_size != sizeof(lora_hip_tx_frame_t)) return tfail(h, LORA_HIP_ERR_ARG, "frame %zu: struct_size %u", i, f->struct_size);
        const lora_hip_status s = check_frame_fields(f);
        if (s != LORA_HIP_OK) return tfail(h, s, "frame %zu: sf %u, cr %u, length %u, implicit %u or flags 0x%x refused", i, f->sf, f->cr, f->length, f->implicit, f->flags);
        const uint32_t D = decimation_of(h->cfg.samp_rate, f);
        if (!D || f->preamble_len > LORA_HIP_TX_MAX_PREAMBLE)
            return tfail(h, LORA_HIP_ERR_BAD_CONFIG, "frame %zu: samp_rate %g over bandwidth %u at sf %u, or preamble_len %u", i, h->cfg.samp_rate, f->bandwidth, f->sf, f->preamble_len);
        if (!std::isfinite(f->amplitude) || !std::isfinite(f->freq_hz)) return tfail(h, LORA_HIP_ERR_ARG, "frame %zu: amplitude or freq_hz not finite", i);
        if (f->start < h->pos || f->start > INT64_MAX / 4) return tfail(h, LORA_HIP_ERR_ARG, "frame %zu: start %lld lies before the position %lld", i, (long long)f->start, h->pos);
        Frame &g = add[i];
        encode(f, g.shifts);
        const int N = 1 << f->sf, sps = (int)(D << f->sf), pre = (int)(f->preamble_len ? f->preamble_len : 8u);
        TxDesc &d = g.d;
        d.start = f->start;
        d.len = (long long)frame_items((uint32_t)sps, (uint32_t)pre, g.shifts.size());
        d.body = (long long)(pre + 4) * sps + sps / 4;
        d.tps = f->freq_hz / h->cfg.samp_rate;
        d.inv_sps = 1.0 / (double)sps;
        d.den = 2.0 * (double)D * (double)sps;
        d.inv_den = 1.0 / d.den;
        d.amp = f->amplitude;
        d.sps = sps; d.D = (int)D; d.pre = pre;
        d.sync0 = f->sync_shifts[0] < 0 ? 3 * N / 16 : f->sync_shifts[0] % N;
        d.sync1 = f->sync_shifts[1] < 0 ? N / 4 : f->sync_shifts[1] % N;
        d.shift_off = 0; d.pad = 0;
        extra += g.shifts.size();
    }
    if (!n) return LORA_HIP_OK;
    TX_TRY(h, hipSetDevice(h->device));
    const size_t first = h->frames.size();
    if (h->shifts_used + extra > h->shifts_cap || h->shifts_used > 2 * h->shifts_live + 65536) { // no room, or mostly retired frames: compact
        for (Frame &g : add) h->frames.push_back(std::move(g));
        const lora_hip_status s = arena_rebuild(h, 0);
        if (s != LORA_HIP_OK) { h->frames.resize(first); return s; }
        return LORA_HIP_OK;
    }
    std::vector<uint16_t> all;
    all.reserve(extra);
    for (Frame &g : add) {
        g.d.shift_off = (unsigned)(h->shifts_used + all.size());
        all.insert(all.end(), g.shifts.begin(), g.shifts.end());
    }
    TX_TRY(h, hipMemcpy(h->d_shifts + h->shifts_used, all.data(), all.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    h->shifts_used += extra;
    h->shifts_live += extra;
    for (Frame &g : add) h->frames.push_back(std::move(g));
    return LORA_HIP_OK;
}

lora_hip_status lora_hip_tx_generate_device(lora_hip_tx_t *h, void *d_out, size_t n, void *hip_stream)
{
    return tx_generate(h, d_out, n, LORA_HIP_IQ_CF32, 1.0, hip_stream);
}

lora_hip_status lora_hip_tx_generate_device_raw(lora_hip_tx_t *h, void *d_out, size_t n, int fmt, double full_scale, void *hip_stream)
{
    return tx_generate(h, d_out, n, fmt, full_scale, hip_stream);
}

lora_hip_status lora_hip_tx_generate(lora_hip_tx_t *h, float *out, size_t n)
{
    if (!h || (n && !out)) return LORA_HIP_ERR_ARG;
    if (!n) return LORA_HIP_OK;
    TX_TRY(h, hipSetDevice(h->device));
    lora_hip_status s = grow(h, h->d_stage, h->stage_cap, n);
    if (s != LORA_HIP_OK) return s;
    if ((s = tx_generate(h, h->d_stage, n, LORA_HIP_IQ_CF32, 1.0, nullptr)) != LORA_HIP_OK) return s;
    TX_TRY(h, hipMemcpy(out, h->d_stage, n * sizeof(float2), hipMemcpyDeviceToHost));
    return LORA_HIP_OK;
}

int64_t lora_hip_tx_position(const lora_hip_tx_t *h) { return h ? h->pos : 0; }
size_t lora_hip_tx_pending(const lora_hip_tx_t *h) { return h ? h->frames.size() : 0; }
float lora_hip_tx_last_kernel_ms(const lora_hip_tx_t *h) { return h ? h->last_ms : 0.0f; }

} // extern "C"
