// lora_soft.inc.hip -- soft-decision decoding at known header positions (beyond the reference).  Included by lora_kernels.hip.
//
// The hard chain keeps one arg-max bin per symbol; everything that tells a wrong bin from a barely-right one is gone before the de-interleaver
// spreads each codeword over 4 + CR symbols.  soft_symbols_kernel keeps, per bit of a symbol's word, the max-log likelihood ratio over the whole
// dechirped spectrum; soft_chain_kernel carries those through de-interleaver, de-shuffle and de-whitening as positions and signs and decides each
// codeword by correlation against the 16 codewords of the Hamming(8,4) code, at every CR (a position that was not sent is an erasure).
// Definition (float64): gr_lora_amd/softdecode.py; contract: include/lora_hip_soft.h; DESIGN.md 4.19.
//
// soft_symbols_kernel: one 256-thread workgroup per window, the pruned polyphase spectrum of get_shift_fft (:430-464, no N/2 fold) as in
// lora_detect.inc.hip - one pass, not two - and an epilogue on the bins each thread holds in registers:
//   m = sqrtf(re^2 + im^2); b = (k - 1) mod N; reduced: b = ((b + 2) >> 2) mod N/4; w = b ^ (b >> 1)
//   2 x 12 running maxima (bit i of w clear / set), reduced over the wavefront with cross-lane shuffles and over the four wavefronts through ONE
//   exchange in LDS together with the arg-max;  L[i] = max0[i] - max1[i].
// The spectrum differs from detect_spectrum's structure in three ways (measured against that structure before it was dropped from this file: DESIGN 4.19,
// profiles/soft_bench.txt):
//   * two radix-2 stages per workgroup barrier (a radix-2^2 step on four elements: the same operations on the same operands, so the same bits);
//   * a row stride of N + 16 / rows cf32 instead of N + 1: an 8-byte LDS store is served in groups of 16 consecutive lanes over 32 banks of 4 bytes,
//     and 16 lanes write `rows` polyphase rows at 16 / rows consecutive columns - with this stride to 16 different bank pairs;
//   * every thread takes the bins whose BIT-REVERSED index is tid + 256 m, so the transform's bit-reversed output is read at consecutive LDS
//     addresses (the word of a bin is computed, not looked up: which bins a thread holds does not matter to the epilogue).

__device__ __forceinline__ void soft_spectrum(const DevParams &P, const float2 *__restrict__ x, float2 *work, const uint32_t stride, float2 (&acc)[kMaxBinsPerThread])
{
    const uint32_t N = P.nbins, D = P.decim, G = P.fft_groups, DG = D / G, logN = P.log_nbins;
    const uint32_t pts = N * DG, smask = P.sps - 1u;
#pragma unroll
    for (int m = 0; m < kMaxBinsPerThread; m++) acc[m] = make_float2(0.0f, 0.0f);
    for (uint32_t g = 0; g < G; g++) {
        for (uint32_t idx = threadIdx.x; idx < pts; idx += kWG) {
            const uint32_t rr = idx % DG, q = idx / DG;
            const uint32_t n = q * D + g * DG + rr;
            work[rr * stride + q] = cmul(x[n], P.down[n]);
        }
        __syncthreads();
        uint32_t h = N >> 1;
        for (; h >= 2u; h >>= 2) { // stages h and h / 2 on the four elements {off, off + h/2, off + h, off + 3h/2} of a block of 2h
            const uint32_t hh = h >> 1, tw_step = (N >> 1) / h;
            for (uint32_t b = threadIdx.x; b < (pts >> 2); b += kWG) {
                const uint32_t arr = b / (N >> 2), j = b % (N >> 2);
                const uint32_t off = j & (hh - 1u), blk = j / hh;
                const uint32_t i0 = arr * stride + blk * 2u * h + off;
                const float2 a = work[i0], bq = work[i0 + hh], c = work[i0 + h], d = work[i0 + h + hh];
                const float2 a1 = make_float2(a.x + c.x, a.y + c.y), c1 = cmul(make_float2(a.x - c.x, a.y - c.y), P.twN[off * tw_step]);
                const float2 b1 = make_float2(bq.x + d.x, bq.y + d.y), d1 = cmul(make_float2(bq.x - d.x, bq.y - d.y), P.twN[(off + hh) * tw_step]);
                const float2 t2 = P.twN[off * 2u * tw_step];
                work[i0] = make_float2(a1.x + b1.x, a1.y + b1.y);
                work[i0 + hh] = cmul(make_float2(a1.x - b1.x, a1.y - b1.y), t2);
                work[i0 + h] = make_float2(c1.x + d1.x, c1.y + d1.y);
                work[i0 + h + hh] = cmul(make_float2(c1.x - d1.x, c1.y - d1.y), t2);
            }
            __syncthreads();
        }
        for (; h >= 1u; h >>= 1) { // (the last stage where log2 N is odd)
            const uint32_t tw_step = (N >> 1) / h;
            for (uint32_t b = threadIdx.x; b < (pts >> 1); b += kWG) {
                const uint32_t arr = b / (N >> 1), j = b % (N >> 1);
                const uint32_t off = j & (h - 1u), blk = j / h;
                const uint32_t i0 = arr * stride + blk * 2u * h + off, i1 = i0 + h;
                const float2 a = work[i0], c = work[i1];
                const float2 d = make_float2(a.x - c.x, a.y - c.y);
                work[i0] = make_float2(a.x + c.x, a.y + c.y);
                work[i1] = cmul(d, P.twN[off * tw_step]);
            }
            __syncthreads();
        }
#pragma unroll
        for (int m = 0; m < kMaxBinsPerThread; m++) {
            const uint32_t p = threadIdx.x + (uint32_t)m * kWG;
            if (p < N) {
                const uint32_t j = bitrev(p, logN); // the bin (k mod N) the transform left at p
                const int32_t k = (j < N / 2u) ? (int32_t)j : (int32_t)j - (int32_t)N;
                for (uint32_t rr = 0; rr < DG; rr++) {
                    const uint32_t r = g * DG + rr;
                    const float2 t = cmul(work[rr * stride + p], P.tws[(uint32_t)(k * (int32_t)r) & smask]);
                    acc[m].x += t.x; acc[m].y += t.y;
                }
            }
        }
        __syncthreads();
    }
}

__host__ __device__ inline uint32_t soft_stride(const DevParams &p)
{
    const uint32_t rows = p.decim / p.fft_groups;
    return p.nbins + (rows >= 2u ? 16u / rows : 0u);
}

__global__ __launch_bounds__(kWG) void soft_symbols_kernel(DevParams P, const float2 *iq, const int64_t *offsets, const uint8_t *reduced, uint32_t n, uint32_t lds_work,
                                                           float *llr, SoftSym *out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float2 *work = reinterpret_cast<float2 *>(smem);
    float *red = reinterpret_cast<float *>(smem + lds_work); // 4 x 32 floats
    const uint32_t N = P.nbins, logN = P.log_nbins, stride = soft_stride(P);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t s = blockIdx.x; s < n; s += gridDim.x) {
        float2 acc[kMaxBinsPerThread];
        soft_spectrum(P, iq + offsets[s], work, stride, acc);
        const bool red_rate = reduced[s] != 0;
        const uint32_t ppm = red_rate ? P.sf - 2u : P.sf;
        float mx0[kSoftStride], mx1[kSoftStride];
#pragma unroll
        for (int i = 0; i < (int)kSoftStride; i++) { mx0[i] = -1.0f; mx1[i] = -1.0f; }
        float bv = -1.0f;
        int bi = 0x7fffffff;
#pragma unroll
        for (int m = 0; m < kMaxBinsPerThread; m++) {
            const uint32_t p = threadIdx.x + (uint32_t)m * kWG;
            if (p < N) {
                const uint32_t j = bitrev(p, logN);
                const float mag = sqrtf(acc[m].x * acc[m].x + acc[m].y * acc[m].y);
                if (mag > bv || (mag == bv && (int)j < bi)) { bv = mag; bi = (int)j; }
                uint32_t b = (j - 1u) & (N - 1u); // the plain FFT demodulator's bin
                if (red_rate) b = ((b + 2u) >> 2) & ((N >> 2) - 1u);
                const uint32_t w = b ^ (b >> 1);
#pragma unroll
                for (int i = 0; i < (int)kSoftStride; i++) {
                    const bool one = (w >> i) & 1u;
                    mx0[i] = fmaxf(mx0[i], one ? -1.0f : mag);
                    mx1[i] = fmaxf(mx1[i], one ? mag : -1.0f);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < (int)kSoftStride; i++) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                mx0[i] = fmaxf(mx0[i], __shfl_xor(mx0[i], o, 64));
                mx1[i] = fmaxf(mx1[i], __shfl_xor(mx1[i], o, 64));
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) {
            float *r = red + wave * 32;
#pragma unroll
            for (int i = 0; i < (int)kSoftStride; i++) { r[i] = mx0[i]; r[kSoftStride + i] = mx1[i]; }
            r[24] = bv; reinterpret_cast<int *>(r)[25] = bi;
        }
        __syncthreads();
        if (threadIdx.x < kSoftStride) {
            const uint32_t i = threadIdx.x;
            const float a = fmaxf(fmaxf(red[i], red[32 + i]), fmaxf(red[64 + i], red[96 + i]));
            const float b = fmaxf(fmaxf(red[kSoftStride + i], red[32 + kSoftStride + i]), fmaxf(red[64 + kSoftStride + i], red[96 + kSoftStride + i]));
            llr[(size_t)s * kSoftStride + i] = (i < ppm) ? a - b : 0.0f;
        } else if (threadIdx.x == 64) {
            float v = red[24];
            int idx = reinterpret_cast<int *>(red)[25];
            for (int w = 1; w < kWG / 64; w++) {
                const float ov = red[w * 32 + 24];
                const int oi = reinterpret_cast<int *>(red)[w * 32 + 25];
                if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
            }
            SoftSym o; o.k = idx; o.peak = v;
            out[s] = o;
        }
        __syncthreads();
    }
}

uint32_t soft_lds_bytes(const DevParams &p, uint32_t *work_bytes)
{
    const uint32_t rows = p.decim / p.fft_groups;
    const uint32_t work = (uint32_t)(((size_t)rows * soft_stride(p) * sizeof(float2) + 15u) & ~(size_t)15u);
    if (work_bytes) *work_bytes = work;
    return work + 4u * 32u * (uint32_t)sizeof(float);
}

int launch_soft_symbols(const DevParams &p, const float2 *iq, const int64_t *d_offsets, const uint8_t *d_reduced, uint32_t n, float *d_llr, SoftSym *d_sym, void *stream)
{
    if (n == 0) return 0;
    uint32_t work = 0;
    const uint32_t lds = soft_lds_bytes(p, &work);
    if (lds > 64u * 1024u) {
        if (hipFuncSetAttribute((const void *)soft_symbols_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -1;
    }
    hipLaunchKernelGGL(soft_symbols_kernel, dim3(n < 4096u ? n : 4096u), dim3(kWG), lds, (hipStream_t)stream, p, iq, d_offsets, d_reduced, n, work, d_llr, d_sym);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// codeword c of frame f: nibble, margin, hard word, sum of |LLR|.  fp32, additions only, j ascending: softdecode.soft_block(dtype=float32) forms the same sums.
__device__ __forceinline__ SoftCw soft_codeword(const DevParams &P, const SoftFrameDesc &f, uint32_t c, const float *__restrict__ llr_hdr, const float *__restrict__ llr_pay)
{
#pragma clang fp contract(off)
    const float *base;
    uint32_t x, nw, ppm;
    if (c < f.n_first) { x = f.first_x + c; nw = 8u; ppm = P.sf - 2u; base = llr_hdr + (size_t)f.hdr_win * kSoftStride; }
    else { const uint32_t cc = c - f.n_first; x = cc % f.ppm; nw = f.n_w; ppm = f.ppm; base = llr_pay + ((size_t)f.pay_win + (size_t)(cc / f.ppm) * f.n_w) * kSoftStride; }
    uint32_t wb = 0;
    if (f.table == 0u) wb = (c < LORA_WHITEN_HEADER_LEN) ? c_whiten_header[c] : 0u;
    else if (f.table == 1u) wb = (c < LORA_WHITEN_CR56_LEN) ? c_whiten_cr56[c] : 0u;
    else wb = (c < LORA_WHITEN_CR78_LEN) ? c_whiten_cr78[c] : 0u;
    float C[8], sa = 0.0f;
#pragma unroll
    for (uint32_t i = 0; i < 8u; i++) {
        C[i] = (i < nw) ? base[i * kSoftStride + (x + 2u * ppm - i) % ppm] : 0.0f; // C_x[i] = L_i[(x - i) mod ppm]; absent: an erasure
        if (i < nw) sa += fabsf(C[i]);
    }
    const float Cs[8] = {C[5], C[0], C[1], C[2], C[4], C[3], C[6], C[7]}; // de-shuffle {5,0,1,2,4,3,6,7} (:568)
    float Dv[8];
    uint32_t hard = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8u; j++) {
        const uint32_t wbit = (wb >> j) & 1u;
        hard |= ((Cs[j] < 0.0f ? 1u : 0u) ^ wbit) << j;
        Dv[j] = wbit ? -Cs[j] : Cs[j];
    }
    float best = -INFINITY, second = -INFINITY;
    uint32_t nib = 0, nib2 = 0;
#pragma unroll
    for (uint32_t s = 0; s < 16u; s++) {
        const uint32_t e = hamming84_encode(s);
        float sc = 0.0f;
#pragma unroll
        for (uint32_t j = 0; j < 8u; j++) sc += ((e >> j) & 1u) ? -Dv[j] : Dv[j];
        if (sc > best) { second = best; nib2 = nib; best = sc; nib = s; } // (a displaced best has the smaller index: the first of equal runners-up stays)
        else if (sc > second) { second = sc; nib2 = s; }
    }
    SoftCw o;
    o.margin = best - second; o.sum_abs = sa; o.nibble = (uint8_t)nib; o.hard = (uint8_t)hard; o.second = (uint8_t)nib2; o.pad = 0;
    return o;
}

// one thread per PAIR of codewords: both decisions, their records, and the byte they make (low nibble first; 0 where a nibble is missing)
__global__ __launch_bounds__(64) void soft_chain_kernel(DevParams P, const SoftFrameDesc *descs, const float *llr_hdr, const float *llr_pay, SoftCw *cws, uint8_t *bytes)
{
    const SoftFrameDesc f = descs[blockIdx.x];
    const uint32_t pair = blockIdx.y * 64u + threadIdx.x;
    uint32_t nib[2] = {0u, 0u};
    for (uint32_t t = 0; t < 2u; t++) {
        const uint32_t c = 2u * pair + t;
        if (c < f.n_cw) {
            const SoftCw o = soft_codeword(P, f, c, llr_hdr, llr_pay);
            cws[f.cw_out + c] = o;
            nib[t] = o.nibble;
        }
    }
    if (pair < f.n_bytes) bytes[f.byte_out + pair] = (uint8_t)(nib[0] | (nib[1] << 4));
}

int launch_soft_chain(const DevParams &p, const SoftFrameDesc *d_descs, uint32_t n_frames, uint32_t max_pairs, const float *d_llr_hdr, const float *d_llr_pay, SoftCw *d_cws,
                      uint8_t *d_bytes, void *stream)
{
    if (n_frames == 0 || max_pairs == 0) return 0;
    if (ensure_constants() != 0) return -1;
    hipLaunchKernelGGL(soft_chain_kernel, dim3(n_frames, (max_pairs + 63u) / 64u), dim3(64), 0, (hipStream_t)stream, p, d_descs, d_llr_hdr, d_llr_pay, d_cws, d_bytes);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- CRC-aided repair of the least reliable codewords (softdecode.crc_repair) ------------------------------------------
// The payload CRC (lora_frame_check.h: CCITT from 0 over all but the last two payload bytes, those XORed in, no final XOR) XOR the received,
// de-whitened CRC bytes is affine over GF(2) in the bits of the frame body: the syndrome is the XOR of one 16-bit word per body byte and of the
// whitening constant, and giving a codeword its runner-up nibble changes it by one fixed word.  All of it is integer arithmetic but the penalty.

// a * b in GF(2)[x] mod x^16 + x^12 + x^5 + 1; a, b < 2^16
__device__ __forceinline__ uint32_t soft_gf_mul(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
    for (int i = 15; i >= 0; i--) {
        r = (r << 1) ^ ((r & 0x8000u) ? 0x11021u : 0u);
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}

// what the value v at byte k of a body of length + 2 bytes adds to the syndrome: the received CRC bytes low byte first; payload byte k with
// m = length - 1 - k bytes behind it: m = 0 enters as the low byte, m = 1 as the high byte, m >= 2 is the high byte advanced 8 (m - 1) steps
__device__ __forceinline__ uint32_t soft_syn_of_byte(uint32_t v, uint32_t k, uint32_t length)
{
    if (k >= length) return k == length ? v : v << 8;
    uint32_t m = length - 1u - k;
    if (m == 0u) return v;
    uint32_t r = 1u, p = 0x100u; // x^(8 (m - 1)) by squaring
    for (m -= 1u; m; m >>= 1) {
        if (m & 1u) r = soft_gf_mul(r, p);
        p = soft_gf_mul(p, p);
    }
    return soft_gf_mul(v << 8, r);
}

// One 256-thread workgroup per frame.  Syndrome: a byte per lane (two for lanes 0 of the longest bodies), XOR over the wavefront by shuffles and
// over the four wavefronts through LDS.  Candidates: the rank of every eligible codeword under (margin, c), counted against the margins in LDS
// (reads of one address by all lanes: a broadcast) - ranks below n_cand name the candidates.  Patterns: lane p owns pattern p.
__global__ __launch_bounds__(kWG) void soft_repair_kernel(const SoftRepairDesc *descs, uint32_t n_frames, uint32_t max_cand, const SoftCw *cws, uint8_t *bytes, SoftRepairRec *recs)
{
#pragma clang fp contract(off)
    __shared__ float s_margin[2u * kSoftRepairMaxBody];
    __shared__ uint32_t s_syn[kWG / 64], s_pat[kWG / 64], s_cand[kSoftRepairMaxCand], s_e[kSoftRepairMaxCand];
    __shared__ float s_pen[kWG / 64], s_m[kSoftRepairMaxCand];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t f = blockIdx.x; f < n_frames; f += gridDim.x) {
        const SoftRepairDesc d = descs[f];
        const uint32_t n_body = d.length + 2u;
        const uint32_t n_elig = 2u * n_body < d.n_cw ? 2u * n_body : d.n_cw;
        const uint32_t n_cand = max_cand < n_elig ? max_cand : n_elig;
        uint32_t syn = 0;
        for (uint32_t k = tid; k < n_body; k += kWG) syn ^= soft_syn_of_byte(bytes[d.byte_io + k], k, d.length);
        for (uint32_t c = tid; c < n_elig; c += kWG) s_margin[c] = cws[d.cw_in + c].margin;
        if (tid < kSoftRepairMaxCand) s_cand[tid] = 0u;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) syn ^= (uint32_t)__shfl_xor((int)syn, o, 64);
        if (lane == 0u) s_syn[wave] = syn;
        __syncthreads();
        syn = (s_syn[0] ^ s_syn[1] ^ s_syn[2] ^ s_syn[3] ^ d.whiten) & 0xffffu;
        if (syn == 0u) { // (the same in every lane)
            if (tid == 0u) {
                SoftRepairRec r = {};
                r.status = 1u; // CRC_HELD
                recs[f] = r;
            }
        } else {
            for (uint32_t c = tid; c < n_elig; c += kWG) {
                const float m = s_margin[c];
                uint32_t rank = 0;
                for (uint32_t o = 0; o < n_elig; o++) {
                    const float mo = s_margin[o];
                    rank += (mo < m || (mo == m && o < c)) ? 1u : 0u;
                }
                if (rank < n_cand) s_cand[rank] = c;
            }
            __syncthreads();
            if (tid < kSoftRepairMaxCand) {
                uint32_t e = 0;
                float m = 0.0f;
                if (tid < n_cand) {
                    const uint32_t c = s_cand[tid];
                    const SoftCw w = cws[d.cw_in + c];
                    e = soft_syn_of_byte((uint32_t)((w.nibble ^ w.second) & 15u) << (4u * (c & 1u)), c >> 1, d.length);
                    m = s_margin[c];
                }
                s_e[tid] = e; s_m[tid] = m;
            }
            __syncthreads();
            float pen = INFINITY;
            uint32_t pat = 0xffffffffu; // no match
            if (tid >= 1u && tid < (1u << n_cand)) {
                uint32_t x = 0;
                float s = 0.0f;
                for (uint32_t i = 0; i < n_cand; i++)
                    if ((tid >> i) & 1u) { x ^= s_e[i]; s += s_m[i]; }
                if (x == syn) { pen = s; pat = tid; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float op = __shfl_xor(pen, o, 64);
                const uint32_t oq = (uint32_t)__shfl_xor((int)pat, o, 64);
                if (op < pen || (op == pen && oq < pat)) { pen = op; pat = oq; }
            }
            if (lane == 0u) { s_pen[wave] = pen; s_pat[wave] = pat; }
            __syncthreads();
            if (tid == 0u) {
                for (uint32_t w = 1; w < kWG / 64; w++)
                    if (s_pen[w] < pen || (s_pen[w] == pen && s_pat[w] < pat)) { pen = s_pen[w]; pat = s_pat[w]; }
                SoftRepairRec r = {};
                r.status = 3u; // FAILED
                r.candidates = n_cand; r.syndrome = (uint16_t)syn;
                for (uint32_t i = 0; i < n_cand; i++) r.codeword[i] = (uint16_t)s_cand[i];
                if (pat != 0xffffffffu) {
                    r.status = 2u; // REPAIRED
                    r.pattern = pat; r.changed = (uint32_t)__popc(pat); r.penalty = pen;
                    for (uint32_t i = 0; i < n_cand; i++) // one lane, one byte after the other: two candidates may share a byte
                        if ((pat >> i) & 1u) {
                            const uint32_t c = s_cand[i];
                            const SoftCw w = cws[d.cw_in + c];
                            uint8_t *b = bytes + d.byte_io + (c >> 1);
                            *b = (uint8_t)(*b ^ (((w.nibble ^ w.second) & 15u) << (4u * (c & 1u))));
                        }
                }
                recs[f] = r;
            }
        }
        __syncthreads(); // the LDS is reused by the next frame of this workgroup
    }
}

int launch_soft_repair(const SoftRepairDesc *d_descs, uint32_t n_frames, uint32_t candidates, const SoftCw *d_cws, uint8_t *d_bytes, SoftRepairRec *d_recs, void *stream)
{
    if (n_frames == 0) return 0;
    if (candidates < 1u || candidates > kSoftRepairMaxCand) return -1;
    hipLaunchKernelGGL(soft_repair_kernel, dim3(n_frames < 4096u ? n_frames : 4096u), dim3(kWG), 0, (hipStream_t)stream, d_descs, n_frames, candidates, d_cws, d_bytes, d_recs);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
