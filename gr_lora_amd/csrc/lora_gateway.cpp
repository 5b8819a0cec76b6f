// lora_gateway.cpp -- the multi-SF gateway (include/lora_hip_gateway.h): one filter bank, one lora_hip_mux per decoder config.
// The filter bank runs in steps of exactly Q = LORA_HIP_GATEWAY_STEP_OUTPUTS outputs per row, whatever the caller's chunking:
// a step's input (first + Q D items) is taken from the caller's buffer where it lies there whole, and otherwise gathered on the
// device (d_pend) until it is; flush runs what is left.  So the launches, hence the rows' bits, do not depend on how the capture
// arrives.  Integer input (work_raw, work_device_raw) keeps all of that: a step read in place is converted by the filter bank's
// own staging load, a gathered item by iq_unpack_kernel on its way into d_pend, which is always cf32 - so neither the format nor a
// change of format between calls moves a step or a bit.  Every mux's batch is a multiple of Q (create rounds an automatic batch up to one), so its fill stays a multiple of Q
// (a pass resets it to 0) and a step fits; after a flush that launched no pass a step takes what room is left, once.  A step:
//   1. every mux publishes a finished pass, and has room for the step;
//   2. the filter bank stores every row into every mux's chunk (lora_hip_filterbank_run_device_rows), after each mux's
//      outstanding copies of that area (lora_mux_dev::before_write);
//   3. every mux commits what was written: its next pass waits for the filter bank, then mux_work's pass loop and latency check.
// Nothing returns to the host but frames.  DESIGN.md 4.10.2.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/lora_hip_gateway.h"
#include "../../include/lora_hip_link.h"
#include "lora_mux_dev.h"
#include "lora_iq.h"

struct lora_hip_gateway {
    lora_hip_filterbank_t *fb = nullptr;
    std::vector<int32_t> channels;
    std::vector<lora_hip_config_t> dec;
    std::vector<lora_hip_mux_t *> mux;
    int device = 0;
    long long D = 1;
    long long n_abs = 0;              // wide-band items consumed
    hipStream_t st = nullptr;         // the filter bank's stream
    hipEvent_t in_ev = nullptr, fb_ev = nullptr;
    size_t Q = LORA_HIP_GATEWAY_STEP_OUTPUTS; // outputs per row and step
    float2 *d_stage = nullptr;        // host input, uploaded in pieces of stage_cap items (of any format: sized for cf32)
    size_t stage_cap = 0;
    float2 *d_pend = nullptr;         // a step's input gathered across calls (fewer than first + Q D items)
    size_t pend_n = 0, items_in = 0;
    std::vector<void *> rows;         // n_decoders * n_channels row pointers of one step
    uint64_t fb_calls = 0;
    double fb_ms = 0.0;
    std::string err;
};

namespace {

constexpr size_t kStageItems = (size_t)1 << 22; // 32 MiB of host input per upload

lora_hip_status gfail(lora_hip_gateway *g, lora_hip_status s, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (g) g->err = buf;
    return s;
}
#define GW_TRY(g, call)                                                                                    \
    do {                                                                                                   \
        hipError_t e_ = (call);                                                                            \
        if (e_ != hipSuccess) return gfail((g), LORA_HIP_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)
#define GW_MUX(g, i, call)                                                                                 \
    do {                                                                                                   \
        lora_hip_status s_ = (call);                                                                       \
        if (s_ != LORA_HIP_OK)                                                                             \
            return gfail((g), s_, "decoder %zu (SF%u): %s", (size_t)(i), (unsigned)(g)->dec[i].sf,         \
                         lora_hip_mux_last_error((g)->mux[i]));                                            \
    } while (0)

lora_hip_status check_config(const lora_hip_gateway_config_t *cfg)
{
    if (cfg->struct_size < sizeof(lora_hip_gateway_config_t) || !cfg->decoders || !cfg->filterbank.channels ||
        cfg->filterbank.struct_size < sizeof(lora_hip_filterbank_config_t))
        return LORA_HIP_ERR_ARG;
    const lora_hip_filterbank_config_t &fb = cfg->filterbank;
    if (cfg->n_decoders < 1 || cfg->n_decoders > LORA_HIP_GATEWAY_MAX_DECODERS || cfg->flags != 0 || fb.decimation < 1)
        return LORA_HIP_ERR_BAD_CONFIG;
    const float rate = (float)(fb.samp_rate / (double)fb.decimation);
    bool seen[13] = {};
    for (uint32_t i = 0; i < cfg->n_decoders; i++) {
        const lora_hip_config_t &d = cfg->decoders[i];
        if (d.struct_size != sizeof(lora_hip_config_t)) return LORA_HIP_ERR_ARG;
        if (d.sf < 6 || d.sf > 12) return LORA_HIP_ERR_BAD_SF;
        if (d.batch_items % LORA_HIP_GATEWAY_STEP_OUTPUTS) return LORA_HIP_ERR_BAD_CONFIG;
        if (seen[d.sf] || d.cr > 4 || d.demod < 0 || d.demod > 2 || d.samp_rate != rate || d.bandwidth != fb.bandwidth || d.device != fb.device)
            return LORA_HIP_ERR_BAD_CONFIG;
        seen[d.sf] = true;
    }
    return LORA_HIP_OK;
}

// outputs per row of the next step: Q, or less where a mux's chunk has less room left (only after a flush that launched no pass)
size_t gw_step_outputs(const lora_hip_gateway *g)
{
    size_t s = g->Q;
    for (const lora_hip_mux_t *m : g->mux) s = std::min(s, lora_mux_dev::room(m));
    return s;
}

// publishes the finished passes of every mux
lora_hip_status gw_collect(lora_hip_gateway *g)
{
    for (size_t i = 0; i < g->mux.size(); i++) GW_MUX(g, i, lora_mux_dev::collect_if_done(g->mux[i]));
    return LORA_HIP_OK;
}

// one filter-bank launch over n_in items of format fmt at d_in (at most one step of outputs per row) into every mux, then the commits
lora_hip_status gw_step(lora_hip_gateway *g, const void *d_in, size_t n_in, int fmt, float scale)
{
    const size_t nch = g->channels.size(), ndec = g->mux.size();
    lora_hip_status s = gw_collect(g);
    if (s != LORA_HIP_OK) return s;
    const size_t max_out = gw_step_outputs(g); // (>= 1: a full chunk launches its pass in the commit that fills it)
    for (size_t i = 0; i < ndec; i++) {
        lora_mux_dev::rows(g->mux[i], g->rows.data() + i * nch);
        GW_MUX(g, i, lora_mux_dev::before_write(g->mux[i], g->st));
    }
    size_t no = 0;
    s = fmt == LORA_HIP_IQ_CF32 ? lora_hip_filterbank_run_device_rows(g->fb, d_in, n_in, g->rows.data(), (uint32_t)ndec, max_out, &no, g->st)
                                : lora_hip_filterbank_run_device_rows_raw(g->fb, d_in, n_in, fmt, scale, g->rows.data(), (uint32_t)ndec, max_out, &no, g->st);
    if (s != LORA_HIP_OK) return gfail(g, s, "filter bank: %s", lora_hip_filterbank_last_error(g->fb));
    GW_TRY(g, hipEventRecord(g->fb_ev, g->st));
    g->n_abs += (long long)n_in;
    if (no) { g->fb_calls++; g->fb_ms += lora_hip_filterbank_last_kernel_ms(g->fb); }
    for (size_t i = 0; i < ndec; i++) GW_MUX(g, i, lora_mux_dev::commit(g->mux[i], no, g->fb_ev));
    return LORA_HIP_OK;
}

// input items of the next whole step: up to the next output's sample, then one step of outputs times D
size_t gw_need(const lora_hip_gateway *g) { return (size_t)((g->D - g->n_abs % g->D) % g->D) + gw_step_outputs(g) * (size_t)g->D; }

// takes n items of format fmt at d_in (device, ordered on g->st); returns once nothing on g->st reads d_in any more
lora_hip_status gw_run(lora_hip_gateway *g, const void *d_in_, size_t n, int fmt, float scale)
{
    const unsigned char *d_in = (const unsigned char *)d_in_;
    const size_t ib = lora_iq::item_bytes(fmt);
    g->items_in += n;
    lora_hip_status s0 = gw_collect(g); // (a pass the latency bound launched is published without waiting for a whole step)
    if (s0 != LORA_HIP_OK) return s0;
    while (n) {
        if (!gw_step_outputs(g)) return gfail(g, LORA_HIP_ERR_INTERNAL, "a decoder's chunks are full and it launched no pass");
        const size_t need = gw_need(g);
        if (g->pend_n || n < need) { // gather
            const size_t k = std::min(n, need - g->pend_n);
            if (fmt == LORA_HIP_IQ_CF32) GW_TRY(g, hipMemcpyAsync(g->d_pend + g->pend_n, d_in, k * sizeof(float2), hipMemcpyDeviceToDevice, g->st));
            else GW_TRY(g, lora_iq::unpack_launch(d_in, k, fmt, scale, g->d_pend + g->pend_n, g->st));
            g->pend_n += k; d_in += k * ib; n -= k;
            if (g->pend_n == need) {
                const lora_hip_status s = gw_step(g, g->d_pend, need, LORA_HIP_IQ_CF32, 0.0f);
                if (s != LORA_HIP_OK) return s;
                g->pend_n = 0;
            }
        } else {
            const lora_hip_status s = gw_step(g, d_in, need, fmt, scale);
            if (s != LORA_HIP_OK) return s;
            d_in += need * ib; n -= need;
        }
    }
    GW_TRY(g, hipStreamSynchronize(g->st));
    return LORA_HIP_OK;
}

} // namespace

extern "C" {

lora_hip_status lora_hip_gateway_create(const lora_hip_gateway_config_t *cfg, lora_hip_gateway_t **out)
{
    if (!cfg || !out) return LORA_HIP_ERR_ARG;
    *out = nullptr;
    lora_hip_status s = check_config(cfg);
    if (s != LORA_HIP_OK) return s;
    auto *g = new lora_hip_gateway;
    s = lora_hip_filterbank_create(&cfg->filterbank, &g->fb); // (its own limits, then the device)
    if (s != LORA_HIP_OK) { lora_hip_gateway_destroy(g); return s; }
    g->channels.assign(cfg->filterbank.channels, cfg->filterbank.channels + cfg->filterbank.n_channels);
    g->dec.assign(cfg->decoders, cfg->decoders + cfg->n_decoders);
    g->device = cfg->filterbank.device;
    g->D = cfg->filterbank.decimation;
    g->rows.assign(g->dec.size() * g->channels.size(), nullptr);
    for (size_t i = 0; i < g->dec.size(); i++) {
        lora_hip_mux_t *m = nullptr;
        s = lora_hip_mux_create(&g->dec[i], (uint32_t)g->channels.size(), &m);
        const size_t b = s == LORA_HIP_OK ? lora_mux_dev::batch(m) : 0;
        if (s == LORA_HIP_OK && b % g->Q) { // an automatic batch that is no multiple of the step (rows at no power-of-two multiple of
                                            // the bandwidth): the next multiple instead
            lora_hip_mux_destroy(m);
            m = nullptr;
            g->dec[i].batch_items = (uint32_t)((b + g->Q - 1) / g->Q * g->Q);
            s = lora_hip_mux_create(&g->dec[i], (uint32_t)g->channels.size(), &m);
        }
        if (s != LORA_HIP_OK) { lora_hip_gateway_destroy(g); return s; }
        g->mux.push_back(m);
    }
    g->stage_cap = kStageItems;
    if (hipSetDevice(g->device) != hipSuccess || hipStreamCreateWithFlags(&g->st, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&g->in_ev, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&g->fb_ev, hipEventDisableTiming) != hipSuccess) {
        lora_hip_gateway_destroy(g);
        return LORA_HIP_ERR_HIP;
    }
    if (hipMalloc((void **)&g->d_stage, g->stage_cap * sizeof(float2)) != hipSuccess ||
        hipMalloc((void **)&g->d_pend, (g->Q + 1) * (size_t)g->D * sizeof(float2)) != hipSuccess) { lora_hip_gateway_destroy(g); return LORA_HIP_ERR_NOMEM; }
    *out = g;
    return LORA_HIP_OK;
}

void lora_hip_gateway_destroy(lora_hip_gateway_t *g)
{
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->st) (void)hipStreamSynchronize(g->st);
    for (lora_hip_mux_t *m : g->mux) lora_hip_mux_destroy(m);
    if (g->fb) lora_hip_filterbank_destroy(g->fb);
    if (g->d_stage) (void)hipFree(g->d_stage);
    if (g->d_pend) (void)hipFree(g->d_pend);
    if (g->in_ev) (void)hipEventDestroy(g->in_ev);
    if (g->fb_ev) (void)hipEventDestroy(g->fb_ev);
    if (g->st) (void)hipStreamDestroy(g->st);
    delete g;
}

const char *lora_hip_gateway_last_error(const lora_hip_gateway_t *g) { return g ? g->err.c_str() : "null handle"; }

static lora_hip_status gw_work(lora_hip_gateway_t *g, const void *iq, size_t n, int fmt, float scale)
{
    if (!g || (n && !iq)) return LORA_HIP_ERR_ARG;
    g->err.clear();
    GW_TRY(g, hipSetDevice(g->device));
    const size_t ib = lora_iq::item_bytes(fmt);
    for (size_t pos = 0; pos < n;) {
        const size_t k = std::min(n - pos, g->stage_cap); // (nothing reads the piece before any more: gw_run synchronises)
        GW_TRY(g, hipMemcpyAsync(g->d_stage, (const unsigned char *)iq + pos * ib, k * ib, hipMemcpyHostToDevice, g->st));
        const lora_hip_status s = gw_run(g, g->d_stage, k, fmt, scale);
        if (s != LORA_HIP_OK) return s;
        pos += k;
    }
    return LORA_HIP_OK;
}

static lora_hip_status gw_work_device(lora_hip_gateway_t *g, const void *d_iq, size_t n, int fmt, float scale, void *hip_stream);

// the raw entry points' own checks (include/lora_hip.h, lora_hip_iq_format)
static lora_hip_status gw_check_raw(lora_hip_gateway_t *g, const void *p, int fmt, float scale)
{
    if (!g) return LORA_HIP_ERR_ARG;
    if (!lora_iq::args_ok(p, fmt, scale)) return gfail(g, LORA_HIP_ERR_ARG, "unknown format %d, unusable scale %g, or input not aligned to its component", fmt, (double)scale);
    return LORA_HIP_OK;
}

lora_hip_status lora_hip_gateway_work(lora_hip_gateway_t *g, const float *iq, size_t n) { return gw_work(g, iq, n, LORA_HIP_IQ_CF32, 0.0f); }

lora_hip_status lora_hip_gateway_work_raw(lora_hip_gateway_t *g, const void *iq, size_t n, int fmt, float scale)
{
    const lora_hip_status s = gw_check_raw(g, iq, fmt, scale);
    return s != LORA_HIP_OK ? s : gw_work(g, iq, n, fmt, scale);
}

lora_hip_status lora_hip_gateway_work_device(lora_hip_gateway_t *g, const void *d_iq, size_t n, void *hip_stream)
{
    return gw_work_device(g, d_iq, n, LORA_HIP_IQ_CF32, 0.0f, hip_stream);
}

lora_hip_status lora_hip_gateway_work_device_raw(lora_hip_gateway_t *g, const void *d_iq, size_t n, int fmt, float scale, void *hip_stream)
{
    const lora_hip_status s = gw_check_raw(g, d_iq, fmt, scale);
    return s != LORA_HIP_OK ? s : gw_work_device(g, d_iq, n, fmt, scale, hip_stream);
}

static lora_hip_status gw_work_device(lora_hip_gateway_t *g, const void *d_iq, size_t n, int fmt, float scale, void *hip_stream)
{
    if (!g || (n && !d_iq)) return LORA_HIP_ERR_ARG;
    g->err.clear();
    if (!n) return LORA_HIP_OK;
    GW_TRY(g, hipSetDevice(g->device));
    GW_TRY(g, hipEventRecord(g->in_ev, (hipStream_t)hip_stream));
    GW_TRY(g, hipStreamWaitEvent(g->st, g->in_ev, 0));
    return gw_run(g, d_iq, n, fmt, scale);
}

lora_hip_status lora_hip_gateway_flush(lora_hip_gateway_t *g)
{
    if (!g) return LORA_HIP_ERR_ARG;
    g->err.clear();
    GW_TRY(g, hipSetDevice(g->device));
    if (g->pend_n) { // the last partial step
        const lora_hip_status s = gw_step(g, g->d_pend, g->pend_n, LORA_HIP_IQ_CF32, 0.0f);
        if (s != LORA_HIP_OK) return s;
        g->pend_n = 0;
    }
    for (size_t i = 0; i < g->mux.size(); i++) GW_MUX(g, i, lora_hip_mux_flush(g->mux[i]));
    return LORA_HIP_OK;
}

lora_hip_status lora_hip_gateway_set_latency(lora_hip_gateway_t *g, float max_latency_ms)
{
    if (!g || !(max_latency_ms >= 0.0f)) return LORA_HIP_ERR_ARG;
    for (size_t i = 0; i < g->mux.size(); i++) GW_MUX(g, i, lora_hip_mux_set_latency(g->mux[i], max_latency_ms));
    return LORA_HIP_OK;
}

size_t lora_hip_gateway_frames_available(const lora_hip_gateway_t *g)
{
    if (!g) return 0;
    size_t n = 0;
    for (const lora_hip_mux_t *m : g->mux) n += lora_hip_mux_frames_available(m);
    return n;
}

lora_hip_status lora_hip_gateway_poll_frame(lora_hip_gateway_t *g, uint8_t *buf, size_t cap, size_t *len, lora_hip_gateway_frame_info_t *info)
{
    if (!g || !len) return LORA_HIP_ERR_ARG;
    *len = 0;
    for (size_t i = 0; i < g->mux.size(); i++) {
        if (!lora_hip_mux_frames_available(g->mux[i])) continue;
        lora_hip_frame_info_t fi{};
        GW_MUX(g, i, lora_hip_mux_poll_frame(g->mux[i], buf, cap, len, &fi));
        if (info) {
            *info = lora_hip_gateway_frame_info_t{};
            info->row = fi.stream;
            info->grid_index = fi.stream < g->channels.size() ? g->channels[fi.stream] : 0;
            info->sf = g->dec[i].sf;
            info->decoder = (uint32_t)i;
            info->length = fi.length;
            info->header_pos = fi.header_pos;
            info->end_pos = fi.end_pos;
        }
        return LORA_HIP_OK;
    }
    return LORA_HIP_OK;
}

// link metrics (include/lora_hip_link.h): both only forward to every decoder's mux
lora_hip_status lora_hip_link_gateway_enable(lora_hip_gateway_t *g, int on)
{
    if (!g) return LORA_HIP_ERR_ARG;
    for (size_t i = 0; i < g->mux.size(); i++) GW_MUX(g, i, lora_hip_link_mux_enable(g->mux[i], on));
    return LORA_HIP_OK;
}

lora_hip_status lora_hip_link_gateway_poll_frame(lora_hip_gateway_t *g, uint8_t *buf, size_t cap, size_t *len, lora_hip_gateway_frame_info_t *info,
                                                 lora_hip_link_metrics_t *metrics)
{
    if (!g || !len || !metrics) return LORA_HIP_ERR_ARG;
    *len = 0;
    for (size_t i = 0; i < g->mux.size(); i++) {
        if (!lora_hip_mux_frames_available(g->mux[i])) continue;
        lora_hip_frame_info_t fi{};
        GW_MUX(g, i, lora_hip_link_mux_poll_frame(g->mux[i], buf, cap, len, &fi, metrics));
        if (info) {
            *info = lora_hip_gateway_frame_info_t{};
            info->row = fi.stream;
            info->grid_index = fi.stream < g->channels.size() ? g->channels[fi.stream] : 0;
            info->sf = g->dec[i].sf;
            info->decoder = (uint32_t)i;
            info->length = fi.length;
            info->header_pos = fi.header_pos;
            info->end_pos = fi.end_pos;
        }
        return LORA_HIP_OK;
    }
    return LORA_HIP_OK;
}

lora_hip_status lora_hip_gateway_stats(const lora_hip_gateway_t *g, lora_hip_gateway_stats_t *stats)
{
    if (!g || !stats || stats->struct_size < sizeof(lora_hip_gateway_stats_t)) return LORA_HIP_ERR_ARG;
    const uint32_t ss = stats->struct_size;
    *stats = lora_hip_gateway_stats_t{};
    stats->struct_size = ss;
    stats->n_decoders = (uint32_t)g->mux.size();
    for (size_t i = 0; i < g->mux.size(); i++) {
        const lora_hip_status s = lora_hip_mux_passes(g->mux[i], &stats->passes[i], &stats->passes_by_latency[i]);
        if (s != LORA_HIP_OK) return s;
    }
    stats->filterbank_calls = g->fb_calls;
    stats->filterbank_ms = g->fb_ms;
    stats->items_in = (uint64_t)g->items_in;
    stats->step_outputs = (uint64_t)g->Q;
    return LORA_HIP_OK;
}

} // extern "C"
