// lora_stitch.hpp -- the speculation scheduler: segments, probes and the stitch, independent of HIP.
//
// decode_streams<Env>() is instantiated twice: by lora_runtime.cpp over the real device (jobs run by the
// walker kernels) and by tests/host_sim/stitch_sim.cpp over a CPU environment whose jobs are run by the
// oracle's state machine -- so the scheduling logic is exercised by the CPU test-suite as well.
//
// Env must provide:  uint32_t sps(), ctor_cr(), segment_symbols(), resident_slots();  bool tracing(), implicit();
//   int  run_jobs(const std::vector<Job> &, uint32_t recs_per_job, uint32_t trace_cap, RunOut &);   (0 = ok; launch and wait)
//   int  run_jobs_begin(same) / run_jobs_end(RunOut &);   (the main launch of a pass, split: launch / wait and fetch)
//   RunOut &run_out(int which);   (two reusable result holders)
//   bool quiet_edges(const std::vector<StreamDesc> &, std::vector<std::vector<int64_t>> &);   (gap starts per stream, false = none)
//   void publish(const AttemptRec &, StreamDesc &);   void append_trace(const RunOut &, uint32_t job, uint32_t cap, int64_t base);
//   void count_jobs(uint32_t), count_probes(uint32_t), count_slow_path(), count_repair(), note_plan(bool burst_aware, size_t n_segments);   double walker_ms();
//   uint32_t resident_slots_alt();   (a second, smaller slot count when the kernel exists in two workgroup sizes; 0: none)
//   bool early_probe();   (the jobs record their FIND_SFD entry states and their tail probes may stop behind the first one: Job.tail_stop_sfd)
//   bool decoupled(size_t n_jobs);   (run this pass's segment jobs header-only and the payloads in the symbol-parallel payload pass)
//   void set_skip_payload(bool);     (the launches that follow run the kernels' header-only variant, LaunchCfg.skip_payload)
//   void abort_payload();   (an error return between the two calls below: wait for whatever the payload pass has in flight and forget it)
//   int  run_payload_begin(std::vector<PayloadReq> &) / run_payload_end(same);   (0 = ok; launch / wait: status, end_shift and frame of every request filled in)   void count_payload(uint32_t packets, uint32_t moved, uint32_t rerun);
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "lora_device.h"

namespace lora_hip {

// d_pwr_queue (boost::circular_buffer<float>(4)) + d_snr, kept on the host: the
// device reports the values each DETECT step pushed (:360), the host replays them.
struct PwrState {
    float q[4];
    int n = 0;
    float snr = 0.0f; // uninitialised upstream (decoder_impl.h:101); pinned to 0
    void push(float v)
    {
        if (n < 4) q[n++] = v;
        else { q[0] = q[1]; q[1] = q[2]; q[2] = q[3]; q[3] = v; }
    }
    void apply(uint32_t npush, const float tail[4])
    {
        const uint32_t k = npush < 4u ? npush : 4u;
        for (uint32_t i = 0; i < k; i++) push(tail[i]);
    }
    void determine_snr() // :377-383
    {
        if (n >= 2) snr = q[n - 1] / q[0];
    }
};

struct StreamDesc {
    uint64_t off, len;
    uint32_t id;
    uint32_t cr_in;       // d_phdr.cr carried in
    PwrState pwr;         // power queue / snr carried in
    int64_t  abs_base;    // added to reported positions
    // results: the serial decoder's state at the end of the pass.  incomplete: the data ended inside an attempt - final_pos is then the start
    // of that attempt's DETECT scan (the end of the attempt before it, or the start of the pass), cr_out the d_phdr.cr the decoder held THERE (the
    // pending attempt's cr_prev, not the CR of the header it may have decoded since) and pwr the power state there: the next pass runs the
    // attempt again from that state
    int64_t  final_pos = 0;
    uint32_t cr_out = 0;
    bool incomplete = false;
    // while a pass is stitched: where the DETECT scan the true trajectory is in began, and the power state there
    int64_t  scan_pos = 0;
    PwrState scan_pwr;
};

// What a stream carries from one pass to the next (lora_hip_work, the mux, the gateways; tests/host_sim runs the same two functions): d_phdr.cr,
// the power state, the absolute index of its next item and the items kept in front of the next chunk.
struct StreamCarry {
    size_t   tail_len = 0;  // items carried over in front of the chunk being filled
    uint32_t cr = 0;        // decoder state carried from pass to pass: d_phdr.cr, power queue,
    PwrState pwr;
    int64_t  host_base = 0; // ... and the absolute item index of the first item of the stream's next region
};

// The end of a pass: takes the decoder state; returns the item of the pass's region from which on the stream is kept (an attempt that ran out
// of data is run again from the start of its scan with the next chunk behind it)
inline size_t carry_collect(StreamCarry &c, const StreamDesc &sd)
{
    c.cr = sd.cr_out; c.pwr = sd.pwr;
    const size_t keep_from = (size_t)std::min<int64_t>(std::max<int64_t>(sd.final_pos, 0), (int64_t)sd.len);
    c.host_base += (int64_t)keep_from;
    c.tail_len = (size_t)sd.len - keep_from;
    return keep_from;
}

// The start of the next: the carried items and `fill` new ones as one stream (off and id are the caller's).  False: fewer than two symbols
// (the reference's set_output_multiple(2 * sps), decoder_impl.cc:91: work() runs only while that many items remain), the stream stays out of the pass and goes on filling.
inline bool carry_launch(const StreamCarry &c, size_t fill, uint32_t sps, StreamDesc &sd)
{
    const size_t len = c.tail_len + fill;
    if (len < 2u * (size_t)sps) return false;
    sd.len = len; sd.cr_in = c.cr; sd.pwr = c.pwr; sd.abs_base = c.host_base;
    return true;
}

// Attempt records of one launch: storage that is neither cleared nor reallocated between launches (a 58-deep
// std::vector<AttemptRec> per job would be megabytes to zero-fill and to page in on every call).
struct RecStore {
    std::unique_ptr<AttemptRec[]> p;
    size_t n = 0, cap = 0;
    AttemptRec *data() { return p.get(); }
    const AttemptRec *data() const { return p.get(); }
    AttemptRec &operator[](size_t i) { return p[i]; }
    const AttemptRec &operator[](size_t i) const { return p[i]; }
    size_t size() const { return n; }
    void clear() { n = 0; }
    void resize_uninit(size_t k) // contents undefined: the caller writes every element it later reads
    {
        if (k > cap) { p.reset(new AttemptRec[k + k / 4]); cap = k + k / 4; }
        n = k;
    }
    void assign(size_t k, const AttemptRec &v)
    {
        resize_uninit(k);
        for (size_t i = 0; i < k; i++) p[i] = v;
    }
};

struct RunOut {
    std::vector<JobResult> res;
    RecStore recs;
    uint32_t rpj = 0; // records stored per job (stride of `recs`): every record the jobs wrote, at most `cap`
    uint32_t cap = 0; // record capacity the jobs ran with
    const AttemptRec &rec(size_t job, uint32_t a) const { return recs[job * rpj + a]; }
    // attempts that ran to completion (the last one is pending when JobResult.pad is set)
    uint32_t n_done(size_t job) const
    {
        const JobResult &r = res[job];
        const uint32_t n = r.pad ? r.n_attempts - 1u : r.n_attempts;
        return n < cap ? n : cap;
    }
};

// One packet of the payload pass: a kAttemptHeaderOnly record of a header-only job, and what the pass made of it.
enum PayloadStatus : uint32_t {
    kPayloadDecoded = 0,   // frame[] is the serial decoder's; its symbols moved the symbol clock by end_shift samples in all (0: the job's scan behind it stands)
    kPayloadOutOfData = 1, // the data ends inside the payload (:91): the packet is pending
    kPayloadUnresolved = 2 // the pass gave up (too many moves of the symbol clock): the complete kernels decode it again from its header
};
struct PayloadReq {
    uint64_t stream_off, stream_len;
    int64_t  start;          // first payload symbol, relative to the stream (symbol k is read at start + k sps while nothing moves the symbol clock)
    int64_t  hdr_pos;        // (for an environment that decodes the packet from its header instead)
    uint32_t n_walk;         // symbols DECODE_PAYLOAD demodulates
    uint32_t cr_prev;
    SkippedPayload sk;
    // results
    uint32_t status;         // PayloadStatus
    int32_t  end_shift;
    uint32_t frame_len;
    uint8_t  frame[kMaxFrame + 4];
};

// A completed attempt of the TRUE trajectory: replay its DETECT pushes, take the
// SNR at the trigger (:756), publish the frame if there is one.
template <class Env>
void adopt(Env &env, const AttemptRec &r, StreamDesc &sd)
{
    sd.pwr.apply(r.npush, r.push_tail);
    sd.pwr.determine_snr();
    if (r.status == kAttemptFrame) env.publish(r, sd);
    sd.scan_pos = r.end_pos; sd.scan_pwr = sd.pwr; // the next DETECT scan begins here
}

struct Cursor { int64_t pos; uint32_t cr; }; // DETECT state between attempts: position + carried d_phdr.cr

// The record of the attempt run `job` was cut short in (JobResult.pad), or null: none pending, or its record did not fit the record capacity
// (the kernels begin no attempt without room for its record; a caller that meets it all the same adopts nothing of the run)
inline const AttemptRec *pending_rec(const RunOut &R, size_t job)
{
    const JobResult &jr = R.res[job];
    return (jr.pad && jr.n_attempts >= 1u && jr.n_attempts - 1u < R.cap) ? &R.rec(job, jr.n_attempts - 1u) : nullptr;
}
inline bool end_known(const RunOut &R, size_t job) { return !R.res[job].pad || pending_rec(R, job) != nullptr; }

// The DETECT state run `job` ended in.  With an attempt pending that is the start of the attempt and the d_phdr.cr it STARTED with (its record's
// cr_prev): JobResult.final_cr is the kernels' d_phdr.cr where they stopped, behind the pending attempt's header if it got that far, which the serial
// decoder does not hold at final_pos - resuming a stream with it decodes the packet's header on the branch of its own CR (:655).  (end_known first.)
inline Cursor end_cursor(const RunOut &R, size_t job)
{
    const JobResult &jr = R.res[job];
    const AttemptRec *p = pending_rec(R, job);
    return Cursor{jr.final_pos, p ? p->cr_prev : jr.final_cr};
}

// A job that walks stream sd from the state `from` up to `limit`; stop_at_header: a probe, which stops on entering the first header
inline Job walk_job(const StreamDesc &sd, Cursor from, int64_t limit, bool stop_at_header)
{
    Job j{};
    j.stream_off = sd.off; j.stream_len = sd.len; j.start = from.pos; j.scan_limit = limit;
    j.stream_id = sd.id; j.cr_prev = from.cr; j.max_attempts = 0; j.stop_at_header = stop_at_header ? 1u : 0u;
    return j;
}

inline bool debug_on() { static const bool on = getenv("LORA_HIP_DEBUG") != nullptr; return on; }
inline bool debug_jobs_on() { static const bool on = getenv("LORA_HIP_DEBUG_JOBS") != nullptr; return on; }

// LORA_HIP_DEBUG_JOBS: job k of a launch, its result and its records ([job]: segment jobs, [probe]: the probe launch, [serial]: serial walks),
// comparable between the device and the CPU simulation
inline void dump_job(const char *tag, size_t k, const Job &j, const RunOut &R)
{
    const JobResult &r = R.res[k];
    fprintf(stderr, "[%s] %zu start %lld limit %lld probe_limit %lld cr %u | final_pos %lld cr %u n_att %u stop %u pad %u npush %u | tail %u: first %u n_att %u final_pos %lld cr %u stop %u pad %u npush %u\n",
            tag, k, (long long)j.start, (long long)j.scan_limit, (long long)j.probe_limit, j.cr_prev, (long long)r.final_pos, r.final_cr, r.n_attempts, r.stop_reason, r.pad,
            r.npush, r.tail_valid, r.tail_first_rec, r.tail_n_attempts, (long long)r.tail_final_pos, r.tail_final_cr, r.tail_stop_reason, r.tail_pad, r.tail_npush);
    const uint32_t n = r.n_attempts + (r.tail_valid ? r.tail_n_attempts : 0u);
    for (uint32_t a = 0; a < n && a < R.cap; a++) {
        const AttemptRec &t = R.rec(k, a);
        fprintf(stderr, "[%s]    rec %u status %u start %lld trig %lld hdr %lld end %lld nsym %u npush %u cr_prev %u ambig %u len %u\n", tag, a, t.status,
                (long long)t.start_pos, (long long)t.trig_pos, (long long)t.hdr_pos, (long long)t.end_pos, t.n_symbols, t.npush, t.cr_prev, t.hdr_ambig, t.frame_len);
    }
}

inline uint32_t recs_for(uint64_t span_items, uint32_t sps)
{ // a completed packet spans >= 13 symbols, a lost-sync attempt >= 5 (+ its DETECT steps)
    return (uint32_t)std::min<uint64_t>(span_items / (5ull * sps) + 6ull, 4096ull);
}

// The truth by construction: one job from `cur` up to `limit`, everything adopted.
template <class Env>
int run_serial(Env &env, StreamDesc &sd, Cursor &cur, int64_t limit, bool tracing)
{
    while (true) {
        const std::vector<Job> jobs(1, walk_job(sd, cur, limit, false));
        const uint64_t span = (uint64_t)std::max<int64_t>(limit - cur.pos, 0);
        const uint32_t rpj = recs_for(span, env.sps());
        const uint32_t trace_cap = tracing ? (uint32_t)std::min<uint64_t>(2ull * (span / env.sps()) + 64ull, 1ull << 22) : 0u;
        RunOut out;
        int s = env.run_jobs(jobs, rpj, trace_cap, out);
        if (s != 0) return s;
        const JobResult &jr = out.res[0];
        if (debug_jobs_on()) dump_job("serial", 0, jobs[0], out);
        if (!end_known(out, 0)) { // (a pending attempt without its record: not a state to go on from, and the kernels never report one)
            if (debug_on()) fprintf(stderr, "[lora_hip] serial walk of stream %u from %lld: %u attempts, the pending one's record did not fit %u records - the decode fails\n",
                                    sd.id, (long long)cur.pos, jr.n_attempts, out.cap);
            return -1;
        }
        for (uint32_t a = 0; a < out.n_done(0); a++) adopt(env, out.rec(0, a), sd);
        if (tracing) env.append_trace(out, 0, trace_cap, sd.abs_base);
        cur = end_cursor(out, 0); // start and carried-in CR of the pending attempt when one was cut short
        if (jr.pad) { sd.incomplete = true; return 0; }
        sd.pwr.apply(jr.npush, jr.push_tail);
        if (jr.stop_reason != 2u) return 0;
    }
}

inline int cr_class(uint32_t cr) { return cr >= 3u ? 2 : (cr >= 1u ? 1 : 0); }

// The header FEC branch follows the carried-in d_phdr.cr (:655): a speculative decode of header r only stands if its branch is the true one
// (that of true_cr), or the two Hamming branches agree on this header - and class 0 (no switch case upstream: the header reads as zeros) never
// agrees with either
inline bool wrong_fec_branch(const AttemptRec &r, uint32_t true_cr)
{
    const int cj = cr_class(r.cr_prev), cl = cr_class(true_cr);
    return cj != cl && (r.hdr_ambig || cj == 0 || cl == 0);
}

// An attempt that entered DECODE_HEADER and decoded the header: a frame, a packet the data ends in, or (with_header_only) a header-only record
// whose payload the payload pass has not decoded yet
inline bool header_bearing(const AttemptRec &r, bool with_header_only)
{
    return r.hdr_pos >= 0 && (r.status == kAttemptFrame || r.status == kAttemptOutOfData || (with_header_only && r.status == kAttemptHeaderOnly));
}

// Did r START a FIND_SFD step in the state pos / fails (position and d_corr_fails)?  That is all decoder_impl.cc:785-818 read: two trajectories
// that pass through the same such state are one from that step on, header entry included.
inline bool passed_sfd_state(const AttemptRec &r, int64_t pos, uint32_t fails)
{
    for (uint32_t z = 0; z < r.n_sfd && z < (uint32_t)kMaxSfdRec; z++)
        if (r.sfd_pos[z] == pos && r.sfd_fails[z] == fails) return true;
    return false;
}

// The pending record job k's tail probe stopped with (at a header, behind its first FIND_SFD step, or out of data), or null: no tail probe, no
// attempt pending, or its record did not fit
inline const AttemptRec *tail_probe_last(const RunOut &R, size_t k)
{
    const JobResult &jr = R.res[k];
    if (!jr.tail_valid || !jr.tail_pad || jr.tail_n_attempts == 0u) return nullptr;
    const uint32_t li = std::min(jr.tail_first_rec, R.cap) + jr.tail_n_attempts - 1u;
    return li < R.cap ? &R.rec(k, li) : nullptr;
}

// Did job k's tail probe end at its first SYNC exit (kStopAtSync)?  The device has then compared positions: the first attempt of job k + 1 of the same
// launch left SYNC at the same sample, with d_corr_fails = 0 and d_fine_sync = 0 like the probe's - the FIND_SFD entry state, which is all that
// decoder_impl.cc:785-818 read.  From there on that attempt IS the true trajectory: its FIND_SFD steps, its header entry (or its loss of sync), all
// that follows.  What the two do not share lies outside the kernels' comparison and is checked here as for any probe: d_phdr.cr, which picks the
// header's FEC branch (wrong_fec_branch; the probe's pending record carries the true one), and the power queue, which only DETECT steps push to
// (:360) - every push of the true scan precedes the probe's SYNC exit and is in its record, FIND_SFD and PAUSE push nothing.
inline bool tail_at_sync(const RunOut &R, size_t k)
{
    const JobResult &jr = R.res[k];
    return jr.tail_valid && jr.tail_pad && jr.tail_stop_reason == kStopAtSync;
}
// ... and the record of the successor job `succ` such a probe is merged with: its first, if that went on into a header (0), else -1 (the attempt lost
// sync: what follows it depends on nothing but the position, but its later headers are decoded under the job's own d_phdr.cr - left to a probe)
inline int sync_stop_match(const RunOut &R, size_t succ, bool with_header_only)
{
    return (R.res[succ].n_attempts >= 1u && R.cap >= 1u && R.rpj >= 1u && header_bearing(R.rec(succ, 0), with_header_only)) ? 0 : -1;
}

// The first of job k's completed or pending records that satisfies pred, or -1
template <class Pred>
int find_record(const RunOut &R, size_t k, Pred pred)
{
    const uint32_t nall = std::min(R.res[k].n_attempts, R.cap);
    for (uint32_t a = 0; a < nall; a++)
        if (pred(R.rec(k, a))) return (int)a;
    return -1;
}

// Does a header-bearing attempt (header-only records included) of a segment job in (first, target] satisfy pred?
template <class Pred>
bool any_segment_record(const RunOut &R, size_t first, size_t target, Pred pred)
{
    for (size_t k = first + 1; k <= target; k++)
        if (find_record(R, k, [&](const AttemptRec &r) { return header_bearing(r, true) && pred(r); }) >= 0) return true;
    return false;
}

// Burst-aware segment plan.  `edges[i]` holds the positions where stream i goes quiet (the start of every gap between
// bursts, ascending).  Cuts are placed only at such positions and chosen greedily so that every segment carries about
// the same load (items plus a fixed acquisition cost per burst) and the whole plan is at most `slots` segments: one
// resident wave of workgroups, each with the same number of packets.  Compared with the fixed grid this removes the
// spread between jobs that happen to hold one packet more than their neighbours, the scan from a cut in mid-packet
// to the next preamble, and the failed attempt on the truncated packet.  Returns false (fixed grid) when the streams
// do not look like dense burst traffic.  Only where the cuts are changes, never what is decoded.
inline bool plan_burst_segments(const std::vector<StreamDesc> &streams, const std::vector<std::vector<int64_t>> &edges, uint32_t sps,
                                uint32_t slots, uint64_t nominal, std::vector<std::vector<int64_t>> &cuts)
{
    if (edges.size() != streams.size() || slots == 0) return false;
    size_t n_edges = 0;
    for (const auto &e : edges) n_edges += e.size();
    if (n_edges < slots) return false;                       // fewer bursts than workgroups: the fixed grid spreads the scan better
    const int64_t acq = 40ll * sps;                          // DETECT + SYNC + FIND_SFD of one packet, in items of payload work
    auto weight = [&](const std::vector<int64_t> &e, size_t k, int64_t len) { // burst k (up to its gap), k == size(): the rest
        const int64_t a = k ? e[k - 1] : 0;
        return k < e.size() ? (e[k] - a) + acq : len - a;
    };
    double total = 0;
    for (size_t i = 0; i < streams.size(); i++)
        for (size_t k = 0; k <= edges[i].size(); k++) total += (double)weight(edges[i], k, (int64_t)streams[i].len);
    double target = total / slots;
    for (int attempt = 0; attempt < 12; attempt++, target *= 1.07) {
        size_t n_segs = 0;
        cuts.assign(streams.size(), {});
        for (size_t i = 0; i < streams.size(); i++) {
            const std::vector<int64_t> &e = edges[i];
            const int64_t len = (int64_t)streams[i].len;
            double acc = 0;
            for (size_t k = 0; k < e.size(); k++) {
                acc += (double)weight(e, k, len);
                if (acc >= target - 0.5 * (double)weight(e, k + 1, len) && len - e[k] > 8ll * sps && e[k] > (cuts[i].empty() ? 0 : cuts[i].back())) {
                    cuts[i].push_back(e[k]);
                    acc = 0;
                }
            }
            // stretches without a gap (back-to-back or weak packets): fall back to the grid inside them
            std::vector<int64_t> c;
            int64_t prev = 0;
            for (size_t k = 0; k <= cuts[i].size(); k++) {
                const int64_t b = k < cuts[i].size() ? cuts[i][k] : len;
                if ((uint64_t)(b - prev) > 3u * nominal) {
                    const uint64_t parts = ((uint64_t)(b - prev) + 2u * nominal - 1u) / (2u * nominal);
                    for (uint64_t q = 1; q < parts; q++) c.push_back(prev + (int64_t)((uint64_t)(b - prev) * q / parts));
                }
                if (k < cuts[i].size()) c.push_back(b);
                prev = b;
            }
            cuts[i].swap(c);
            n_segs += cuts[i].size() + 1u;
        }
        if (n_segs <= slots) return true;
    }
    return false;
}

// Decodes a set of independent streams.
//
// Every stream is cut into fixed segments.  Round 1 runs one walker job per
// segment, each starting in DETECT at its segment boundary (a guess: the true
// decoder arrives there with some other window phase and possibly mid-packet).
// Round 2 is, for every segment, a probe that starts from the END state of the
// preceding segment's job and walks DETECT/SYNC/FIND_SFD up to the first header.
// Normally the preceding job has run it itself (Job.probe_limit: having reached its
// own limit the workgroup runs that probe as a second phase and reports it as its
// "tail"); a separate probe job is launched only where no such tail exists
// (header-less segments in between, kernels without the feature).
// The host then stitches: if the probe enters DECODE_HEADER at the same sample
// as one of the segment job's attempts, the two trajectories are identical from
// there on (the decoder state at header entry is position + d_phdr.cr), and the
// job's remaining attempts are the true ones.  Anything else is re-run serially
// from the true state.  The result is exactly the serial state machine's.
struct Seg { uint32_t stream; int64_t b0, b1; };

// What the first half of a pass (plan + main launch, decode_begin) hands to the second (decode_end: results, probes,
// stitch).  The two halves exist so that a caller can put another pass's launch between them: while the device runs
// one batch the host plans the next and stitches the previous.
struct PassCtx {
    std::vector<Seg> segs;
    std::vector<size_t> first_seg;
    std::vector<Job> jobs;
    uint32_t rpj1 = 0, rpj2 = 8, trace_cap = 0;
    bool segmenting = false, tracing = false, launched = false;
    bool decoupled = false;  // the segment jobs run header-only (LaunchCfg.skip_payload), payload_round() decodes the payloads
    std::chrono::steady_clock::time_point tp_in, tp0;
};

template <class Env>
int decode_begin(Env &env, std::vector<StreamDesc> &streams, PassCtx &ctx)
{
    const uint32_t sps = env.sps();
    const bool tracing = env.tracing();
    ctx = PassCtx{};
    ctx.tp_in = std::chrono::steady_clock::now();
    uint64_t total = 0;
    for (const StreamDesc &sd : streams) total += sd.len;
    // auto: as many segments as workgroups fit on the device at once (one wave of workgroups per launch;
    // kernel time is ceil(jobs / resident slots) x job latency), never shorter than 64 symbols
    const uint32_t slots = env.resident_slots();
    const uint64_t want_jobs = std::max<uint64_t>(slots - slots / 16u, (uint64_t)streams.size());
    uint64_t seg = env.segment_symbols() ? (uint64_t)env.segment_symbols() * sps
                                          : std::max<uint64_t>(64ull * sps, (total + want_jobs - 1) / want_jobs);
    if (seg < 16ull * sps) seg = 16ull * sps;
    const bool segmenting = !tracing && !env.implicit();
    ctx.segmenting = segmenting; ctx.tracing = tracing;

    // auto mode on a batch worth cutting up: look for the gaps between bursts and plan the cuts around them
    std::vector<std::vector<int64_t>> cuts;
    bool planned = false, balanced = false; // balanced: plan_burst_segments' plan - at least as many bursts as workgroups, every job whole packets
    static const bool no_plan = getenv("LORA_HIP_NO_BURST_PLAN") != nullptr;
    if (segmenting && env.segment_symbols() == 0 && !no_plan && total > 2ull * seg) {
        std::vector<std::vector<int64_t>> edges;
        if (env.quiet_edges(streams, edges)) {
            // a pass that will run decoupled wants one job per burst: header-only jobs cost an acquisition and a header each, whatever the packet's
            // length, so nothing is gained by balancing them - and cuts at the gaps need no explicit probes (plan_burst_segments refuses with fewer
            // bursts than workgroups, which is exactly when a pass is decoupled)
            if (env.decoupled(1)) {
                size_t nb = streams.size();
                for (const auto &e : edges) nb += e.size();
                if (edges.size() == streams.size() && env.decoupled(nb)) {
                    // ... and stretches without a gap (back-to-back packets) are cut on the grid, as plan_burst_segments does
                    cuts.assign(streams.size(), {});
                    size_t n_segs = 0;
                    for (size_t i = 0; i < streams.size(); i++) {
                        int64_t prev = 0;
                        constexpr uint64_t dsym = 24u; // (config 4 at 2 s per pass: 24 symbols 48.0 Gsamples/s, 32: 46.1, 16: 38.3 - the scan for preambles is what a header-only job spends most of its time on, and short segments spread it over the idle CUs)
                        const uint64_t dseg = std::max<uint64_t>(dsym, 8u) * sps;
                        auto grid_to = [&](int64_t b) {
                            if (2u * (uint64_t)(b - prev) > 3u * dseg) {
                                const uint64_t parts = ((uint64_t)(b - prev) + dseg - 1u) / dseg;
                                for (uint64_t q = 1; q < parts; q++) cuts[i].push_back(prev + (int64_t)((uint64_t)(b - prev) * q / parts));
                            }
                        };
                        for (int64_t c : edges[i]) {
                            if (!(c > prev && (int64_t)streams[i].len - c > 8ll * sps)) continue;
                            grid_to(c);
                            cuts[i].push_back(c);
                            prev = c;
                        }
                        grid_to((int64_t)streams[i].len);
                        n_segs += cuts[i].size() + 1u;
                    }
                    planned = env.decoupled(n_segs);
                    if (!planned) cuts.clear();
                }
            }
            if (!planned) balanced = planned = plan_burst_segments(streams, edges, sps, slots, seg, cuts);
            // fewer bursts than slots, but the kernel also exists with half as many, larger workgroups (walker3 SF9 / SF10 as one or two per CU):
            // one wave of those
            const uint32_t alt = env.resident_slots_alt();
            if (!planned && alt && alt < slots) {
                const uint64_t seg_alt = std::max<uint64_t>(64ull * sps, (total + alt - alt / 16u - 1) / (alt - alt / 16u));
                balanced = planned = plan_burst_segments(streams, edges, sps, alt, seg_alt, cuts);
            }
        }
    }

    // the fixed grid (no burst-aware plan) is sized for the LARGER workgroups where the kernel exists in two sizes: its jobs start inside packets, and
    // each pays a scan to the next preamble, an acquisition and a tail probe - twice as many jobs cost more than two workgroups per CU give back
    // (BASELINE config 4, 32 s per pass: 11.7 % of HBM peak with 244 jobs against 10.8 % with 484)
    if (!planned && segmenting && env.segment_symbols() == 0 && env.resident_slots_alt() && env.resident_slots_alt() < slots) {
        const uint32_t alt = env.resident_slots_alt();
        const uint64_t wj = std::max<uint64_t>(alt - alt / 16u, (uint64_t)streams.size());
        seg = std::max<uint64_t>(64ull * sps, (total + wj - 1) / wj);
    }
    std::vector<Seg> &segs = ctx.segs;
    std::vector<size_t> &first_seg = ctx.first_seg;
    first_seg.assign(streams.size() + 1, 0);
    for (size_t i = 0; i < streams.size(); i++) {
        first_seg[i] = segs.size();
        StreamDesc &sd = streams[i];
        sd.cr_out = sd.cr_in; sd.final_pos = 0; sd.incomplete = false;
        if (planned) { // burst-aware cuts
            int64_t prev = 0;
            for (int64_t c : cuts[i]) { segs.push_back(Seg{(uint32_t)i, prev, c}); prev = c; }
            segs.push_back(Seg{(uint32_t)i, prev, (int64_t)sd.len});
            continue;
        }
        uint64_t n = 1;
        if (segmenting && sd.len > seg + seg / 2) n = (sd.len + seg - 1) / seg;
        for (uint64_t k = 0; k < n; k++)
            segs.push_back(Seg{(uint32_t)i, (int64_t)(k * seg), (k + 1 == n) ? (int64_t)sd.len : (int64_t)((k + 1) * seg)});
    }
    first_seg[streams.size()] = segs.size();
    if (segs.empty()) return 0;
    env.note_plan(planned, segs.size());

    // ---- round 1: every segment speculatively
    std::vector<Job> &jobs = ctx.jobs;
    jobs.assign(segs.size(), Job{});
    // Decoupled pass: the jobs stop behind every header and skip the payload, whose symbols the payload pass demodulates all at once.  It pays
    // wherever the ordinary pass leaves the device short of work or makes it do work twice: few packets (a packet's symbols are a serial chain on ONE
    // CU, the others idle), or continuous traffic cut on the grid (every job first scans the rest of a packet another job decodes).  It does not pay
    // for the balanced plan - bursty traffic with at least a burst per workgroup, every job whole packets: there all CUs demodulate payload already
    // (BASELINE config 3, 256 packets: SF9 -8 %, SF12 -1 % decoupled; config 4: +100 % at 4 s per pass, +40 % at 8 s, +14 % at 32 s).
    ctx.decoupled = segmenting && !balanced && env.decoupled(jobs.size());

    uint64_t max_span = 0;
    for (size_t k = 0; k < segs.size(); k++) {
        const StreamDesc &sd = streams[segs[k].stream];
        Job &j = jobs[k];
        j = walk_job(sd, Cursor{segs[k].b0, (k == first_seg[segs[k].stream]) ? sd.cr_in : env.ctor_cr()}, segs[k].b1, false);
        // tail probe: past its own limit the job continues as the next segment's probe (same limit an explicit probe gets)
        const bool has_next = k + 1 < segs.size() && segs[k + 1].stream == segs[k].stream;
        static const bool no_tail = getenv("LORA_HIP_NO_TAIL") != nullptr; // diagnostics: separate probe jobs, as the generic kernels need
        // (a decoupled pass probes in a launch of its own: it runs beside the payload pass, on CUs that would idle, instead of lengthening every
        // header-only job by a second acquisition - config 4 at 2 s per pass 49.4 -> 54.0 Gsamples/s, at 8 s the same either way)
        j.probe_limit = (segmenting && has_next && !no_tail && !ctx.decoupled) ? std::min<int64_t>((int64_t)sd.len, segs[k + 1].b1 + 16ll * sps) : 0;
        j.tail_stop_sfd = (j.probe_limit && env.early_probe()) ? 1u : 0u;
        // the job whose first SYNC exit the tail probe may end on (kStopAtSync): the next segment's, job k + 1 of THIS launch - copies of the job that run in
        // other launches (re-runs, repairs) drop it.  Kernels without the early stop, and launches without LaunchCfg.sync_pos, ignore it
        j.sync_succ = (j.probe_limit && !j.tail_stop_sfd) ? (uint32_t)(k + 2u) : 0u;
        max_span = std::max<uint64_t>(max_span, (uint64_t)(segs[k].b1 - segs[k].b0));
    }
    ctx.rpj1 = recs_for(max_span, sps) + (segmenting ? ctx.rpj2 : 0u);
    ctx.trace_cap = tracing ? (uint32_t)std::min<uint64_t>(2ull * (max_span / sps) + 64ull, 1ull << 22) : 0u;
    env.count_jobs((uint32_t)jobs.size());
    env.set_skip_payload(ctx.decoupled);
    ctx.tp0 = std::chrono::steady_clock::now();
    const int s = env.run_jobs_begin(jobs, ctx.rpj1, ctx.trace_cap, env.run_out(0)); // (result holders are kept by the environment between calls)
    if (s != 0) return s;
    ctx.launched = true;
    return 0;
}

// The payload round of a decoupled pass.  Every kAttemptHeaderOnly record of the segment jobs goes through the payload pass (env.run_payload), which
// returns the packet's frame and by how many samples its symbols moved the symbol clock in all.
//  * Not at all: the record becomes the frame (kAttemptFrame); the job's scan behind it - started where the payload ends under that very assumption -
//    stands.
//  * By some samples: the frame stands, the scan behind it started beside the true position.  That is the situation at every segment boundary, and it
//    is handled the same way: the job is split there into two - the second half's records are a speculation like any later segment's, and a probe from
//    the TRUE end of the packet decides whether the true trajectory enters one of its headers (it does when SYNC / FIND_SFD pull both onto the next
//    preamble, as they do for a few samples' difference).
//  * The data ends inside the payload: the packet is pending, the job ends there.
//  * Unresolved: the rest of the job is run again from that packet's header by the complete kernels (Job.start_at_header, same limits, same tail
//    probe), all such jobs in one launch, and spliced in.
// What the stitch then sees are ordinary records, jobs and segments.
// (In two halves, so that the pass's explicit probes run while the device works on the payloads: payload_begin hands the requests to the payload
// pass and returns; payload_end takes the results and re-lays the pass.  It returns 1 when jobs were split, cut short or run again - the probes
// planned meanwhile are then planned again.)
struct PayloadRound {
    struct Ref { size_t k; uint32_t a; };
    std::vector<Ref> refs;
    std::vector<PayloadReq> reqs;
    bool open = false;
};

template <class Env>
int payload_begin(Env &env, const std::vector<StreamDesc> &streams, const PassCtx &ctx, const RunOut &R1, PayloadRound &pr)
{
    const uint32_t sps = env.sps();
    typedef PayloadRound::Ref Ref;
    std::vector<Ref> &refs = pr.refs;
    std::vector<PayloadReq> &reqs = pr.reqs;
    refs.clear(); reqs.clear(); pr.open = false;
    for (size_t k = 0; k < ctx.jobs.size(); k++) {
        const uint32_t nall = std::min(std::min(R1.res[k].n_attempts, R1.cap), R1.rpj);
        const StreamDesc &sd = streams[ctx.segs[k].stream];
        for (uint32_t a = 0; a < nall; a++) {
            const AttemptRec &r = R1.rec(k, a);
            if (r.status != kAttemptHeaderOnly) continue;
            PayloadReq q{};
            std::memcpy(&q.sk, r.frame, sizeof q.sk);
            q.n_walk = (uint32_t)(q.sk.payload_symbols > 0 ? q.sk.payload_symbols : 1);
            q.stream_off = sd.off; q.stream_len = sd.len;
            q.start = r.end_pos - (int64_t)q.n_walk * (int64_t)sps;
            q.hdr_pos = r.hdr_pos; q.cr_prev = r.cr_prev;
            refs.push_back(Ref{k, a});
            reqs.push_back(q);
        }
    }
    if (reqs.empty()) return 0;
    pr.open = true;
    return env.run_payload_begin(reqs);
}

template <class Env>
int payload_end(Env &env, const std::vector<StreamDesc> &streams, PassCtx &ctx, RunOut &R1, PayloadRound &pr)
{
    if (!pr.open) return 0;
    pr.open = false;
    typedef PayloadRound::Ref Ref;
    std::vector<Ref> &refs = pr.refs;
    std::vector<PayloadReq> &reqs = pr.reqs;
    int s = env.run_payload_end(reqs);
    if (s != 0) return s < 0 ? s : -1;

    // in place: frames and true end positions; per job, where it is split and where it ends early
    struct Plan { std::vector<uint32_t> split; int term = -1; uint32_t term_kind = 0; }; // split: behind these attempts; term: the job ends with this attempt (1 pending, 2 run again)
    std::vector<Plan> plan(ctx.jobs.size());
    uint32_t n_moved = 0, n_rerun = 0, n_pending = 0;
    for (size_t i = 0; i < reqs.size(); i++) {
        const size_t k = refs[i].k;
        Plan &pl = plan[k];
        if (pl.term >= 0) continue; // behind the attempt this job ends with
        AttemptRec &r = R1.recs[k * R1.rpj + refs[i].a];
        const PayloadReq &q = reqs[i];
        if (q.status == kPayloadDecoded) {
            r.status = kAttemptFrame;
            r.frame_len = q.frame_len;
            std::memcpy(r.frame, q.frame, std::min<size_t>(q.frame_len, sizeof r.frame));
            r.n_symbols += q.n_walk;
            r.end_pos += q.end_shift;
            if (q.end_shift != 0) { pl.split.push_back(refs[i].a); n_moved++; }
        } else {
            pl.term = (int)refs[i].a; pl.term_kind = q.status == kPayloadOutOfData ? 1u : 2u;
            if (pl.term_kind == 1u) n_pending++; else n_rerun++;
        }
    }
    env.count_payload((uint32_t)reqs.size(), n_moved, n_rerun);
    if (n_moved == 0 && n_rerun == 0 && n_pending == 0) return 0;

    // jobs to run again (complete kernels), one launch
    std::vector<Job> rjobs; // (in job order: the re-lay below takes their results in the same order)
    for (size_t k = 0; k < plan.size(); k++) {
        if (plan[k].term < 0 || plan[k].term_kind != 2u) continue;
        const AttemptRec &r = R1.rec(k, (uint32_t)plan[k].term);
        Job j = ctx.jobs[k];
        j.start = r.hdr_pos; j.start_at_header = 1; j.cr_prev = r.cr_prev; j.sync_succ = 0;
        rjobs.push_back(j);
    }
    RunOut &R3 = env.run_out(1);
    R3.res.clear(); R3.recs.clear();
    if (!rjobs.empty()) {
        env.set_skip_payload(false);
        s = env.run_jobs(rjobs, ctx.rpj1, 0, R3);
        if (s != 0) return s;
    }

    // the pass re-laid: every job cut into its pieces
    struct Row { JobResult res; std::vector<AttemptRec> recs; };
    std::vector<Seg> nsegs;
    std::vector<Job> njobs;
    std::vector<Row> nrows;
    std::vector<size_t> nfirst(streams.size() + 1, 0);
    size_t rq = 0;
    for (size_t i = 0; i < streams.size(); i++) {
        nfirst[i] = nsegs.size();
        for (size_t k = ctx.first_seg[i]; k < ctx.first_seg[i + 1]; k++) {
            const Plan &pl = plan[k];
            const JobResult &jr = R1.res[k];
            const uint32_t n_rows = std::min(std::min(jr.n_attempts + (jr.tail_valid ? jr.tail_n_attempts : 0u), R1.cap), R1.rpj);
            uint32_t lo = 0;
            int64_t b0 = ctx.segs[k].b0;
            std::vector<uint32_t> cuts;
            for (uint32_t a : pl.split) if (pl.term < 0 || (int)a < pl.term) cuts.push_back(a);
            for (size_t c = 0; c <= cuts.size(); c++) {
                const bool last = c == cuts.size();
                Row row;
                Job j = ctx.jobs[k];
                Seg sg = ctx.segs[k];
                j.start = b0; sg.b0 = b0;
                if (!last) { // [lo, cuts[c]]: ends with a packet that moved the symbol clock; the scan behind it becomes the next piece
                    const uint32_t hi = cuts[c];
                    const AttemptRec &e = R1.rec(k, hi);
                    int32_t shift = 0;
                    for (size_t t = 0; t < reqs.size(); t++) if (refs[t].k == k && refs[t].a == hi) shift = reqs[t].end_shift;
                    const int64_t assumed_end = e.end_pos - shift;
                    for (uint32_t a = lo; a <= hi; a++) row.recs.push_back(R1.rec(k, a));
                    row.res = JobResult{};
                    row.res.final_pos = e.end_pos; row.res.n_attempts = hi - lo + 1u; row.res.final_cr = (uint32_t)e.frame[1] >> 5;
                    row.res.stop_reason = 0; row.res.pad = 0; row.res.npush = 0; row.res.tail_valid = 0;
                    j.scan_limit = assumed_end; j.probe_limit = 0; j.tail_stop_sfd = 0;
                    sg.b1 = assumed_end;
                    b0 = assumed_end; lo = hi + 1u;
                } else if (pl.term >= 0 && pl.term_kind == 1u) { // ends with a pending packet
                    const uint32_t hi = (uint32_t)pl.term;
                    for (uint32_t a = lo; a <= hi; a++) row.recs.push_back(R1.rec(k, a));
                    AttemptRec &e = row.recs.back();
                    e.status = kAttemptOutOfData; e.frame_len = 0;
                    row.res = JobResult{};
                    row.res.final_pos = e.start_pos; row.res.n_attempts = hi - lo + 1u; row.res.final_cr = (uint32_t)e.frame[1] >> 5;
                    row.res.stop_reason = 1; row.res.pad = 1; row.res.npush = 0; row.res.tail_valid = 0;
                } else if (pl.term >= 0) { // ends with the re-run: the packet (its scan and acquisition are the original attempt's) and whatever the complete kernels found behind it
                    const uint32_t hi = (uint32_t)pl.term;
                    for (uint32_t a = lo; a < hi; a++) row.recs.push_back(R1.rec(k, a));
                    JobResult nr = R3.res[rq];
                    const uint32_t n_new = std::min(nr.n_attempts + (nr.tail_valid ? nr.tail_n_attempts : 0u), R3.rpj);
                    const AttemptRec &old = R1.rec(k, hi);
                    for (uint32_t t = 0; t < n_new; t++) row.recs.push_back(R3.rec(rq, t));
                    if (nr.n_attempts >= 1u && n_new >= 1u) {
                        AttemptRec &m = row.recs[hi - lo];
                        m.start_pos = old.start_pos; m.trig_pos = old.trig_pos; m.npush = old.npush;
                        for (int t = 0; t < 4; t++) m.push_tail[t] = old.push_tail[t];
                        m.n_sfd = old.n_sfd;
                        for (int t = 0; t < kMaxSfdRec; t++) { m.sfd_pos[t] = old.sfd_pos[t]; m.sfd_fails[t] = old.sfd_fails[t]; }
                        if (nr.pad && nr.n_attempts == 1u) nr.final_pos = old.start_pos; // pending: the stream resumes at the start of this attempt's scan
                    }
                    nr.n_attempts += hi - lo;
                    nr.tail_first_rec += hi - lo;
                    row.res = nr;
                    rq++;
                } else { // the rest of the job as it ran
                    for (uint32_t a = lo; a < n_rows; a++) row.recs.push_back(R1.rec(k, a));
                    row.res = jr;
                    row.res.n_attempts = jr.n_attempts >= lo ? jr.n_attempts - lo : 0u;
                    row.res.tail_first_rec = jr.tail_first_rec >= lo ? jr.tail_first_rec - lo : 0u;
                }
                nsegs.push_back(sg);
                njobs.push_back(j);
                nrows.push_back(std::move(row));
            }
        }
    }
    nfirst[streams.size()] = nsegs.size();
    uint32_t stride = 1;
    for (const Row &r : nrows) stride = std::max<uint32_t>(stride, (uint32_t)r.recs.size());
    R1.res.resize(nrows.size());
    R1.recs.resize_uninit(nrows.size() * (size_t)stride);
    R1.rpj = stride; R1.cap = std::max(R1.cap, stride);
    for (size_t k = 0; k < nrows.size(); k++) {
        R1.res[k] = nrows[k].res;
        for (size_t a = 0; a < nrows[k].recs.size(); a++) R1.recs[k * stride + a] = nrows[k].recs[a];
    }
    ctx.segs.swap(nsegs); ctx.jobs.swap(njobs); ctx.first_seg.swap(nfirst);
    return 1;
}

// ---- decode_end's phases: round 1b, probe planning and the repairs, probe views, the stitch of one stream

// One probe per segment whose own job reached a header (and one for a header-less tail): it starts from the end state of the previous header-bearing
// job.  job: index into the probe launch, or -1 with tail_of = the segment job whose tail probe it is.  rep_out / rep_job: the repair that runs the rest
// of the target segment again from the probe's header, if one was planned (the launch it ran in and its index there).
struct Probe {
    uint32_t stream; size_t target; Cursor start; int job; int tail_of;
    const RunOut *rep_out; size_t rep_job;
};

struct ProbePlan {
    std::vector<Probe> probes;
    std::vector<size_t> first_probe; // per stream, and the end
    std::vector<Job> jobs;           // the probe launch: explicit probes, tail probes promoted to explicit ones, the tail probes' repairs
    uint32_t rpj = 0;                // the probe launch's record capacity
};

// ---- round 1b: segment jobs that guessed the wrong header FEC branch.  A later segment's job runs with the constructor's d_phdr.cr; the true
// one is its predecessor's last header's (:655).  Where the two are of different Hamming classes AND the two decodes of the job's first header
// disagree (bit errors: hdr_ambig), its frames are not the true decoder's - at CR 4/5 / 4/6 under noise that is most packets - and used to cost
// one serial launch per segment (32 ms for 16 of SF12's 256 packets).  The predecessor's tail probe has already reported the true value
// (cr_prev of its pending record): all such jobs are run again, together, with it, and take their originals' place before anything is
// stitched.  (The choice is checked like any other speculation: the stitch compares branch classes again.)
template <class Env>
int rerun_wrong_branch(Env &env, const std::vector<StreamDesc> &streams, const PassCtx &ctx, RunOut &R1)
{
    std::vector<Job> rjobs;
    std::vector<size_t> rk;
    for (size_t i = 0; i < streams.size(); i++) {
        for (size_t k = ctx.first_seg[i] + 1; k < ctx.first_seg[i + 1]; k++) {
            const AttemptRec *L = tail_probe_last(R1, k - 1);
            const bool at_sync = L && tail_at_sync(R1, k - 1);
            if (!L || (!at_sync && L->status != kAttemptAtHeader && L->status != kAttemptAtSfd)) continue;
            const bool at_sfd = !at_sync && L->status == kAttemptAtSfd;
            if (at_sfd && L->n_sfd == 0u) continue;
            // the job's first header-bearing attempt on the probe's trajectory (a probe that ended at SYNC: the job's first attempt)
            const int a = at_sync ? sync_stop_match(R1, k, true) : find_record(R1, k, [&](const AttemptRec &r) {
                return header_bearing(r, true) && (at_sfd ? passed_sfd_state(r, L->sfd_pos[L->n_sfd - 1u], L->sfd_fails[L->n_sfd - 1u]) : r.hdr_pos == L->hdr_pos);
            });
            if (a < 0 || !wrong_fec_branch(R1.rec(k, (uint32_t)a), L->cr_prev)) continue;
            Job j = ctx.jobs[k];
            j.cr_prev = L->cr_prev; j.sync_succ = 0;
            rjobs.push_back(j);
            rk.push_back(k);
        }
    }
    if (rjobs.empty()) return 0;
    RunOut &R3 = env.run_out(1);
    R3.res.clear(); R3.recs.clear();
    env.count_slow_path();
    env.set_skip_payload(ctx.decoupled);
    const int s = env.run_jobs(rjobs, ctx.rpj1, 0, R3);
    if (s != 0) return s;
    for (size_t q = 0; q < rk.size(); q++) {
        const JobResult &nr = R3.res[q];
        const uint32_t n = nr.n_attempts + (nr.tail_valid ? nr.tail_n_attempts : 0u);
        if (n > R1.rpj || n > R3.cap) continue; // (does not fit the original's row: the original stands, the stitch falls back)
        R1.res[rk[q]] = nr;
        for (uint32_t a = 0; a < n; a++) R1.recs[rk[q] * R1.rpj + a] = R3.rec(q, a);
    }
    if (debug_on()) fprintf(stderr, "[lora_hip] %zu segment job(s) run again with the header FEC branch their predecessor's tail probe reported\n", rjobs.size());
    return 0;
}

// The one repair planner.  L: the record probe `pb` stopped with.  With any noise over the stream detect_upchirp's tie between adjacent shifts is
// decided by the noise, differently for two DETECT alignments: the speculative job then sits ONE sample beside the true trajectory, at about every
// second cut.  Walking such a segment serially, one workgroup at a time, is what a pass would then spend its time on (round 6: 263 -> 5 Gsamples/s
// at a noise floor 60 dB down); instead, where the probe reached a header NO segment job of its chain entered at the same sample, the REST of the
// target segment's job is run again from the true header - Job.start_at_header, the true d_phdr.cr, the job's own limits and tail probe.  The stitch adopts a repair's records as the true trajectory (which they
// are); where its end state is the speculative job's - fine_sync pulls the two together within a packet - the chain goes on, else the next cut's
// check falls back as before.  Appends the repair to `launch`, which runs into `out`; false: nothing to repair.
inline bool plan_repair(const PassCtx &ctx, const RunOut &R1, const StreamDesc &sd, const AttemptRec &L, Probe &pb, std::vector<Job> &launch,
                        const RunOut &out)
{
    if (L.status != kAttemptAtHeader || L.hdr_pos < 0) return false;
    // (header-only records count: a decoupled pass ahead of its payload_end.  Where a job did enter it, the stitch's own match - with its
    // FEC-branch condition - decides)
    if (any_segment_record(R1, ctx.first_seg[pb.stream], pb.target, [&](const AttemptRec &r) { return r.hdr_pos == L.hdr_pos; })) return false;
    const Job &target = ctx.jobs[pb.target];
    Job j = walk_job(sd, Cursor{L.hdr_pos, L.cr_prev}, target.scan_limit, false);
    j.start_at_header = 1; j.probe_limit = target.probe_limit;
    pb.rep_out = &out;
    pb.rep_job = launch.size();
    launch.push_back(j);
    return true;
}

// ---- round 2: the probes of a pass and the jobs of its probe launch, planned on R1 as it stands.  repair: plan repairs and whole-segment probes
// (not under tracing or LORA_HIP_NO_REPAIR); R2: where the probe launch will put its results.
inline void plan_probes(uint32_t sps, const std::vector<StreamDesc> &streams, const PassCtx &ctx, const RunOut &R1, const RunOut &R2, bool repair,
                        ProbePlan &plan)
{
    const std::vector<Seg> &segs = ctx.segs;
    std::vector<Probe> &probes = plan.probes;
    probes.clear(); plan.jobs.clear();
    plan.first_probe.assign(streams.size() + 1, 0);
    auto has_header = [&](size_t k) { return find_record(R1, k, [](const AttemptRec &r) { return header_bearing(r, true); }) >= 0; };
    auto job_ok = [&](size_t k) { return !R1.res[k].pad && R1.res[k].stop_reason != 2u; };
    // Probes along the speculative chain.  Only segments whose own job reached a header get a probe; it starts from the end state of the previous
    // header-bearing job and scans through any header-less segments in between.
    for (size_t i = 0; i < streams.size(); i++) {
        plan.first_probe[i] = probes.size();
        const size_t f = ctx.first_seg[i], e = ctx.first_seg[i + 1];
        if (e - f < 2) continue;
        const StreamDesc &sd = streams[i];
        bool chain = job_ok(f), pending = false;
        Cursor cur{R1.res[f].final_pos, R1.res[f].final_cr};
        size_t cur_job = f; // the job whose end state `cur` is
        auto add_probe = [&](size_t target, int64_t limit) {
            const bool tail = R1.res[cur_job].tail_valid && ctx.jobs[cur_job].probe_limit == limit; // that job has already run this probe
            probes.push_back(Probe{(uint32_t)i, target, cur, tail ? -1 : (int)plan.jobs.size(), tail ? (int)cur_job : -1, nullptr, 0});
            if (!tail) plan.jobs.push_back(walk_job(sd, cur, limit, true));
        };
        for (size_t k = f + 1; k < e && chain; k++) {
            if (cur.pos >= segs[k].b1) continue; // a packet ran across this whole segment
            if (!has_header(k)) { pending = true; continue; }
            add_probe(k, std::min<int64_t>((int64_t)sd.len, segs[k].b1 + 16ll * sps));
            chain = job_ok(k);
            cur = Cursor{R1.res[k].final_pos, R1.res[k].final_cr};
            cur_job = k;
            pending = false;
        }
        if (chain && pending) add_probe(e - 1, (int64_t)sd.len); // header-less tail still has to be walked
    }
    plan.first_probe[streams.size()] = probes.size();
    // Tail probes that stopped behind their first FIND_SFD step (Job.tail_stop_sfd) in a state NO header-bearing attempt of their successors
    // passed through - the successor triggered two or more chirps later, as happens when a cut falls inside a packet train: they are run to the
    // header after all, as explicit probe jobs in the one launch below (a mismatch must cost a probe, not a serial walk of the segment).
    // (tail_of is set only where the job's tail_valid holds: tail_probe_last finds the record.)
    bool through = false; // some explicit probe of this launch walks its whole target segment (it needs a segment job's record capacity)
    for (Probe &pb : probes) {
        if (pb.job >= 0) continue;
        const AttemptRec *L = tail_probe_last(R1, (size_t)pb.tail_of);
        if (!L) continue;
        if (tail_at_sync(R1, (size_t)pb.tail_of)) {
            // (likewise a probe that ended at SYNC on the position of a successor whose first attempt then lost sync: the true trajectory loses sync
            // there too, and the probe that would have walked on to the next header is run now)
            if (pb.target == (size_t)pb.tail_of + 1u && sync_stop_match(R1, pb.target, true) >= 0) continue;
        } else {
            if (L->status != kAttemptAtSfd || L->n_sfd == 0u) continue;
            const int64_t pos = L->sfd_pos[L->n_sfd - 1u];
            const uint32_t fails = L->sfd_fails[L->n_sfd - 1u];
            if (any_segment_record(R1, ctx.first_seg[pb.stream], pb.target, [&](const AttemptRec &r) { return passed_sfd_state(r, pos, fails); })) continue;
        }
        Job j = walk_job(streams[pb.stream], pb.start, ctx.jobs[(size_t)pb.tail_of].probe_limit, true);
        if (repair) {
            // (round 6) ... and past it: the job walks the whole target segment from the true state - the true trajectory itself, adopted by the stitch as a probe that
            // "ended without a header" at its limit; with noise over the stream such cuts are every second one, and a probe that stops at a header one sample beside the
            // speculative job's would send the segment down the serial path
            j.scan_limit = ctx.jobs[pb.target].scan_limit; j.stop_at_header = 0;
            through = true;
        }
        pb.job = (int)plan.jobs.size(); pb.tail_of = -1;
        plan.jobs.push_back(j);
    }
    // Tail probes that reached a header no successor job entered at the same sample: repaired in the same launch, all such cuts at once.
    plan.rpj = through ? std::max(ctx.rpj2, ctx.rpj1) : ctx.rpj2;
    if (!repair) return;
    for (Probe &pb : probes) {
        if (pb.job >= 0) continue; // (an explicit probe's result is not known yet: repair_explicit_probes, behind the launch)
        const AttemptRec *L = tail_probe_last(R1, (size_t)pb.tail_of);
        if (L && plan_repair(ctx, R1, streams[pb.stream], *L, pb, plan.jobs, R2)) plan.rpj = std::max(plan.rpj, ctx.rpj1);
    }
}

// ... and the same repair for EXPLICIT probes (a decoupled pass has no tail probes; the generic kernels none either): that a probe job reached a header no
// segment job entered is known only now, so these repairs take a launch of their own - one for all of them, into R4
template <class Env>
int repair_explicit_probes(Env &env, const std::vector<StreamDesc> &streams, const PassCtx &ctx, const RunOut &R1, const RunOut &R2, ProbePlan &plan,
                           RunOut &R4)
{
    std::vector<Job> rjobs;
    for (Probe &pb : plan.probes) {
        if (pb.job < 0) continue;
        const size_t pj = (size_t)pb.job;
        if (!plan.jobs[pj].stop_at_header) continue; // (a probe that walks its whole target segment: nothing to match)
        const JobResult &pr = R2.res[pj];
        if (!pr.pad || pr.n_attempts == 0u || pr.n_attempts > R2.cap) continue;
        plan_repair(ctx, R1, streams[pb.stream], R2.rec(pj, pr.n_attempts - 1u), pb, rjobs, R4);
    }
    if (rjobs.empty()) return 0;
    env.count_probes((uint32_t)rjobs.size());
    return env.run_jobs(rjobs, ctx.rpj1, 0, R4);
}

// One view per probe, whether it ran as its own job or as the tail of the preceding segment's job
struct ProbeView {
    JobResult res; const AttemptRec *recs; uint32_t cap; int64_t limit;
    uint32_t n_done() const // attempts that ran to completion (cf. RunOut::n_done)
    {
        const uint32_t n = res.pad ? res.n_attempts - 1u : res.n_attempts;
        return n < cap ? n : cap;
    }
};

inline std::vector<ProbeView> probe_views(const PassCtx &ctx, const RunOut &R1, const RunOut &R2, const ProbePlan &plan)
{
    std::vector<ProbeView> pv(plan.probes.size());
    for (size_t q = 0; q < plan.probes.size(); q++) {
        const Probe &pb = plan.probes[q];
        ProbeView &v = pv[q];
        if (pb.job >= 0) {
            const size_t pj = (size_t)pb.job;
            v.res = R2.res[pj]; v.recs = R2.recs.data() + pj * R2.rpj; v.cap = R2.cap; v.limit = plan.jobs[pj].scan_limit;
            continue;
        }
        const size_t tj = (size_t)pb.tail_of;
        const JobResult &jr = R1.res[tj];
        v.res = JobResult{};
        v.res.final_pos = jr.tail_final_pos; v.res.n_attempts = jr.tail_n_attempts; v.res.final_cr = jr.tail_final_cr;
        v.res.npush = jr.tail_npush;
        for (int t = 0; t < 4; t++) v.res.push_tail[t] = jr.tail_push_tail[t];
        v.res.stop_reason = jr.tail_stop_reason; v.res.pad = jr.tail_pad;
        const uint32_t first = std::min(jr.tail_first_rec, R1.cap);
        v.recs = R1.recs.data() + tj * R1.rpj + first; v.cap = R1.cap - first; v.limit = ctx.jobs[tj].probe_limit;
    }
    return pv;
}

// Adopts run `job` of R from its header record `a` on, where the probe's pending record L reached that header: the true DETECT scan is the probe's
// (its pushes, and the SNR at the trigger, :756), the header record and everything behind it the run's.  publish_any: publish the header record as
// it is (a merge with a segment job: the matched record is a frame); else only if it is a frame (a repair's first record).  False: the run ends with
// an attempt pending, the stream is incomplete.
template <class Env>
bool adopt_from_header(Env &env, StreamDesc &sd, Cursor &cur, const AttemptRec &L, const RunOut &R, size_t job, uint32_t a, bool publish_any)
{
    sd.pwr.apply(L.npush, L.push_tail);
    sd.pwr.determine_snr();
    if (publish_any || R.rec(job, a).status == kAttemptFrame) env.publish(R.rec(job, a), sd);
    sd.scan_pos = R.rec(job, a).end_pos; sd.scan_pwr = sd.pwr;
    for (uint32_t b = a + 1u; b < R.n_done(job); b++) adopt(env, R.rec(job, b), sd);
    const JobResult &jr = R.res[job];
    cur = end_cursor(R, job);
    if (jr.pad) { sd.incomplete = true; return false; }
    sd.pwr.apply(jr.npush, jr.push_tail);
    return true;
}

// ---- the stitch of stream i, probe by probe: merge with the segment job that entered the probe's header, adopt a repair, or walk serially
template <class Env>
int stitch_stream(Env &env, StreamDesc &sd, size_t i, const PassCtx &ctx, const RunOut &R1, const ProbePlan &plan, const std::vector<ProbeView> &pv)
{
    const uint32_t sps = env.sps();
    const std::vector<Seg> &segs = ctx.segs;
    const size_t f = ctx.first_seg[i];
    sd.scan_pos = segs[f].b0; sd.scan_pwr = sd.pwr;
    // the first segment starts from the true state: adopt it wholesale
    const bool first_known = end_known(R1, f);
    for (uint32_t a = 0; first_known && a < R1.n_done(f); a++) adopt(env, R1.rec(f, a), sd);
    if (ctx.tracing) env.append_trace(R1, (uint32_t)f, ctx.trace_cap, sd.abs_base);
    Cursor cur = first_known ? end_cursor(R1, f) : Cursor{segs[f].b0, sd.cr_in};
    int64_t covered = first_known ? segs[f].b1 : segs[f].b0; // the true trajectory is known up to here
    if (first_known && R1.res[f].pad) sd.incomplete = true;
    else if (first_known) sd.pwr.apply(R1.res[f].npush, R1.res[f].push_tail);
    auto serial_to = [&](int64_t limit, const char *why) -> int {
        if (debug_on()) fprintf(stderr, "[lora_hip] serial fallback stream %u pos %lld -> %lld: %s\n", sd.id, (long long)cur.pos, (long long)limit, why);
        env.count_slow_path();
        int r = run_serial(env, sd, cur, limit, false);
        covered = std::max(covered, limit);
        return r;
    };
    if (!first_known) {
        if (const int r = serial_to(segs[f].b1, "first segment's pending record did not fit")) return r;
    } else if (!sd.incomplete && R1.res[f].stop_reason == 2u)
        if (const int r = serial_to(segs[f].b1, "first segment out of records")) return r;
    for (size_t q = plan.first_probe[i]; q < plan.first_probe[i + 1] && !sd.incomplete; q++) {
        const Probe &pb = plan.probes[q];
        const int64_t b1 = segs[pb.target].b1;
        if (cur.pos >= b1) continue;
        if (pb.start.pos != cur.pos || pb.start.cr != cur.cr) { // speculation chain broken: redo serially
            if (const int r = serial_to(b1, "probe start differs from the true state")) return r;
            continue;
        }
        const ProbeView &view = pv[q];
        const JobResult &pr = view.res;
        if (pr.pad && pr.n_attempts > view.cap) { // the pending attempt's record did not fit: nothing of the probe is adopted, the cursor stands
            if (const int r = serial_to(b1, "probe out of records")) return r;
            continue;
        }
        // the attempts the true trajectory completed before the header: lost-sync ones, and a whole-segment probe's frames
        for (uint32_t a = 0; a < view.n_done(); a++) adopt(env, view.recs[a], sd);
        if (!pr.pad) { // no header before the probe's limit
            cur = Cursor{pr.final_pos, pr.final_cr};
            sd.pwr.apply(pr.npush, pr.push_tail);
            covered = std::max(covered, std::min<int64_t>(view.limit, b1));
            if (pr.stop_reason == 2u || (cur.pos < b1 && cur.pos + 2 * (int64_t)sps <= (int64_t)sd.len))
                if (const int r = serial_to(b1, "probe ended without a header")) return r;
            continue;
        }
        const AttemptRec &L = view.recs[pr.n_attempts - 1u];
        // a tail probe that ended at its first SYNC exit, on the position the next segment's job published there (tail_at_sync); its record is an out-of-data one
        const bool at_sync = pb.tail_of >= 0 && pr.stop_reason == kStopAtSync;
        if (!at_sync && L.status != kAttemptAtHeader && L.status != kAttemptAtSfd) { // ran out of data before reaching a header (a whole-segment probe: or inside a packet)
            cur = Cursor{L.start_pos, L.cr_prev};
            sd.incomplete = true;
            break;
        }
        // which segment job entered a header at the same sample?  (A probe that stopped behind its first FIND_SFD step, Job.tail_stop_sfd:
        // which job's header-bearing attempt STARTED a FIND_SFD step in the state the probe stopped in - passed_sfd_state.)
        const bool at_sfd = L.status == kAttemptAtSfd;
        const int64_t probe_sfd_pos = (at_sfd && L.n_sfd) ? L.sfd_pos[L.n_sfd - 1u] : -1;
        const uint32_t probe_sfd_fails = (at_sfd && L.n_sfd) ? L.sfd_fails[L.n_sfd - 1u] : 0u;
        int match = -1;
        size_t mk = 0;
        if (at_sync) { // the same FIND_SFD entry state as the successor's first attempt: that record and all behind it, if its header stands under the true d_phdr.cr
            mk = pb.target;
            if (pb.target == (size_t)pb.tail_of + 1u && segs[mk].b1 > cur.pos) match = sync_stop_match(R1, mk, false);
            if (match >= 0 && (wrong_fec_branch(R1.rec(mk, (uint32_t)match), L.cr_prev) || !end_known(R1, mk))) match = -1;
        }
        for (size_t k = f + 1; !at_sync && k <= pb.target && match < 0; k++) {
            if (segs[k].b1 <= cur.pos) continue;
            mk = k;
            match = find_record(R1, k, [&](const AttemptRec &r) { // (not a header-only record: a merge publishes the matched record's frame)
                return header_bearing(r, false) && (at_sfd ? passed_sfd_state(r, probe_sfd_pos, probe_sfd_fails) : r.hdr_pos == L.hdr_pos) &&
                       !wrong_fec_branch(r, L.cr_prev);
            });
            if (match >= 0 && !end_known(R1, k)) match = -1;
        }
        if (match < 0 && pb.rep_out && !at_sfd && !at_sync) { // the rest of the target segment, run again from the true header
            const RunOut &RR = *pb.rep_out;
            const size_t rj = pb.rep_job;
            if (RR.n_done(rj) >= 1u && RR.rec(rj, 0).hdr_pos == L.hdr_pos && RR.res[rj].stop_reason != 2u && end_known(RR, rj)) {
                if (!adopt_from_header(env, sd, cur, L, RR, rj, 0, false)) break;
                covered = std::max(covered, b1);
                env.count_repair();
                continue;
            }
        }
        if (match < 0) {
            if (debug_on()) {
                fprintf(stderr, "[lora_hip] probe for segment %zu [%lld, %lld): start %lld cr %u -> trig %lld hdr %lld (stopped %s, FIND_SFD state %lld / %u)\n", pb.target, (long long)segs[pb.target].b0, (long long)b1,
                        (long long)pb.start.pos, pb.start.cr, (long long)L.trig_pos, (long long)L.hdr_pos, at_sync ? "at SYNC" : at_sfd ? "behind its first FIND_SFD step" : "at the header", (long long)(at_sync ? L.end_pos : probe_sfd_pos), probe_sfd_fails);
                for (size_t k = pb.target ? pb.target - 1 : 0; k <= pb.target; k++)
                    for (uint32_t a = 0; a < std::min(R1.res[k].n_attempts, R1.cap); a++) {
                        const AttemptRec &r = R1.rec(k, a);
                        fprintf(stderr, "[lora_hip]    job %zu [%lld, %lld) rec %u status %u start %lld trig %lld hdr %lld end %lld\n", k, (long long)segs[k].b0, (long long)segs[k].b1, a, r.status,
                                (long long)r.start_pos, (long long)r.trig_pos, (long long)r.hdr_pos, (long long)r.end_pos);
                    }
            }
            cur = Cursor{L.start_pos, L.cr_prev};
            if (const int r = serial_to(b1, at_sync ? "the successor's first attempt, which left SYNC where the probe did, is not one to merge with"
                                                     : at_sfd ? "no segment job passed through the probe's FIND_SFD state" : "no segment job entered the same header")) return r;
            continue;
        }
        if (R1.rec(mk, (uint32_t)match).status == kAttemptOutOfData) {
            cur = Cursor{L.start_pos, L.cr_prev};
            sd.incomplete = true;
            break;
        }
        // merged: the true DETECT scan is the probe's, everything after the header is the job's
        if (!adopt_from_header(env, sd, cur, L, R1, mk, (uint32_t)match, true)) break;
        covered = std::max(covered, segs[mk].b1);
        if (R1.res[mk].stop_reason == 2u)
            if (const int r = serial_to(segs[mk].b1, "segment job out of records")) return r;
    }
    // whatever the probes did not cover is walked serially (exactness before speed)
    if (!sd.incomplete && cur.pos < (int64_t)sd.len && covered < (int64_t)sd.len && cur.pos + 2 * (int64_t)sps <= (int64_t)sd.len)
        if (const int r = serial_to((int64_t)sd.len, "uncovered tail")) return r;
    if (sd.incomplete) { // the attempt is run again from the start of its scan, wherever a job or probe of this pass took the scan up
        cur.pos = sd.scan_pos;
        sd.pwr = sd.scan_pwr;
    }
    sd.final_pos = cur.pos;
    sd.cr_out = cur.cr;
    return 0;
}

template <class Env>
int decode_end(Env &env, std::vector<StreamDesc> &streams, PassCtx &ctx)
{
    if (!ctx.launched) return 0; // nothing to decode
    ctx.launched = false;
    RunOut &R1 = env.run_out(0), &R2 = env.run_out(1);
    int s = env.run_jobs_end(R1);
    if (s != 0) return s;
    const auto tp1 = std::chrono::steady_clock::now();
    if (debug_jobs_on()) // diagnostics: every segment job's result
        for (size_t k = 0; k < ctx.jobs.size(); k++) dump_job("job", k, ctx.jobs[k], R1);
    if (ctx.segmenting) {
        s = rerun_wrong_branch(env, streams, ctx, R1);
        if (s != 0) return s;
    }
    // the payloads of the header-only jobs: the payload pass starts here and is collected behind the launch of the explicit probes below - which are
    // planned on the records as they stand (a header-only record says where its packet ends if nothing moves the symbol clock) and planned again in the
    // rare pass whose payloads change that (payload_end: jobs split, cut short or run again)
    PayloadRound pround;
    // whatever goes wrong between payload_begin and payload_end (a failed probe launch, a failed round of the payload pass itself), the pass's kernels may
    // still be reading and writing the handle's page-locked staging buffers on their own stream: every early return drains it first
    struct PayloadGuard { Env &env; bool armed; ~PayloadGuard() { if (armed) env.abort_payload(); } } pguard{env, false};
    if (ctx.decoupled) {
        pguard.armed = true;
        s = payload_begin(env, streams, ctx, R1, pround);
        if (s != 0) return s;
        pguard.armed = pround.open; // (a pass without a header-only record launched nothing: no stream to drain, and the staging vectors keep their capacity)
    }
    env.set_skip_payload(false);
    static const bool no_repair = getenv("LORA_HIP_NO_REPAIR") != nullptr; // (A/B: every mismatching cut takes the serial path, as until round 6)
    const bool repair = !ctx.tracing && !no_repair;
    ProbePlan plan;
    while (true) {
        plan_probes(env.sps(), streams, ctx, R1, R2, repair, plan);
        R2.res.clear(); R2.recs.clear();
        if (!plan.jobs.empty()) {
            env.count_probes((uint32_t)plan.jobs.size());
            s = env.run_jobs(plan.jobs, plan.rpj, 0, R2);
            if (s != 0) return s;
        }
        if (!pround.open) break;
        s = payload_end(env, streams, ctx, R1, pround); // from here on the records are ordinary ones
        if (s < 0) return s;
        pguard.armed = false;
        if (s == 0) break; // (1: the pass was re-laid - its probes are planned again)
    }
    RunOut R4;
    if (repair) {
        s = repair_explicit_probes(env, streams, ctx, R1, R2, plan, R4);
        if (s != 0) return s;
    }
    if (debug_jobs_on())
        for (size_t k = 0; k < plan.jobs.size(); k++) dump_job("probe", k, plan.jobs[k], R2);
    const std::vector<ProbeView> pv = probe_views(ctx, R1, R2, plan);
    const auto tp2 = std::chrono::steady_clock::now();
    for (size_t i = 0; i < streams.size(); i++) { // stream by stream, in stream order
        s = stitch_stream(env, streams[i], i, ctx, R1, plan, pv);
        if (s != 0) return s;
    }
    if (debug_on()) {
        const auto tp3 = std::chrono::steady_clock::now();
        auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "[lora_hip] plan %.3f ms, round1 %.3f ms (%zu jobs, rpj %u), round2 %.3f ms (%zu probe jobs, %zu tail probes), stitch %.3f ms, walker %.3f ms\n",
                ms(ctx.tp_in, ctx.tp0), ms(ctx.tp0, tp1), ctx.jobs.size(), ctx.rpj1, ms(tp1, tp2), plan.jobs.size(), plan.probes.size() - plan.jobs.size(), ms(tp2, tp3),
                env.walker_ms());
    }
    return 0;
}

// One pass, start to finish (the synchronous entry points and the CPU simulation).
template <class Env>
int decode_streams(Env &env, std::vector<StreamDesc> &streams)
{
    PassCtx ctx;
    const int s = decode_begin(env, streams, ctx);
    if (s != 0) return s;
    return decode_end(env, streams, ctx);
}


} // namespace lora_hip
