// sync_stop_sim.cpp -- TEST-ONLY: stitch_sim.cpp's environment plus what the SF7 / SF8 walker does with LaunchCfg.sync_pos in the main launch of a
// pass (gr_lora_amd/csrc/lora_walker2.inc.hip): every job publishes the sample at which its first attempt leaves SYNC, and a tail probe whose own
// first attempt leaves SYNC at the sample its successor (Job.sync_succ) published ends there with tail_stop_reason = kStopAtSync and the pending
// record the out-of-data path writes.  Built by tests/test_sync_stop_sim.py with g++.
#include "stitch_sim.cpp"

namespace {
struct SyncEnv : SimEnv {
    uint32_t hide_mask = 0;  // bit (job & 31): that job's word reads zero - on the device, a successor that has not reached SYNC when the probe looks
    uint32_t n_published = 0, n_sync_stop = 0, n_differ = 0, n_failed_first = 0;

    // the sample at which the first attempt of a job started like this leaves SYNC for FIND_SFD, or -1: no trigger before the limit, or no FIND_SFD step
    int64_t first_sync_exit(const Job &jb, int64_t start, int64_t limit, uint32_t cr)
    {
        oracle_attempt_t rec{};
        oracle_job_result_t r{};
        lora_oracle_run_job(o, iq + 2 * jb.stream_off, (size_t)jb.stream_len, start, limit, cr, 1, 3, 1, &rec, &r);
        return (r.n_attempts >= 1u && rec.n_sfd >= 1u) ? rec.sfd_pos[0] : -1;
    }

    int run_jobs_begin(const std::vector<Job> &jobs, uint32_t rpj, uint32_t tc, RunOut &out) // (the main launch: the only one with sync words)
    {
        const int s = SimEnv::run(jobs, rpj, tc, out);
        if (s != 0 || !tail_probes) return s;
        std::vector<uint64_t> word(jobs.size(), 0);
        for (size_t j = 0; j < jobs.size(); j++) {
            if (jobs[j].start_at_header) continue;
            const int64_t p = first_sync_exit(jobs[j], jobs[j].start, jobs[j].scan_limit, jobs[j].cr_prev);
            if (p >= 0) { word[j] = (uint64_t)(p + 1); n_published++; }
        }
        for (size_t j = 0; j < jobs.size(); j++) {
            JobResult &jr = out.res[j];
            const uint32_t succ = jobs[j].sync_succ;
            if (!jr.tail_valid || succ == 0u || succ - 1u >= jobs.size() || jr.tail_n_attempts == 0u || jr.tail_first_rec >= rpj) continue;
            const int64_t p = first_sync_exit(jobs[j], jr.final_pos, jobs[j].probe_limit, jr.final_cr);
            if (p < 0) continue;
            // (a probe whose first attempt lost sync and that went on to a second: the device compares at the first SYNC exit only - as here)
            n_failed_first += (jr.tail_n_attempts >= 2u && out.rec(j, jr.tail_first_rec).status == kAttemptLostSync && word[succ - 1u] != (uint64_t)(p + 1)) ? 1u : 0u;
            const uint64_t w = ((hide_mask >> ((succ - 1u) & 31u)) & 1u) ? 0ull : word[succ - 1u];
            if (w != (uint64_t)(p + 1)) { n_differ += w ? 1u : 0u; continue; }
            AttemptRec &t = out.recs[j * (size_t)rpj + jr.tail_first_rec]; // the probe's first attempt: its scan and its pushes stand, the rest never ran
            t.status = kAttemptOutOfData; t.hdr_pos = -1; t.end_pos = p; t.frame_len = 0; t.n_symbols = 0; t.hdr_ambig = 0; t.n_sfd = 0;
            jr.tail_n_attempts = 1; jr.tail_pad = 1; jr.tail_stop_reason = kStopAtSync; jr.tail_final_pos = t.start_pos; jr.tail_final_cr = jr.final_cr;
            jr.tail_npush = 0;
            n_sync_stop++;
        }
        return s;
    }
};
} // namespace

// stitch_sim_decode_streams with the early stop at SYNC.  stats[0..13] as there; [14] tail probes that stopped at SYNC, [15] jobs that published a
// position, [16] probes that read a position other than their own, [17] probes whose first attempt lost sync elsewhere than their successor's.
extern "C" int sync_stop_sim_decode_streams(const float *iq, size_t n_items, const unsigned long long *offs, const unsigned long long *lens, int n_streams,
                                            int sf, int ctor_cr, int demod, uint32_t segment_symbols, uint32_t resident_slots, int burst_plan,
                                            uint32_t hide_mask, uint8_t *out, size_t cap, int *frame_lens, long long *hdr_pos, int *stream_of,
                                            int max_frames, uint32_t *stats)
{
    if (n_streams < 1 || n_streams > 32) return -4;
    for (int i = 0; i < n_streams; i++) if (offs[i] + lens[i] > n_items) return -4;
    lora_oracle_t *o = lora_oracle_create(1e6f, 125000, (uint8_t)sf, 0, (uint8_t)ctor_cr, 1, 0, 0, demod);
    if (!o) return -1;
    SyncEnv env{{o, iq, n_items, lora_oracle_sps(o), (uint32_t)ctor_cr, segment_symbols, resident_slots}};
    env.tail_probes = true;
    env.burst_plan = burst_plan != 0;
    env.hide_mask = hide_mask;
    std::vector<StreamDesc> sds(n_streams);
    for (int i = 0; i < n_streams; i++) {
        sds[i].off = offs[i]; sds[i].len = lens[i]; sds[i].id = (uint32_t)i; sds[i].cr_in = (uint32_t)ctor_cr; sds[i].abs_base = 0;
    }
    const int rc = decode_streams(env, sds);
    lora_oracle_destroy(o);
    if (rc != 0) return -2;
    size_t used = 0;
    int n = 0;
    for (const SimFrame &f : env.frames) {
        if (n >= max_frames || used + f.blob.size() > cap) return -3;
        std::memcpy(out + used, f.blob.data(), f.blob.size());
        frame_lens[n] = (int)f.blob.size(); hdr_pos[n] = f.hdr_pos; used += f.blob.size();
        if (stream_of) stream_of[n] = (int)f.stream;
        n++;
    }
    uint32_t incomplete = 0;
    for (int i = 0; i < n_streams; i++) incomplete |= sds[i].incomplete ? 1u << i : 0u;
    stats[0] = env.n_jobs; stats[1] = env.n_probes; stats[2] = env.n_slow; stats[3] = incomplete; stats[4] = env.n_tails; stats[5] = env.planned;
    stats[11] = env.n_repairs; stats[14] = env.n_sync_stop; stats[15] = env.n_published; stats[16] = env.n_differ; stats[17] = env.n_failed_first;
    return n;
}
