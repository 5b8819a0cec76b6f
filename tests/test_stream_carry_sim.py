"""What a stream carries from one pass to the next - the resume position, d_phdr.cr and the power state (StreamCarry, carry_collect / carry_launch in
gr_lora_amd/csrc/lora_stitch.hpp, called by pipe_collect / pipe_rotate of lora_runtime.cpp) - held to the serial decoder on the CPU: the host
simulation (tests/host_sim/stitch_sim.cpp, stitch_sim_decode_passes) decodes a stream in passes through the product's scheduler and the product's
carry rule, its jobs run by the oracle's state machine.

Two things are required of every run.  The frames - blobs with their SNR byte, absolute header positions, order, none twice, none missing - equal the
serial oracle's over the whole stream.  And every pass ends in the state the serial decoder is in at that point: final_pos, incomplete, d_phdr.cr and
the power state equal those of ONE oracle job (stitch_sim_serial_state: lora_oracle_run_job alone, no scheduler) over the same items from the same
start state; with an attempt pending that is the start of the attempt's scan, the CR the attempt started with (its cr_prev - not the CR of the header
it may have decoded since) and the power state behind the last completed attempt."""
import ctypes as C

import numpy as np
import pytest

import stream_carry_cases as cases
from test_stitch_sim import SIM_LIB, load_sim

MODES = {
    "one_job": dict(seg=100000),
    "grid16": dict(seg=16), "grid24": dict(seg=24), "grid33": dict(seg=33), "grid57": dict(seg=57),
    "grid16_no_tails": dict(seg=16, tails=False), "grid24_no_tails": dict(seg=24, tails=False), "grid33_no_tails": dict(seg=33, tails=False),
    "grid57_no_tails": dict(seg=57, tails=False),
    "early24": dict(seg=24, early=True), "early57": dict(seg=57, early=True),
    "plan": dict(seg=0, slots=6, plan=True), "plan_early": dict(seg=0, slots=6, plan=True, early=True),
    "decoupled24": dict(seg=24, decoupled=True), "decoupled_early33": dict(seg=33, decoupled=True, early=True),
    "auto": dict(seg=0, slots=64, plan=True, early=True, auto=True),
}


class Sim:
    def __init__(self):
        load_sim()  # (builds the library when stale)
        self.L = L = C.CDLL(SIM_LIB)
        vp = C.c_void_p
        L.stitch_sim_decode_passes.argtypes = [vp, C.c_size_t, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_int,
                                               C.c_uint32, vp, C.c_size_t, vp, vp, C.c_int, vp, C.c_int, vp]
        L.stitch_sim_serial_state.argtypes = [vp, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, vp, vp, vp, vp]

    def passes(self, w, chunks, seg=0, slots=64, tails=True, plan=False, early=False, decoupled=False, auto=False, rec_cap=0, tight_probes=False):
        """-> frames, header positions, per-pass states, counters"""
        a = np.ascontiguousarray(w.iq, dtype=np.complex64)
        ch = np.asarray(chunks, dtype=np.uint64)
        assert int(ch.sum()) == a.size
        out = np.zeros(1 << 18, dtype=np.uint8)
        lens = np.zeros(1024, dtype=np.int32)
        hp = np.zeros(1024, dtype=np.int64)
        ps = np.zeros((len(ch) + 1, 20), dtype=np.int64)
        st = np.zeros(16, dtype=np.uint32)
        mode = int(tails) | (2 if plan else 0) | (4 if early else 0) | (8 if decoupled else 0) | (16 if auto else 0)
        n = self.L.stitch_sim_decode_passes(a.ctypes.data, a.size, ch.ctypes.data, len(ch), w.sf, w.ctor_cr, 1, 0, w.demod, seg, slots, mode, rec_cap | (int(tight_probes) << 16),
                                            out.ctypes.data, out.size, lens.ctypes.data, hp.ctypes.data, 1024, ps.ctypes.data, ps.shape[0], st.ctypes.data)
        assert n >= 0, n
        frames, off = [], 0
        for i in range(n):
            frames.append(bytes(out[off:off + lens[i]]))
            off += int(lens[i])
        states = [dict(host_base=int(r[0]), len=int(r[1]), cr_in=int(r[2]), final_pos=int(r[3]), cr_out=int(r[4]), incomplete=int(r[5]), frames=int(r[6]),
                       pwr_in=tuple(int(x) for x in r[7:13]), pwr_out=tuple(int(x) for x in r[13:19]), keep_from=int(r[19])) for r in ps[:int(st[3])]]
        stats = dict(jobs=int(st[0]), probes=int(st[1]), slow=int(st[2]), passes=int(st[3]), tails=int(st[4]), planned=int(st[5]), early=int(st[6]),
                     payload=int(st[7]), repairs=int(st[11]), through=int(st[12]), through_pending=int(st[13]), dropped=int(st[14]), dropped_behind_frames=int(st[15]))
        return frames, hp[:n].tolist(), states, stats

    def serial_state(self, w, iq, cr_in, pwr_in):
        """the serial decoder behind iq, from DETECT at its first item with d_phdr.cr = cr_in and the power state pwr_in: one oracle job"""
        a = np.ascontiguousarray(iq, dtype=np.complex64)
        pin = np.asarray(pwr_in, dtype=np.uint32)
        state = np.zeros(4, dtype=np.int64)
        pout = np.zeros(6, dtype=np.uint32)
        crp = C.c_int(0)
        rc = self.L.stitch_sim_serial_state(a.ctypes.data, a.size, w.sf, w.ctor_cr, 1, 0, w.demod, cr_in, pin.ctypes.data, state.ctypes.data, pout.ctypes.data,
                                            C.byref(crp))
        assert rc == 0, rc
        return dict(final_pos=int(state[0]), incomplete=int(state[1]), cr_out=int(state[2]), pwr_out=tuple(int(x) for x in pout), cr_pending=crp.value)


@pytest.fixture(scope="module")
def sim(oracle_mod):
    return Sim()


_truth = {}


def truth(O, w):
    """the serial oracle over the whole stream, once per workload"""
    if w.name not in _truth:
        o = O.Oracle(sf=w.sf, cr=w.ctor_cr, demod=w.demod)
        o.run(w.iq)
        _truth[w.name] = (o.frames(), o.frame_positions())
    return _truth[w.name]


_workloads = {}


def workload(name):
    if name not in _workloads:
        _workloads[name] = getattr(cases, name)()
    return _workloads[name]


def check(sim, O, w, chunks, what, **mode):
    """one chunked decode: frames against the whole-stream oracle, every pass's end state against one oracle job"""
    want, wpos = truth(O, w)
    got, gpos, states, stats = sim.passes(w, chunks, **mode)
    assert len(set(gpos)) == len(gpos), (what, "a frame was published twice", gpos)
    assert gpos == wpos, (what, gpos, wpos)
    assert got == want, (what, [i for i, (g, t) in enumerate(zip(got, want)) if g != t])
    base = 0
    for k, s in enumerate(states):
        assert s["host_base"] == base, (what, k, s)
        one = sim.serial_state(w, w.iq[base:base + s["len"]], s["cr_in"], s["pwr_in"])
        for key in ("final_pos", "incomplete", "cr_out", "pwr_out"):
            assert s[key] == one[key], (what, "pass %d of %d" % (k, len(states)), key, s, one)
        assert s["keep_from"] == min(max(s["final_pos"], 0), s["len"])
        base += s["keep_from"]
        if k + 1 < len(states):
            assert (states[k + 1]["cr_in"], states[k + 1]["pwr_in"]) == (s["cr_out"], s["pwr_out"]), (what, k)
    return states, stats


def check_cut(sim, O, w, k, cut, what, **mode):
    """two passes, the first ending at `cut` inside packet k; the stream is taken up to the start of packet k + 3"""
    p = w.prefix(k + 3)
    return check(sim, O, p, [cut, p.iq.size - cut], what, **mode)


def _chunks_of(total, sizes):
    out, left, i = [], total, 0
    while left > 0:
        c = min(int(sizes[i % len(sizes)]), left)
        out.append(c); left -= c; i += 1
    return out


def test_workloads_have_the_frames_they_should(sim, oracle_mod):
    for name, n in (("header_cr_zero", 12), ("mixed_cr_noisy", 10), ("alternating_cr_idle_noise", 12)):
        w = workload(name)
        want, wpos = truth(oracle_mod, w)
        assert len(want) == n and 100000 < w.iq.size < 1100000, (name, len(want), w.iq.size)
        assert len(w.cuts()) == 5 * n and all(0 < c < w.iq.size for _, _, c in w.cuts())
        assert truth(oracle_mod, w.prefix(5)) == (want[:5], wpos[:5])


# ---- header CR 0: no noise needed

@pytest.mark.parametrize("kind", ["preamble", "sync", "header", "payload", "gap"])
def test_header_cr_zero_every_cut_one_job(sim, oracle_mod, kind):
    """the simplest path: two passes, each decoded as one job.  A pass that ends inside a packet behind its header must hand on the CR the packet was
    ENTERED with, not the packet's own: packets 1, 4, 5, 9 carry CR 0, and the packets behind them read as the all-zero header only on that branch."""
    w = workload("header_cr_zero")
    for k, _, cut in w.cuts(kinds=[kind]):
        check_cut(sim, oracle_mod, w, k, cut, (kind, k, cut), **MODES["one_job"])


@pytest.mark.parametrize("mode", [m for m in MODES if m != "one_job"])
def test_header_cr_zero_every_scheduler_mode(sim, oracle_mod, mode):
    w = workload("header_cr_zero")
    for k, kind, cut in w.cuts(packets=[1], kinds=["header", "payload"]) + w.cuts(packets=[2], kinds=["payload"]) + w.cuts(packets=[5], kinds=["preamble", "sync", "payload"]):
        check_cut(sim, oracle_mod, w, k, cut, (mode, kind, k, cut), **MODES[mode])


def test_constructor_cr_of_another_class_than_the_first_packet(sim, oracle_mod):
    import dataclasses
    for ctor in (1, 0):
        w = dataclasses.replace(workload("header_cr_zero"), name="header_cr_zero_ctor%d" % ctor, ctor_cr=ctor)
        for mode in ("one_job", "grid24", "decoupled_early33"):
            for k, kind, cut in w.cuts(packets=[0, 1], kinds=["preamble", "header", "payload"]):
                check_cut(sim, oracle_mod, w, k, cut, (ctor, mode, kind, k, cut), **MODES[mode])


# ---- chunk sizes

def test_chunk_sizes(sim, oracle_mod):
    """chunks from two symbols up, a random list, 4096-item calls, and chunks so short that a pending packet stays pending across three passes and more"""
    rng = np.random.default_rng(5)
    for name in ("header_cr_zero", "alternating_cr_idle_noise"):
        w = workload(name)
        sps, n = w.sps, w.iq.size
        for mode in ("one_job", "grid16"):
            check(sim, oracle_mod, w, _chunks_of(n, rng.integers(1, 90 * sps, 64)), (name, "random", mode), **MODES[mode])
        p = w.prefix(4)
        check(sim, oracle_mod, p, _chunks_of(p.iq.size, [13 * sps - 5]), (name, "13 symbols"), **MODES["one_job"])
        for pname, sizes in (("two_symbols", [2 * sps]), ("three_symbols_and_one", [3 * sps + 1]), ("items_4096", [4096]),
                             ("random_short", rng.integers(1, 9 * sps, 512))):
            states, _ = check(sim, oracle_mod, p, _chunks_of(p.iq.size, sizes), (name, pname), **MODES["one_job"])
            if pname == "two_symbols":
                run = best = 0
                for s in states:
                    run = run + 1 if s["incomplete"] else 0
                    best = max(best, run)
                assert best >= 3, best  # a packet pending across three passes (it spans 20 symbols and more)


# ---- mixed CR 1-4 under noise

def _teeth(sim, O, w):
    """by the oracle alone: the packets with a cut at which resuming with the pending packet's own CR (d_phdr.cr behind its header) instead of the CR
    the serial decoder holds at the resume point changes the frames"""
    want, wpos = truth(O, w)
    teeth = []
    for k, kind, cut in w.cuts(kinds=["payload"]):
        one = sim.serial_state(w, w.iq[:cut], w.ctor_cr, (0,) * 6)
        if not one["incomplete"] or one["cr_pending"] < 0 or one["cr_pending"] == one["cr_out"]:
            continue
        res = []
        for cr in (one["cr_out"], one["cr_pending"]):
            o = O.Oracle(sf=w.sf, cr=cr, demod=w.demod)
            o.run(w.iq[one["final_pos"]:])
            res.append(([f[15:] for f in o.frames()], [p + one["final_pos"] for p in o.frame_positions()]))
        n_before = sum(1 for p in wpos if p < one["final_pos"])
        assert res[0] == ([f[15:] for f in want[n_before:]], wpos[n_before:]), (k, cut)   # the true CR: the serial decoder's frames
        if res[1] != res[0]:
            teeth.append(k)
    return teeth


def test_mixed_cr_under_noise_has_teeth(sim, oracle_mod):
    """With CRs 1-4 a wrong carried CR shows only on a header with bit errors on which the two Hamming branches disagree: this workload has such a
    packet behind one of its cuts (stream_carry_cases.MIXED_CR_SIGMA says how the level was found)."""
    teeth = _teeth(sim, oracle_mod, workload("mixed_cr_noisy"))
    print("packets inside which a carry of the pending packet's own CR changes the output:", teeth)
    assert teeth == [3], teeth


@pytest.mark.parametrize("mode", list(MODES))
def test_mixed_cr_under_noise_every_scheduler_mode(sim, oracle_mod, mode):
    w = workload("mixed_cr_noisy")
    for k, kind, cut in w.cuts(packets=[3], kinds=["header", "payload"]):   # (packet 3: the one test_mixed_cr_under_noise_has_teeth finds)
        check_cut(sim, oracle_mod, w, k, cut, (mode, kind, k, cut), **MODES[mode])
    if mode in ("one_job", "grid33", "early24", "decoupled24"):
        p = w.prefix(6)
        check(sim, oracle_mod, p, _chunks_of(p.iq.size, [61 * w.sps + 17]), (mode, "61 symbols"), **MODES[mode])


# ---- the whole-segment probes (first finding)

@pytest.mark.parametrize("mode", list(MODES))
def test_alternating_cr_idle_noise_every_scheduler_mode(sim, oracle_mod, mode):
    w = workload("alternating_cr_idle_noise")
    for k, kind, cut in w.cuts(packets=[3], kinds=["payload"]) + w.cuts(packets=[7], kinds=["header"]):
        check_cut(sim, oracle_mod, w, k, cut, (mode, kind, k, cut), **MODES[mode])
    if mode in ("grid24", "grid57", "plan", "plan_early", "decoupled_early33", "auto"):   # (the modes the tests below do not run this workload in)
        p = w.prefix(7)
        check(sim, oracle_mod, p, _chunks_of(p.iq.size, [61 * w.sps + 17]), (mode, "61 symbols"), **MODES[mode])


def test_whole_segment_probe_that_runs_out_of_data_behind_adopted_frames(sim, oracle_mod):
    """Noise over the idle gaps and early-stopping tail probes: cuts whose probe found no partner are walked by whole-segment probes
    (stop_at_header = 0), which adopt real frames - those move d_phdr.cr - and, in a pass that ends inside a packet, run out of data behind them.  The
    counters show that this happened; the carry must be the serial decoder's all the same."""
    w = workload("alternating_cr_idle_noise")
    through = pending = 0
    for mode in ("plan_early", "early57"):
        for k, kind, cut in w.cuts(packets=[7, 8, 9], kinds=["header", "payload"]):
            _, stats = check_cut(sim, oracle_mod, w, k, cut, (mode, kind, k, cut), **MODES[mode])
            through += stats["through"]; pending += stats["through_pending"]
    print("whole-segment probes:", through, "of which ran out of data behind a frame:", pending)
    assert through > 0 and pending > 0, (through, pending)


@pytest.mark.parametrize("rec_cap", [1, 2, 3])
def test_probes_and_walks_short_of_records_publish_nothing_twice(sim, oracle_mod, rec_cap):
    """Every launch behind a pass's main one (probes, whole-segment probes, repairs, serial walks) held to one, two or three attempt records per job: they
    stop 'out of records' behind frames they have already handed over, and whatever goes on from there must start behind those frames."""
    w = workload("alternating_cr_idle_noise")
    for mode in ("early24", "grid16_no_tails", "decoupled24"):
        for k, kind, cut in w.cuts(packets=[4], kinds=["payload"]) + w.cuts(packets=[7], kinds=["gap"]):
            check_cut(sim, oracle_mod, w, k, cut, (rec_cap, mode, kind, k, cut), rec_cap=rec_cap, **MODES[mode])


def test_probe_whose_pending_record_did_not_fit_publishes_nothing_twice(sim, oracle_mod):
    """The kernels, like the oracle, begin no attempt without room for its record, so a pending attempt's record always fits.  The stitch has a branch
    for a probe whose pending record did NOT fit all the same.  The simulation reaches it (SimEnv::tight_probes) by giving a probe launch exactly the
    record capacity that the completed attempts of one of its jobs with an attempt pending fill: by preference a job that completed a frame first
    (a whole-segment probe), else the pending job with the fewest completed attempts.  Nothing of such a probe is adopted, the segment is walked from
    the cursor, and no frame comes out twice.  The sim counts the records it dropped, and those of them whose job had completed a frame."""
    w = workload("alternating_cr_idle_noise")
    dropped = behind_frames = 0
    for mode in ("plan_early", "early57", "grid24_no_tails"):
        for k, kind, cut in w.cuts(packets=[7, 8], kinds=["header", "payload"]):
            _, stats = check_cut(sim, oracle_mod, w, k, cut, (mode, kind, k, cut), tight_probes=True, **MODES[mode])
            dropped += stats["dropped"]
            behind_frames += stats["dropped_behind_frames"]
    assert dropped > behind_frames > 0, (dropped, behind_frames)  # probes that stopped ahead of a header, and whole-segment ones behind frames
