"""CPU tests of the product's speculation scheduler (gr_lora_amd/csrc/lora_stitch.hpp): the same
decode_streams<> template the device runtime uses, instantiated over an environment whose jobs are run by the
oracle's state machine (tests/host_sim/stitch_sim.cpp).  Segmenting + probing + stitching must reproduce the
serial decoder exactly: frames, order, header positions."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gr_lora_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "host_sim")
SIM_LIB = os.path.join(SIM_DIR, "libstitch_sim.so")


def load_sim():
    """Builds tests/host_sim/libstitch_sim.so when stale (the oracle library must exist) and returns its runner."""
    src = os.path.join(SIM_DIR, "stitch_sim.cpp")
    deps = [src, os.path.join(ROOT, "gr_lora_amd", "csrc", "lora_stitch.hpp"), os.path.join(ROOT, "gr_lora_amd", "csrc", "lora_device.h"),
            os.path.join(ROOT, "oracle", "liblora_oracle.so")]
    if not os.path.exists(SIM_LIB) or any(os.path.getmtime(d) > os.path.getmtime(SIM_LIB) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-o", SIM_LIB, src, "-L", os.path.join(ROOT, "oracle"),
                               "-llora_oracle", "-Wl,-rpath," + os.path.join(ROOT, "oracle")])
    L = C.CDLL(SIM_LIB)
    L.stitch_sim_decode_streams.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                            C.c_void_p]

    def run(iq, sf, ctor_cr=4, demod=2, reduced=False, seg=0, slots=512, tails=True, plan=False, early=False, decoupled=False, force_rerun=0, auto=False,
            two_per_cu=False, streams=None):
        """streams: [(offset, length), ...] of several streams laid back to back in iq (default: one stream, all of it); the frames' streams are
        returned in stats["stream"], their header positions are relative to their stream"""
        a = np.ascontiguousarray(iq, dtype=np.complex64)
        sd = np.asarray(streams if streams is not None else [(0, a.size)], dtype=np.uint64).reshape(-1, 2)
        offs, lns = np.ascontiguousarray(sd[:, 0]), np.ascontiguousarray(sd[:, 1])
        out = np.zeros(1 << 20, dtype=np.uint8)
        lens = np.zeros(4096, dtype=np.int32)
        hp = np.zeros(4096, dtype=np.int64)
        so = np.zeros(4096, dtype=np.int32)
        st = np.zeros(16, dtype=np.uint32)
        mode = int(tails) | (2 if plan else 0) | (4 if early else 0) | (8 if decoupled else 0) | (16 if auto else 0) | (32 if two_per_cu else 0) | ((force_rerun & 0xff) << 8)
        n = L.stitch_sim_decode_streams(a.ctypes.data, a.size, offs.ctypes.data, lns.ctypes.data, len(offs), sf, ctor_cr, 1, int(reduced), demod, seg,
                                        slots, mode, out.ctypes.data, out.size, lens.ctypes.data, hp.ctypes.data, so.ctypes.data, 4096, st.ctypes.data)
        assert n >= 0, n
        frames, off = [], 0
        for i in range(n):
            frames.append(bytes(out[off:off + lens[i]]))
            off += int(lens[i])
        return frames, hp[:n].tolist(), dict(jobs=int(st[0]), probes=int(st[1]), slow=int(st[2]), incomplete=int(st[3]), tails=int(st[4]), planned=int(st[5]), early=int(st[6]),
                                           payload=int(st[7]), rerun=int(st[8]), moved=int(st[9]), pending=int(st[10]), repairs=int(st[11]),
                                           hash="%016x" % (int(st[12]) | int(st[13]) << 32), stream=so[:n].tolist())
    return run


@pytest.fixture(scope="module")
def sim(oracle_mod):
    return load_sim()


def _serial(O, iq, sf, ctor_cr=4, demod=2, reduced=False):
    o = O.Oracle(sf=sf, cr=ctor_cr, demod=demod, reduced_rate=reduced)
    o.run(iq)
    return o.frames(), o.frame_positions()


@pytest.mark.parametrize("tails", [True, False])
@pytest.mark.parametrize("seg", [16, 23, 40, 64, 150, 0])
def test_segmented_equals_serial(sim, oracle_mod, seg, tails):
    cfg = synth.TxConfig(sf=7, cr=4)
    rng = np.random.default_rng(900 + seg)
    payloads = [bytes(rng.integers(0, 256, int(rng.integers(1, 48)), dtype=np.uint8)) for _ in range(30)]
    gaps = [int(g) for g in rng.integers(0, 7 * cfg.sps, len(payloads))]
    gaps[5] = 0; gaps[6] = 1; gaps[7] = cfg.sps // 2; gaps[8] = 2 * cfg.sps + 3
    st = synth.build_stream(payloads, cfg, gaps=gaps)
    want, wpos = _serial(oracle_mod, st.iq, 7)
    got, gpos, stats = sim(st.iq, 7, seg=seg, slots=40, tails=tails)
    assert got == want and gpos == wpos
    assert stats["jobs"] >= (st.iq.size // (seg * cfg.sps) if seg else 2)
    if tails: # the probes ride on the segment jobs; explicit probe jobs only across header-less segments
        assert stats["tails"] > 0 and stats["probes"] <= stats["tails"]
    else:
        assert stats["probes"] > 0 and stats["tails"] == 0


@pytest.mark.parametrize("slots,snr_db", [(8, None), (16, None), (30, None), (100, None), (16, 10.0), (16, -8.0)])
def test_burst_aware_plan_equals_serial(sim, oracle_mod, slots, snr_db):
    """Auto mode with the envelope pre-pass: cuts fall in the gaps between bursts (plan_burst_segments).  Same frames
    as the serial decoder; on clean dense traffic every job starts at a gap, so nothing falls back and the job count
    is the slot count or less.  Below the noise (wideband) the envelope shows no gaps and the fixed grid is used."""
    cfg = synth.TxConfig(sf=7, cr=4)
    rng = np.random.default_rng(4100 + slots)
    payloads = [bytes(rng.integers(0, 256, int(rng.integers(4, 40)), dtype=np.uint8)) for _ in range(64)]
    st = synth.build_stream(payloads, cfg, rng=rng, gap_symbols=(2.0, 6.0))
    iq = st.iq
    if snr_db is not None:
        sigma = synth.awgn_sigma_for_snr(snr_db, cfg)
        iq = (iq + sigma / np.sqrt(2.0) * (rng.standard_normal(iq.size) + 1j * rng.standard_normal(iq.size))).astype(np.complex64)
    want, wpos = _serial(oracle_mod, iq, 7)
    got, gpos, stats = sim(iq, 7, seg=0, slots=slots, plan=True)
    assert got == want and gpos == wpos
    if snr_db is None:
        assert len(want) == len(payloads)
        assert stats["planned"] == (1 if slots <= 30 else 0)  # fewer bursts than slots: fixed grid
        print(slots, stats)
        if stats["planned"]:
            assert stats["jobs"] <= slots and stats["slow"] == 0 and stats["probes"] == 0


@pytest.mark.parametrize("slots,auto", [(100, False), (100, True), (200, True), (60, True)])
def test_fewer_bursts_than_slots_is_planned_for_one_workgroup_per_cu(sim, oracle_mod, slots, auto):
    """A kernel that fits a CU twice reports twice the CUs as slots; a pass with fewer bursts than that, but at least one per CU, is planned for
    one workgroup per CU (resident_slots_alt = walker_resident_slots_full on the device: whole packets per job, no fixed grid, no probes) and is
    decoupled only with no more jobs than CUs (round 5: config 3's 256 packets per cell at SF7 / SF8).  Same frames as the serial decoder."""
    cfg = synth.TxConfig(sf=7, cr=4)
    rng = np.random.default_rng(5100 + slots)
    payloads = [bytes(rng.integers(0, 256, int(rng.integers(4, 40)), dtype=np.uint8)) for _ in range(64)]
    st = synth.build_stream(payloads, cfg, rng=rng, gap_symbols=(2.0, 6.0))
    want, wpos = _serial(oracle_mod, st.iq, 7)
    assert len(want) == len(payloads)
    got, gpos, stats = sim(st.iq, 7, seg=0, slots=slots, plan=True, auto=auto, two_per_cu=True)
    assert got == want and gpos == wpos
    cap = slots if len(payloads) >= slots else slots // 2   # bursts for every slot: the ordinary plan; at least one per CU: the plan for slots / 2 jobs
    if len(payloads) >= slots // 2 and stats["payload"] == 0:
        assert stats["planned"] == 1 and stats["jobs"] <= cap + 1 and stats["slow"] == 0 and stats["probes"] == 0, stats
    if auto and len(payloads) + 1 <= slots // 2:
        assert stats["payload"] > 0, stats    # no more jobs than CUs: a decoupled pass
    base, _, bstats = sim(st.iq, 7, seg=0, slots=slots, plan=True, auto=auto)
    assert base == want
    print(slots, auto, stats, bstats)


def test_fast_path_dominates_on_regular_traffic(sim, oracle_mod):
    """On ordinary traffic nearly every segment merges through its probe; serial fall-backs stay rare."""
    cfg = synth.TxConfig(sf=7, cr=4)
    rng = np.random.default_rng(4)
    payloads = [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(60)]
    st = synth.build_stream(payloads, cfg, rng=rng)
    want, wpos = _serial(oracle_mod, st.iq, 7)
    got, gpos, stats = sim(st.iq, 7, seg=64)
    assert got == want and gpos == wpos
    assert stats["slow"] <= 2 and stats["jobs"] > 60
    got, gpos, stats = sim(st.iq, 7, seg=0, slots=30, plan=True, early=True)      # burst-aware cuts + early-stopping tail probes (walker3's mode)
    assert got == want and gpos == wpos
    assert stats["slow"] == 0 and stats["early"] > 0 and stats["probes"] == 0, stats


@pytest.mark.parametrize("sf,cr,noise_db", [(8, 1, -32), (7, 2, -30), (9, 3, None)])
def test_noise_and_stale_cr_carry(sim, oracle_mod, sf, cr, noise_db):
    cfg = synth.TxConfig(sf=sf, cr=cr)
    rng = np.random.default_rng(77 + sf)
    payloads = [bytes(rng.integers(0, 256, int(rng.integers(4, 30)), dtype=np.uint8)) for _ in range(12)]
    st = synth.build_stream(payloads, cfg, rng=rng, noise_sigma=(10 ** (noise_db / 20.0) if noise_db else 0.0))
    want, wpos = _serial(oracle_mod, st.iq, sf)
    for seg in (20, 57):
        for tails in (True, False):
            got, gpos, _ = sim(st.iq, sf, seg=seg, tails=tails)
            assert got == want and gpos == wpos


def test_gradient_mode_and_truncated_stream(sim, oracle_mod):
    """demod = GRAD through the scheduler, and a stream that ends in the middle of a packet."""
    cfg = synth.TxConfig(sf=7, cr=4)
    rng = np.random.default_rng(12)
    payloads = [bytes(rng.integers(0, 256, 20, dtype=np.uint8)) for _ in range(10)]
    st = synth.build_stream(payloads, cfg, rng=rng)
    cut = st.iq[: st.header_starts[-1] + 30 * cfg.sps]
    for demod in (0, 2):
        want, wpos = _serial(oracle_mod, cut, 7, demod=demod)
        got, gpos, stats = sim(cut, 7, demod=demod, seg=33)
        assert got == want and gpos == wpos and len(got) == 9
        assert stats["incomplete"] == 1


def _plan(sim_lib, lens, edges, sps, slots, nominal):
    import ctypes as C
    L = C.CDLL(SIM_LIB)
    ne = np.asarray([len(e) for e in edges], dtype=np.int32)
    flat = np.asarray([x for e in edges for x in e], dtype=np.int64)
    ln = np.asarray(lens, dtype=np.int64)
    out = np.zeros(1 << 16, dtype=np.int64)
    nc = np.zeros(len(lens), dtype=np.int32)
    L.stitch_sim_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_ulonglong, C.c_void_p, C.c_int, C.c_void_p]
    rc = L.stitch_sim_plan(ln.ctypes.data, ne.ctypes.data, flat.ctypes.data, len(lens), sps, slots, nominal, out.ctypes.data, out.size, nc.ctypes.data)
    cuts, k = [], 0
    for n in nc:
        cuts.append(out[k:k + int(n)].tolist()); k += int(n)
    return rc, cuts


def test_burst_plan_properties(sim):
    """plan_burst_segments by its contract: cuts ascending, strictly inside the stream, at gap starts (or on the grid inside
    gap-less stretches), at most `slots` segments in all; equal bursts -> equal packets per job; too few bursts -> fixed grid."""
    sps = 1024
    rng = np.random.default_rng(3)
    # 1. equal bursts, the bench shape: 8 streams x 128 bursts, 512 slots -> 2 bursts per job
    period = 108 * sps
    lens = [128 * period + 5 * sps] * 8
    edges = [[(k + 1) * period - 4 * sps for k in range(128)] for _ in range(8)]
    rc, cuts = _plan(sim, lens, edges, sps, 512, 225 * sps)
    assert rc == 1 and sum(len(c) + 1 for c in cuts) <= 512
    for c, e in zip(cuts, edges):
        assert c == sorted(set(c)) and set(c) <= set(e) and 0 < c[0] and c[-1] < lens[0]
        assert all((e.index(b) - e.index(a)) == 2 for a, b in zip(c, c[1:]))     # two bursts between consecutive cuts
    # 2. ragged bursts and stream lengths: invariants only
    lens, edges = [], []
    for s in range(5):
        n = int(rng.integers(40, 400))
        gaps = rng.integers(30, 400, n) * sps
        e = np.cumsum(gaps).tolist()
        edges.append([int(x) for x in e]); lens.append(int(e[-1] + int(rng.integers(9, 50)) * sps))
    total = sum(lens)
    for slots in (64, 200, 512):
        nominal = max(64 * sps, total // slots)
        rc, cuts = _plan(sim, lens, edges, sps, slots, nominal)
        if sum(len(e) for e in edges) < slots:
            assert rc == 0
            continue
        assert rc == 1 and sum(len(c) + 1 for c in cuts) <= slots
        for c, e, ln in zip(cuts, edges, lens):
            assert c == sorted(set(c)) and all(0 < x < ln for x in c)
            prev = 0
            for x in c + [ln]:
                assert x in e or x == ln or (x - prev) <= 3 * nominal   # a cut off the gap list only subdivides an over-long stretch
                prev = x
    # 3. a stretch without gaps is subdivided on the grid
    lens = [4000 * sps]
    edges = [[50 * sps * k for k in range(1, 21)] + [3990 * sps]]
    rc, cuts = _plan(sim, lens, edges, sps, 16, 200 * sps)
    assert rc == 1 and max(b - a for a, b in zip([0] + cuts[0], cuts[0] + lens)) <= 3 * 200 * sps


@pytest.mark.parametrize("seg", [20, 33, 57])
def test_header_with_cr_zero_ahead_of_a_cut(sim, oracle_mod, seg):
    """A header whose CR field is 0 leaves d_phdr.cr = 0 behind: the NEXT header then decodes through neither Hamming
    branch (no switch case, lib/decoder_impl.cc:655-675) and reads as zeros.  A segment job that speculated the
    constructor's CR on that next header must not be merged, wherever the cut falls: segmented == serial."""
    rng = np.random.default_rng(77 + seg)
    pieces = []
    for cr in (4, 0, 4, 2, 0, 0, 3, 4):
        cfg = synth.TxConfig(sf=7, cr=cr)
        p = bytes(rng.integers(0, 256, int(rng.integers(4, 20)), dtype=np.uint8))
        pieces.append(synth.build_stream([p], cfg, rng=rng, tail_symbols=0.0).iq)
    iq = np.concatenate(pieces + [np.zeros(4096, np.complex64)])
    for ctor_cr in (4, 1):
        want, wpos = _serial(oracle_mod, iq, 7, ctor_cr=ctor_cr)
        for tails in (True, False):
            got, gpos, stats = sim(iq, 7, ctor_cr=ctor_cr, seg=seg, slots=64, tails=tails)
            assert got == want and gpos == wpos, (seg, ctor_cr, tails)


@pytest.mark.parametrize("seg", [16, 23, 40, 64, 150, 0])
def test_early_stopping_tail_probes_equal_serial(sim, oracle_mod, seg):
    """Job.tail_stop_sfd (walker3): tail probes stop behind their first FIND_SFD step and are matched against the FIND_SFD entry
    states their successor recorded - the same ragged traffic as test_segmented_equals_serial (back-to-back packets, gaps of 0, 1,
    half a symbol), noisy and clean: segmented == serial, and the probes really do stop early."""
    cfg = synth.TxConfig(sf=7, cr=4)
    rng = np.random.default_rng(900 + seg)
    payloads = [bytes(rng.integers(0, 256, int(rng.integers(1, 48)), dtype=np.uint8)) for _ in range(30)]
    gaps = [int(g) for g in rng.integers(0, 7 * cfg.sps, len(payloads))]
    gaps[5] = 0; gaps[6] = 1; gaps[7] = cfg.sps // 2; gaps[8] = 2 * cfg.sps + 3
    for sigma in (0.0, 10 ** (-30 / 20.0)):
        st = synth.build_stream(payloads, cfg, gaps=gaps, rng=np.random.default_rng(seg), noise_sigma=sigma)
        want, wpos = _serial(oracle_mod, st.iq, 7)
        got, gpos, stats = sim(st.iq, 7, seg=seg, slots=40, early=True)
        assert got == want and gpos == wpos, (seg, sigma)
        assert stats["early"] > 0 and stats["early"] <= stats["tails"], stats
        ref_stats = sim(st.iq, 7, seg=seg, slots=40)[2]
        # (a probe that stopped early finds no partner when its successor triggered more than a symbol later - cuts in mid-preamble, which
        # this adversarial grid produces and burst-aware cuts do not; the price is a serial fall-back, never a wrong frame)
        # (round 6: the reference run's mismatching cuts - its tail probes ran to their headers - are repaired in the probe launch, lora_stitch.hpp; a
        # probe that stopped early knows no header to repair from)
        assert stats["slow"] <= ref_stats["slow"] + 6, (stats, ref_stats)


@pytest.mark.parametrize("sf,cr,noise_db", [(8, 1, -32), (7, 2, -30), (9, 3, None)])
def test_early_stopping_probes_with_noise_and_stale_cr(sim, oracle_mod, sf, cr, noise_db):
    cfg = synth.TxConfig(sf=sf, cr=cr)
    rng = np.random.default_rng(77 + sf)
    payloads = [bytes(rng.integers(0, 256, int(rng.integers(4, 30)), dtype=np.uint8)) for _ in range(12)]
    st = synth.build_stream(payloads, cfg, rng=rng, noise_sigma=(10 ** (noise_db / 20.0) if noise_db else 0.0))
    want, wpos = _serial(oracle_mod, st.iq, sf)
    for seg in (20, 57):
        got, gpos, stats = sim(st.iq, sf, seg=seg, early=True)
        assert got == want and gpos == wpos
    got, gpos, stats = sim(st.iq, sf, seg=0, slots=8, plan=True, early=True)
    assert got == want and gpos == wpos


def test_wrong_header_branch_jobs_are_rerun_in_one_batch(sim, oracle_mod):
    """CR 4/5 traffic under noise into a decoder constructed with CR 4: every later segment's job guesses Hamming class 2 for its first header
    where the true d_phdr.cr (the predecessor's header's) is of class 1, and with bit errors in the header the two decodes disagree.  Those jobs
    are run again TOGETHER with the value their predecessor's tail probe reported (decode_end, round 1b) instead of one serial launch each:
    segmented == serial, and the serial fall-backs stay a handful."""
    cfg = synth.TxConfig(sf=8, cr=1)
    rng = np.random.default_rng(321)
    payloads = [bytes(rng.integers(0, 256, int(rng.integers(6, 24)), dtype=np.uint8)) for _ in range(40)]
    st = synth.build_stream(payloads, cfg, rng=rng, noise_sigma=10 ** (-27 / 20.0))
    want, wpos = _serial(oracle_mod, st.iq, 8, ctor_cr=4, demod=0)
    for early in (False, True):
        got, gpos, stats = sim(st.iq, 8, ctor_cr=4, demod=0, seg=0, slots=20, plan=True, early=early)
        assert got == want and gpos == wpos, early
        assert stats["planned"] == 1 and stats["slow"] <= 6, stats
    assert len(want) >= 30


@pytest.mark.parametrize("early", [False, True])
@pytest.mark.parametrize("seg", [16, 40, 150, 0])
def test_decoupled_pass_equals_serial(sim, oracle_mod, seg, early):
    """The decoupled pass (header-only segment jobs, LaunchCfg.skip_payload + the payload pass, lora_stitch.hpp payload_round) against the serial
    decoder: clean traffic (no packet is run again), noisy traffic with a drifting symbol clock (packets that move the clock ARE run again, and the
    rest of their job with them), and every third / every packet forced through the re-run path."""
    cfg = synth.TxConfig(sf=7, cr=4)
    rng = np.random.default_rng(4100 + seg)
    payloads = [bytes(rng.integers(0, 256, int(rng.integers(1, 48)), dtype=np.uint8)) for _ in range(24)]
    gaps = [int(g) for g in rng.integers(0, 9 * cfg.sps, len(payloads))]
    gaps[3] = 0; gaps[4] = 1; gaps[9] = cfg.sps // 2
    st = synth.build_stream(payloads, cfg, gaps=gaps)
    want, wpos = _serial(oracle_mod, st.iq, 7)
    assert len(want) >= 20
    for force in (0, 3, 1):
        got, gpos, stats = sim(st.iq, 7, seg=seg, slots=40, early=early, decoupled=True, force_rerun=force)
        assert got == want and gpos == wpos, (seg, force, stats)
        assert stats["payload"] >= len(want) - 2, stats
        if force == 0:
            assert stats["rerun"] == 0, stats
        else:
            assert stats["rerun"] > 0, stats
    # noise + a transmitter clock 40 ppm off (linear resampling): fine_sync moves the symbol clock inside payloads
    stn = synth.build_stream(payloads, cfg, gaps=gaps, rng=np.random.default_rng(5), noise_sigma=synth.awgn_sigma_for_snr(40.0, cfg))
    t = np.arange(int(stn.iq.size / (1 + 40e-6)) - 2, dtype=np.float64) * (1 + 40e-6)
    i0 = t.astype(np.int64)
    fr = (t - i0).astype(np.float32)
    noisy = (stn.iq[i0] * (1 - fr) + stn.iq[i0 + 1] * fr).astype(np.complex64)
    want, wpos = _serial(oracle_mod, noisy, 7)
    assert len(want) >= 15
    got, gpos, stats = sim(noisy, 7, seg=seg, slots=40, early=early, decoupled=True)
    assert got == want and gpos == wpos, (seg, stats)
    assert stats["moved"] > 0 and stats["rerun"] == 0, stats     # jobs split behind the packets that moved the clock, a probe from each true end
    got, gpos, stats2 = sim(noisy, 7, seg=seg, slots=40, early=early, decoupled=True, force_rerun=2)
    assert got == want and gpos == wpos, (seg, stats2)
    print(seg, early, stats, stats2)


def test_decoupled_pass_cut_mid_packet_and_other_coding_rates(sim, oracle_mod):
    """Header-only jobs where the data ends inside a payload (the packet is pending, the stream resumes at its scan's start) and with the header FEC
    branch carried across segments (CR 4/5 traffic, constructor CR 4/8: round 1b runs header-only jobs again)."""
    for cr, ctor in ((1, 4), (2, 1), (3, 4)):
        cfg = synth.TxConfig(sf=7, cr=cr)
        rng = np.random.default_rng(77 + cr)
        payloads = [bytes(rng.integers(0, 256, int(rng.integers(4, 40)), dtype=np.uint8)) for _ in range(12)]
        st = synth.build_stream(payloads, cfg, gaps=[int(g) for g in rng.integers(0, 6 * cfg.sps, len(payloads))])
        iq = st.iq[: st.iq.size - 30 * cfg.sps]  # the last packet loses its tail
        want, wpos = _serial(oracle_mod, iq, 7, ctor_cr=ctor)
        for seg in (24, 0):
            got, gpos, stats = sim(iq, 7, ctor_cr=ctor, seg=seg, slots=24, decoupled=True)
            ref = sim(iq, 7, ctor_cr=ctor, seg=seg, slots=24)
            assert got == want and gpos == wpos, (cr, seg, stats)
            assert stats["incomplete"] == ref[2]["incomplete"] == 1 and stats["pending"] >= 1, (stats, ref[2])


def test_decoupled_pass_one_job_per_burst(sim, oracle_mod):
    """the device's per-pass rule (the jobs fit the device at once): with the gaps between bursts known, a decoupled pass gets one job per burst - cuts in
    the gaps, plus a 24-symbol grid inside longer bursts - and a pass with more bursts than workgroup slots stays an ordinary one"""
    cfg = synth.TxConfig(sf=7, cr=4)
    rng = np.random.default_rng(11)
    payloads = [bytes(rng.integers(0, 256, int(rng.integers(8, 48)), dtype=np.uint8)) for _ in range(20)]
    st = synth.build_stream(payloads, cfg, rng=rng, gap_symbols=(3.0, 9.0))
    want, wpos = _serial(oracle_mod, st.iq, 7)
    got, gpos, stats = sim(st.iq, 7, slots=128, plan=True, early=True, auto=True)
    assert got == want and gpos == wpos, stats
    # (the grid cuts fall inside packets and may cost an explicit probe each)
    assert stats["payload"] >= 20 and 19 <= stats["jobs"] <= 128 and stats["slow"] == 0 and stats["planned"] == 1, stats
    got, gpos, stats = sim(st.iq, 7, slots=16, plan=True, early=True, auto=True)     # 20 bursts for 16 slots: not a decoupled pass
    assert got == want and gpos == wpos and stats["payload"] == 0, stats


# ---- scheduling fingerprints: which path produced the frames, pinned against tests/golden/stitch_fingerprints.json
# (tests/golden/make_stitch_fingerprints.py writes it).  Each workload is one an existing test above runs, with its parameters; the
# fingerprint is the sim's FNV-1a hash over every scheduler call (jobs, payload requests, counters, publishes) plus frames, positions
# and counters.  A refactor of the scheduler must leave all of it unchanged.
FINGERPRINTS = os.path.join(ROOT, "tests", "golden", "stitch_fingerprints.json")


def _ragged_sf7(seg, sigma):
    """test_early_stopping_tail_probes_equal_serial's traffic"""
    cfg = synth.TxConfig(sf=7, cr=4)
    rng = np.random.default_rng(900 + seg)
    payloads = [bytes(rng.integers(0, 256, int(rng.integers(1, 48)), dtype=np.uint8)) for _ in range(30)]
    gaps = [int(g) for g in rng.integers(0, 7 * cfg.sps, len(payloads))]
    gaps[5] = 0; gaps[6] = 1; gaps[7] = cfg.sps // 2; gaps[8] = 2 * cfg.sps + 3
    return synth.build_stream(payloads, cfg, gaps=gaps, rng=np.random.default_rng(seg), noise_sigma=sigma).iq


def _noise_stale_cr(sf, cr, noise_db):
    """test_noise_and_stale_cr_carry's traffic"""
    cfg = synth.TxConfig(sf=sf, cr=cr)
    rng = np.random.default_rng(77 + sf)
    payloads = [bytes(rng.integers(0, 256, int(rng.integers(4, 30)), dtype=np.uint8)) for _ in range(12)]
    return synth.build_stream(payloads, cfg, rng=rng, noise_sigma=(10 ** (noise_db / 20.0) if noise_db else 0.0)).iq


def _decoupled_traffic(seg, drift):
    """test_decoupled_pass_equals_serial's traffic: clean, or noisy with a transmitter clock 40 ppm off"""
    cfg = synth.TxConfig(sf=7, cr=4)
    rng = np.random.default_rng(4100 + seg)
    payloads = [bytes(rng.integers(0, 256, int(rng.integers(1, 48)), dtype=np.uint8)) for _ in range(24)]
    gaps = [int(g) for g in rng.integers(0, 9 * cfg.sps, len(payloads))]
    gaps[3] = 0; gaps[4] = 1; gaps[9] = cfg.sps // 2
    if not drift:
        return synth.build_stream(payloads, cfg, gaps=gaps).iq
    stn = synth.build_stream(payloads, cfg, gaps=gaps, rng=np.random.default_rng(5), noise_sigma=synth.awgn_sigma_for_snr(40.0, cfg))
    t = np.arange(int(stn.iq.size / (1 + 40e-6)) - 2, dtype=np.float64) * (1 + 40e-6)
    i0 = t.astype(np.int64)
    fr = (t - i0).astype(np.float32)
    return (stn.iq[i0] * (1 - fr) + stn.iq[i0 + 1] * fr).astype(np.complex64)


def _wrong_header_branch():
    """test_wrong_header_branch_jobs_are_rerun_in_one_batch's traffic"""
    cfg = synth.TxConfig(sf=8, cr=1)
    rng = np.random.default_rng(321)
    payloads = [bytes(rng.integers(0, 256, int(rng.integers(6, 24)), dtype=np.uint8)) for _ in range(40)]
    return synth.build_stream(payloads, cfg, rng=rng, noise_sigma=10 ** (-27 / 20.0)).iq


def _header_cr_zero(seg):
    """test_header_with_cr_zero_ahead_of_a_cut's traffic"""
    rng = np.random.default_rng(77 + seg)
    pieces = []
    for cr in (4, 0, 4, 2, 0, 0, 3, 4):
        cfg = synth.TxConfig(sf=7, cr=cr)
        p = bytes(rng.integers(0, 256, int(rng.integers(4, 20)), dtype=np.uint8))
        pieces.append(synth.build_stream([p], cfg, rng=rng, tail_symbols=0.0).iq)
    return np.concatenate(pieces + [np.zeros(4096, np.complex64)])


def _bursts(seed):
    """test_burst_aware_plan_equals_serial's (clean) / test_fewer_bursts_than_slots_...'s traffic"""
    cfg = synth.TxConfig(sf=7, cr=4)
    rng = np.random.default_rng(seed)
    payloads = [bytes(rng.integers(0, 256, int(rng.integers(4, 40)), dtype=np.uint8)) for _ in range(64)]
    return synth.build_stream(payloads, cfg, rng=rng, gap_symbols=(2.0, 6.0)).iq


def _truncated(before_header_symbols=-30):
    """test_gradient_mode_and_truncated_stream's traffic, cut 30 symbols into the last packet - or, negative, this many symbols before its header
    (inside the preamble: a probe runs out of data before it reaches a header)"""
    cfg = synth.TxConfig(sf=7, cr=4)
    rng = np.random.default_rng(12)
    payloads = [bytes(rng.integers(0, 256, 20, dtype=np.uint8)) for _ in range(10)]
    st = synth.build_stream(payloads, cfg, rng=rng)
    return st.iq[: st.header_starts[-1] - before_header_symbols * cfg.sps]


def _decoupled_cut_mid_packet():
    """test_decoupled_pass_cut_mid_packet_and_other_coding_rates's first case (CR 4/5 traffic, constructor CR 4/8)"""
    cfg = synth.TxConfig(sf=7, cr=1)
    rng = np.random.default_rng(78)
    payloads = [bytes(rng.integers(0, 256, int(rng.integers(4, 40)), dtype=np.uint8)) for _ in range(12)]
    st = synth.build_stream(payloads, cfg, gaps=[int(g) for g in rng.integers(0, 6 * cfg.sps, len(payloads))])
    return st.iq[: st.iq.size - 30 * cfg.sps]


def fingerprint_workloads():
    """name -> (iq, sim keyword arguments)"""
    w = {
        "noise_stale_cr_sf8_seg20": (_noise_stale_cr(8, 1, -32), dict(sf=8, seg=20)),
        "noise_stale_cr_sf7_seg57_explicit_probes": (_noise_stale_cr(7, 2, -30), dict(sf=7, seg=57, tails=False)),
        "noise_stale_cr_sf9_plan_early": (_noise_stale_cr(9, 3, None), dict(sf=9, seg=0, slots=8, plan=True, early=True)),
        "early_probes_seg40_noisy": (_ragged_sf7(40, 10 ** (-30 / 20.0)), dict(sf=7, seg=40, slots=40, early=True)),
        "ragged_seg16_tails": (_ragged_sf7(16, 0.0), dict(sf=7, seg=16, slots=40)),
        "decoupled_seg40_force_rerun3": (_decoupled_traffic(40, False), dict(sf=7, seg=40, slots=40, decoupled=True, force_rerun=3)),
        "decoupled_seg16_drift_early_force_rerun2": (_decoupled_traffic(16, True), dict(sf=7, seg=16, slots=40, early=True, decoupled=True, force_rerun=2)),
        "wrong_header_branch": (_wrong_header_branch(), dict(sf=8, ctor_cr=4, demod=0, seg=0, slots=20, plan=True)),
        "wrong_header_branch_early": (_wrong_header_branch(), dict(sf=8, ctor_cr=4, demod=0, seg=0, slots=20, plan=True, early=True)),
        "burst_plan_slots16": (_bursts(4116), dict(sf=7, seg=0, slots=16, plan=True)),
        "header_cr_zero_seg33": (_header_cr_zero(33), dict(sf=7, ctor_cr=4, seg=33, slots=64)),
        "two_per_cu_auto_slots100": (_bursts(5200), dict(sf=7, seg=0, slots=100, plan=True, auto=True, two_per_cu=True)),
        "cut_mid_packet_grad_seg33": (_truncated(), dict(sf=7, demod=0, seg=33)),
        "cut_mid_packet_decoupled_seg24": (_decoupled_cut_mid_packet(), dict(sf=7, ctor_cr=4, seg=24, slots=24, decoupled=True)),
        "cut_mid_preamble_seg20": (_truncated(4), dict(sf=7, seg=20)),
    }
    parts = [_ragged_sf7(23, 10 ** (-30 / 20.0)), _noise_stale_cr(7, 2, -30), _truncated(), _decoupled_traffic(40, False)]
    offs = np.cumsum([0] + [p.size for p in parts[:-1]]).tolist()
    w["multi_stream_4_seg20"] = (np.concatenate(parts), dict(sf=7, seg=20, slots=40, streams=[(o, p.size) for o, p in zip(offs, parts)]))
    return w


def fingerprints(sim):
    out = {}
    for name, (iq, kw) in fingerprint_workloads().items():
        kw = dict(kw)
        frames, pos, stats = sim(iq, kw.pop("sf"), **kw)
        out[name] = dict(frames=[f.hex() for f in frames], header_pos=pos, stats=stats)
    return out


def test_scheduling_fingerprints_match_golden(sim):
    """Frames, header positions, counters (repairs included) and the hash over every scheduler call, per workload, equal the golden's: a change
    of the scheduler that keeps the frames but takes other paths (a repair turned into a serial walk) shows here."""
    import json
    with open(FINGERPRINTS) as f:
        want = json.load(f)
    got = fingerprints(sim)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
