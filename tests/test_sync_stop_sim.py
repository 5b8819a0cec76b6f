"""CPU tests of the stitch's rule for tail probes that end at SYNC (kStopAtSync, gr_lora_amd/csrc/lora_stitch.hpp): decode_streams<> over the oracle's
state machine as in test_stitch_sim.py, with the SF7 / SF8 walker's part emulated by tests/host_sim/sync_stop_sim.cpp - every job of a pass's main
launch publishes where its first attempt leaves SYNC, and a tail probe whose own first attempt leaves SYNC at the sample its successor published ends
there.  Whatever the probes do, the adopted sequence must be the serial walk: frames, order, header positions, SNR bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gr_lora_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "host_sim")
SIM_LIB = os.path.join(SIM_DIR, "libsync_stop_sim.so")
ALL = 0xFFFFFFFF


def load_sim():
    src = os.path.join(SIM_DIR, "sync_stop_sim.cpp")
    deps = [src, os.path.join(SIM_DIR, "stitch_sim.cpp"), os.path.join(ROOT, "gr_lora_amd", "csrc", "lora_stitch.hpp"),
            os.path.join(ROOT, "gr_lora_amd", "csrc", "lora_device.h"), os.path.join(ROOT, "oracle", "liblora_oracle.so")]
    if not os.path.exists(SIM_LIB) or any(os.path.getmtime(d) > os.path.getmtime(SIM_LIB) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-o", SIM_LIB, src, "-L", os.path.join(ROOT, "oracle"),
                               "-llora_oracle", "-Wl,-rpath," + os.path.join(ROOT, "oracle")])
    L = C.CDLL(SIM_LIB)
    L.sync_stop_sim_decode_streams.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32,
                                               C.c_int, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]

    def run(iq, sf, ctor_cr=4, demod=2, seg=0, slots=512, plan=False, hide=0, streams=None):
        """hide: bit (job & 31) set - that job's published position reads as zero (a successor that has not reached SYNC when the probe looks)"""
        a = np.ascontiguousarray(iq, dtype=np.complex64)
        sd = np.asarray(streams if streams is not None else [(0, a.size)], dtype=np.uint64).reshape(-1, 2)
        offs, lns = np.ascontiguousarray(sd[:, 0]), np.ascontiguousarray(sd[:, 1])
        out = np.zeros(1 << 18, dtype=np.uint8)
        lens = np.zeros(1024, dtype=np.int32)
        hp = np.zeros(1024, dtype=np.int64)
        so = np.zeros(1024, dtype=np.int32)
        st = np.zeros(20, dtype=np.uint32)
        n = L.sync_stop_sim_decode_streams(a.ctypes.data, a.size, offs.ctypes.data, lns.ctypes.data, len(offs), sf, ctor_cr, demod, seg, slots, int(plan),
                                           hide, out.ctypes.data, out.size, lens.ctypes.data, hp.ctypes.data, so.ctypes.data, 1024, st.ctypes.data)
        assert n >= 0, n
        frames, off = [], 0
        for i in range(n):
            frames.append(bytes(out[off:off + lens[i]]))
            off += int(lens[i])
        return frames, hp[:n].tolist(), dict(jobs=int(st[0]), probes=int(st[1]), slow=int(st[2]), incomplete=int(st[3]), tails=int(st[4]), repairs=int(st[11]),
                                           stops=int(st[14]), published=int(st[15]), differ=int(st[16]), failed_first=int(st[17]), stream=so[:n].tolist())
    return run


@pytest.fixture(scope="module")
def sim(oracle_mod):
    return load_sim()


def _serial(O, iq, sf, ctor_cr=4, demod=2):
    o = O.Oracle(sf=sf, cr=ctor_cr, demod=demod)
    o.run(iq)
    return o.frames(), o.frame_positions()


def _packets(n, cfg, seed, length=8, **kw):
    rng = np.random.default_rng(seed)
    payloads = [bytes(rng.integers(0, 256, length, dtype=np.uint8)) for _ in range(n)]
    return synth.build_stream(payloads, cfg, rng=rng, **kw)


def _one(cfg, seed, length=8):
    return _packets(1, cfg, seed, length, gaps=[0], tail_symbols=0.0).iq


def _silence(symbols, cfg):
    return np.zeros(int(symbols * cfg.sps), np.complex64)


@pytest.mark.parametrize("sf,demod,seg", [(7, 2, 40), (7, 0, 56), (8, 2, 47), (8, 0, 64)])
def test_matching_tails_stop_at_sync_and_unpublished_ones_run_on(sim, oracle_mod, sf, demod, seg):
    """Clean traffic: every cut's probe leaves SYNC where its successor did, stops there, and the successor's records are adopted from its first attempt
    on.  A successor that has not published (all of them; every other one) leaves the probe to run to its header as before: the same frames."""
    cfg = synth.TxConfig(sf=sf, cr=4)
    st = _packets(7, cfg, 100 + sf + demod, gap_symbols=(2.0, 6.0))
    want, wpos = _serial(oracle_mod, st.iq, sf, demod=demod)
    assert len(want) == 7
    got, gpos, stats = sim(st.iq, sf, demod=demod, seg=seg)
    assert got == want and gpos == wpos
    assert stats["jobs"] >= 3 and stats["stops"] >= 2 and stats["slow"] == 0, stats
    for hide in (ALL, 0x55555555, 0xAAAAAAAA):
        g2, p2, s2 = sim(st.iq, sf, demod=demod, seg=seg, hide=hide)
        assert g2 == want and p2 == wpos, hide
        assert s2["stops"] < stats["stops"] and (hide != ALL or s2["stops"] == 0), (hide, s2)


@pytest.mark.parametrize("sf,seed", [(7, 5), (8, 6)])
def test_position_one_sample_off_does_not_stop(sim, oracle_mod, sf, seed):
    """40 dB of SNR: detect_upchirp's tie between adjacent shifts falls differently for the two DETECT alignments at about every second cut.  There
    the probe reads a position that is not its own and runs on; the cuts that do match stop.  Serial either way."""
    cfg = synth.TxConfig(sf=sf, cr=4)
    st = _packets(14, cfg, seed, gap_symbols=(2.0, 6.0), noise_sigma=synth.awgn_sigma_for_snr(40.0, cfg))
    want, wpos = _serial(oracle_mod, st.iq, sf)
    assert len(want) == 14
    got, gpos, stats = sim(st.iq, sf, seg=50)
    assert got == want and gpos == wpos
    assert stats["differ"] >= 1 and stats["stops"] >= 1, stats


def test_probe_with_a_failed_first_attempt_runs_to_its_header(sim, oracle_mod):
    """Two upchirps on their own trigger DETECT only for a scan that steps onto them within a few samples.  Moved through one symbol in steps, they are
    met by the probe's scan and not by the successor's at some offsets: the probe's first attempt loses sync, it reaches the next preamble in its
    SECOND attempt, and although it leaves SYNC there exactly where the successor's first attempt did, it does not stop.  At other offsets both scans
    meet them, or neither.  Serial at every offset."""
    cfg = synth.TxConfig(sf=7, cr=4)
    sps, seg = cfg.sps, 50
    a, b, c, d = (_one(cfg, s) for s in (1, 2, 3, 4))
    blip = a[:2 * sps]
    seen = dict(failed_first=0, stops=0)
    for off in range(0, sps, 48):
        lead = _silence(2, cfg)
        gap1 = np.zeros(seg * sps + sps // 2 + off - (lead.size + a.size), np.complex64)       # the two upchirps begin half a symbol and `off` samples behind the cut
        iq = np.concatenate([lead, a, gap1, blip, _silence(14, cfg), b, _silence(3, cfg), c, _silence(4, cfg), d, _silence(4, cfg)])
        want, wpos = _serial(oracle_mod, iq, 7)
        assert len(want) == 4
        got, gpos, stats = sim(iq, 7, seg=seg)
        assert got == want and gpos == wpos, off
        seen["failed_first"] += stats["failed_first"]
        seen["stops"] += stats["stops"]
    assert seen["failed_first"] >= 1 and seen["stops"] >= 1, seen


def test_successor_whose_first_acquisition_fails(sim, oracle_mod):
    """Six upchirps and nothing behind them, right after a cut: the probe and the successor both acquire them, leave SYNC at the same sample - the
    probe stops - and both lose sync in FIND_SFD.  The successor's first record is no header to merge with: the cut is probed again, explicitly,
    and the packet behind is the one the successor acquired on its second trigger."""
    cfg = synth.TxConfig(sf=7, cr=4)
    sps, seg = cfg.sps, 70
    a, b, c, d = (_one(cfg, s) for s in (11, 12, 13, 14))           # (44.25 symbols each)
    lead = _silence(2, cfg)
    gap1 = np.zeros(seg * sps + int(2.6 * sps) - (lead.size + a.size), np.complex64)
    # cuts at 70 (ahead of the six upchirps at 72.6; the packet behind them at 90.6 lies in the same segment) and 140 (ahead of the third packet at 142.6).
    # (Off the symbol grid on purpose: a successor whose scan steps exactly onto a preamble's first sample leaves SYNC one symbol ahead of any other scan.)
    iq = np.concatenate([lead, a, gap1, a[:6 * sps], _silence(12, cfg), b, _silence(7.75, cfg), c, _silence(4, cfg), d, _silence(4, cfg)])
    want, wpos = _serial(oracle_mod, iq, 7)
    assert len(want) == 4
    got, gpos, stats = sim(iq, 7, seg=seg)
    assert got == want and gpos == wpos
    assert stats["stops"] >= 2 and stats["probes"] >= 1, stats          # (the cut behind the six upchirps, and at least one ordinary one)
    ref = sim(iq, 7, seg=seg, hide=ALL)
    assert ref[0] == want and ref[1] == wpos


@pytest.mark.parametrize("seg", [20, 33, 57])
def test_stale_cr_and_cr_zero_header_across_the_cut(sim, oracle_mod, seg):
    """The successor decodes its first header under the constructor's d_phdr.cr; the true one is the previous header's - another Hamming class, or 0
    (no branch at all: the header reads as zeros).  A probe that stopped at SYNC carries the true value like one that ran to the header, and the same
    checks apply (rerun_wrong_branch, wrong_fec_branch)."""
    rng = np.random.default_rng(77 + seg)
    pieces = []
    for cr in (4, 0, 4, 2, 0, 0, 3, 4, 1, 4):
        cfg = synth.TxConfig(sf=7, cr=cr)
        p = bytes(rng.integers(0, 256, int(rng.integers(4, 20)), dtype=np.uint8))
        pieces.append(synth.build_stream([p], cfg, rng=rng, tail_symbols=0.0).iq)
    iq = np.concatenate(pieces + [np.zeros(4096, np.complex64)])
    stops = 0
    for ctor_cr in (4, 1):
        want, wpos = _serial(oracle_mod, iq, 7, ctor_cr=ctor_cr)
        got, gpos, stats = sim(iq, 7, ctor_cr=ctor_cr, seg=seg, slots=64)
        assert got == want and gpos == wpos, (seg, ctor_cr)
        stops += stats["stops"]
    assert stops >= 1


def test_noise_with_stale_cr_and_two_streams(sim, oracle_mod):
    """CR 4/5 traffic under noise into a decoder constructed with CR 4 (the successors guess the wrong Hamming class and bit errors make the two
    decodes differ), gradient demodulator, two streams in one pass, burst-aware cuts."""
    cfg = synth.TxConfig(sf=8, cr=1)
    s0 = _packets(10, cfg, 321, length=12, noise_sigma=10 ** (-27 / 20.0))
    s1 = _packets(5, cfg, 322, length=12, noise_sigma=10 ** (-27 / 20.0))
    iq = np.concatenate([s0.iq, s1.iq])
    streams = [(0, s0.iq.size), (s0.iq.size, s1.iq.size)]
    w0, p0 = _serial(oracle_mod, s0.iq, 8, ctor_cr=4, demod=0)
    w1, p1 = _serial(oracle_mod, s1.iq, 8, ctor_cr=4, demod=0)
    for kw in (dict(seg=60), dict(seg=0, slots=8, plan=True)):
        got, gpos, stats = sim(iq, 8, ctor_cr=4, demod=0, streams=streams, **kw)
        assert got == w0 + w1 and gpos == p0 + p1, kw
        assert stats["stream"] == [0] * len(w0) + [1] * len(w1)
