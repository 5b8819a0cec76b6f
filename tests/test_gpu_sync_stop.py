"""GPU: tail probes that end at SYNC (SF7 / SF8 at decimation 8, both demodulators; lora_walker2.inc.hip kSyncStop, lora_stitch.hpp tail_at_sync).
The smallest streams that still have two cuts - six packets of 8 bytes in one stream, three in a second, segments of 70 symbols - decoded clean and
under 40 dB of SNR (where about every second cut's probe leaves SYNC one sample beside its successor and must run on), with gaps of 2 and of 6
symbols, and one stream whose last packet the end of the data cuts.  Frames, header positions and loratap bytes against the oracle, and against the
same decode with LORA_HIP_NO_SYNC_STOP=1 in a fresh process; the number of probes that stopped against what the CPU simulation of the same streams
allows (tests/host_sim/sync_stop_sim.cpp: a probe may stop only where the two positions are the same) - and on clean streams some must stop."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from gr_lora_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = 70                      # segment_symbols (as tests/test_gpu_strict_sync.py: a packet and its gap are 46 to 50 symbols)
CONFIGS = [(7, 2), (7, 0), (8, 2), (8, 0)]


def cases(sf):
    """[(name, iq, [(offset, length)], clean)] - the same for both demodulators"""
    cfg = synth.TxConfig(sf=sf, cr=4)
    sps = cfg.sps
    out = []
    for gap in (2.0, 6.0):
        for snr in (None, 40.0):
            rng = np.random.default_rng(1000 * sf + int(10 * gap) + (1 if snr else 0))
            sigma = synth.awgn_sigma_for_snr(snr, cfg) if snr else 0.0
            parts = []
            for n, lead in ((6, 1.37), (3, 2.71)):     # (leads off the symbol grid: a scan that steps exactly onto a preamble's first sample leaves SYNC a symbol early)
                payloads = [bytes(rng.integers(0, 256, 8, dtype=np.uint8)) for _ in range(n)]
                parts.append(synth.build_stream(payloads, cfg, rng=rng, gap_symbols=(gap, gap), lead=int(lead * sps), noise_sigma=sigma).iq)
            iq = np.concatenate(parts)
            out.append(("gap%d_%s" % (gap, "snr40" if snr else "clean"), iq, [(0, parts[0].size), (parts[0].size, parts[1].size)], snr is None))
    rng = np.random.default_rng(77 + sf)
    payloads = [bytes(rng.integers(0, 256, 8, dtype=np.uint8)) for _ in range(6)]
    st = synth.build_stream(payloads, cfg, rng=rng, gap_symbols=(2.0, 6.0), lead=int(1.37 * sps))
    cut = st.iq[: st.header_starts[-1] + 14 * sps]       # the data ends inside the last packet's payload
    out.append(("cut_by_end", cut, [(0, cut.size)], True))
    return out


def decode_all(torch):
    """{(sf, demod, case): (frames per stream, jobs, tail probes, probes stopped at SYNC)} on the device, one handle per case"""
    from gr_lora_amd import capi
    res = {}
    for sf, demod in CONFIGS:
        for name, iq, streams, _ in cases(sf):
            h = capi.Handle(sf=sf, cr=4, demod=demod, segment_symbols=SEG)
            dev = torch.from_numpy(np.ascontiguousarray(iq).view(np.float32)).to("cuda:0")
            h.decode_device(dev.data_ptr(), iq.size, [s[0] for s in streams], [s[1] for s in streams], torch.cuda.current_stream().cuda_stream)
            per = {}
            for blob, info in h.drain():
                per.setdefault(int(info.stream), []).append((bytes(blob), int(info.header_pos)))
            tails, stops = h.sync_stops()
            res[(sf, demod, name)] = (per, int(h.timing().jobs), tails, stops)
            h.close()
    return res


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU: the HIP path has no CPU fallback")
    return torch


@pytest.fixture(scope="module")
def device_runs(torch_cuda, tmp_path_factory):
    """every case decoded here, and again in ONE fresh process with LORA_HIP_NO_SYNC_STOP=1 (the switch is read once per process)"""
    assert "LORA_HIP_NO_SYNC_STOP" not in os.environ
    # LORA_HIP_DECOUPLED=0 (read when a handle is made): passes this small would otherwise run decoupled - header-only jobs, which have no tail probes
    saved = os.environ.get("LORA_HIP_DECOUPLED")
    os.environ["LORA_HIP_DECOUPLED"] = "0"
    try:
        on = decode_all(torch_cuda)
    finally:
        if saved is None:
            del os.environ["LORA_HIP_DECOUPLED"]
        else:
            os.environ["LORA_HIP_DECOUPLED"] = saved
    out = str(tmp_path_factory.mktemp("sync_stop") / "off.pkl")
    env = dict(os.environ, LORA_HIP_NO_SYNC_STOP="1", LORA_HIP_DECOUPLED="0", PYTHONPATH=os.pathsep.join([ROOT] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    with open(out, "rb") as f:
        off = pickle.load(f)
    return on, off


@pytest.fixture(scope="module")
def sim(oracle_mod):
    from test_sync_stop_sim import load_sim
    return load_sim()


@pytest.mark.gpu
@pytest.mark.parametrize("sf,demod", CONFIGS)
def test_tail_probes_that_end_at_sync_change_nothing(device_runs, oracle_mod, sim, sf, demod):
    on, off = device_runs
    clean_stops = 0
    for name, iq, streams, clean in cases(sf):
        per, jobs, tails, stops = on[(sf, demod, name)]
        want = {}
        for i, (o, n) in enumerate(streams):
            orc = oracle_mod.Oracle(sf=sf, cr=4, demod=demod)
            orc.run(iq[o:o + n])
            if orc.frames():
                want[i] = list(zip(orc.frames(), orc.frame_positions()))
        assert per == want, (name, "against the oracle")
        assert sum(len(v) for v in want.values()) == (5 if name == "cut_by_end" else 9), name
        per_off, jobs_off, tails_off, stops_off = off[(sf, demod, name)]
        assert per_off == per and jobs_off == jobs, (name, "against LORA_HIP_NO_SYNC_STOP=1")
        assert stops_off == 0 and tails_off == tails, (name, tails_off, stops_off)
        assert jobs >= (3 if name == "cut_by_end" else 6), (name, jobs)          # at least three segment jobs per stream: two cuts
        # a probe stops only where the CPU simulation finds the two SYNC exits at the same sample (on the device it may also come too early to see
        # its successor's); under noise that leaves the cuts that are one sample off running on
        _, _, s = sim(iq, sf, demod=demod, seg=SEG, streams=streams)
        print(sf, demod, name, "jobs", jobs, "tail probes", tails, "stopped at SYNC", stops, "simulation", s["stops"], "positions that differ", s["differ"])
        assert tails >= 2, (name, tails)                                          # the pass ran with tail probes (not decoupled), one per cut
        assert stops <= s["stops"] and stops <= tails, (name, stops, s)
        if clean:
            clean_stops += stops
            assert s["stops"] == 0 or stops >= 1, (name, stops, s)               # (every job of these launches is resident from the start: the successors publish early)
    assert clean_stops >= 1, "no tail probe stopped at SYNC on the clean streams: the feature is dead"


if __name__ == "__main__":   # the child process of device_runs
    import torch
    with open(sys.argv[1], "wb") as f:
        pickle.dump(decode_all(torch), f)
