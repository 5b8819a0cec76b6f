"""What a stream carries from one device pass to the next - the resume position, d_phdr.cr and the power state behind the SNR byte (pipe_collect /
pipe_rotate in lora_runtime.cpp, by the rule of lora_stitch.hpp's carry_collect / carry_launch) - on the device, through every streaming entry point:
lora_hip_work, the mux, the gateway.  The traffic is tests/stream_carry_cases.py's, whose packets change the coding rate from one to the next (the next
header's FEC branch follows the previous packet's CR, CR 0 included: decoder_impl.cc:655); batch_items is chosen so that passes end inside packets.
Every stream must equal the serial oracle run once over all of it: blobs with their SNR byte, absolute header positions, no frame twice, none
missing.  (tests/test_stream_carry_sim.py holds the same carry, pass by pass, to the serial decoder's state on the CPU.)"""
import numpy as np
import pytest

import stream_carry_cases as cases
from gr_lora_amd import synth

pytestmark = pytest.mark.gpu

_cache = {}


def _workload(name, *args):
    """the workload and the serial oracle's frames and header positions over the whole stream, computed once"""
    key = (name,) + args
    if key not in _cache:
        from oracle import oracle as O
        w = getattr(cases, name)(*args)
        o = O.Oracle(sf=w.sf, cr=w.ctor_cr, demod=w.demod)
        o.run(w.iq)
        _cache[key] = (w, list(zip(o.frames(), o.frame_positions())))
    return _cache[key]


def _equal(got, want, what):
    gpos, wpos = [p for _, p in got], [p for _, p in want]
    assert len(set(gpos)) == len(gpos), (what, "a frame was published twice", gpos)
    assert gpos == wpos, (what, gpos, wpos)
    assert got == want, (what, [i for i, (g, t) in enumerate(zip(got, want)) if g != t])


def _stream(h, iq, call_items):
    """-> frames with their header positions; the most segment jobs a pass was cut into (lora_hip_last_timing describes the pass the call launched)"""
    got, jobs = [], 0
    for lo in range(0, iq.size, call_items):
        h.work(iq[lo:lo + call_items])
        got += [(b, i.header_pos) for b, i in h.drain()]
        jobs = max(jobs, h.timing().jobs)
    h.flush()
    got += [(b, i.header_pos) for b, i in h.drain()]
    return got, jobs


@pytest.mark.parametrize("decoupled", ["0", "1"])
@pytest.mark.parametrize("name,args,kernel,no_fast", [
    ("header_cr_zero", (), "walker2_kernel_sf7", False),
    ("header_cr_zero", (9, 6), "walker3_kernel_sf9", False),
    ("header_cr_zero", (), "walker_kernel", True),
    ("mixed_cr_noisy", (), "walker2_kernel_sf8_grad", False),
    ("alternating_cr_idle_noise", (), "walker2_kernel_sf7", False),
])
def test_work_in_small_passes_equals_the_serial_oracle(oracle_mod, monkeypatch, name, args, kernel, no_fast, decoupled):
    """lora_hip_work with a small batch_items, then flush: the wave-per-symbol walker (SF7, SF8 with the gradient demodulator: demod 2 and 0), walker3
    (SF9) and the generic kernels (LORA_HIP_NO_FAST), each with LORA_HIP_DECOUPLED 0 (ordinary passes) and 1 (every pass decoupled where the kernel has a
    header-only variant: a streaming handle's payload-pass counters are cleared by the next pass's launch, inside the same work() call that collected
    them, so that such passes ran is asserted where it can be read, in test_decode_device_on_a_prefix_then_a_fresh_handle_from_the_resume_point)"""
    from gr_lora_amd import capi
    w, want = _workload(name, *args)
    assert len(want) == len(w.crs)
    monkeypatch.setenv("LORA_HIP_DECOUPLED", decoupled)
    if no_fast:
        monkeypatch.setenv("LORA_HIP_NO_FAST", "1")
    sps = w.sps
    # 23 and 61 symbols and 11 / 17 items: about every pass ends inside a packet (they span 30 to 60 symbols), at another point of it each time, and
    # the longer passes are cut into speculation segments (segment_symbols 16)
    for batch, seg in ((23 * sps + 11, 0), (61 * sps + 17, 16)):
        h = capi.Handle(sf=w.sf, cr=w.ctor_cr, demod=w.demod, batch_items=batch, segment_symbols=seg)
        h.set_stream_latency(0.0)
        assert h.kernel_name() == kernel or (no_fast and h.kernel_name().startswith(kernel)), h.kernel_name()
        got, jobs = _stream(h, w.iq, 50000)
        si = h.stream_info()
        h.close()
        _equal(got, want, (name, args, batch, decoupled))
        assert si.passes >= w.iq.size // batch, (si.passes, w.iq.size // batch)
        print(name, args, batch, seg, "passes", si.passes, "most jobs in a pass", jobs)
        if seg:
            assert jobs >= 4, jobs    # 61 symbols and the carried items in segments of 16: the segmented path ran
        assert si.resume_pos == si.consumed_base <= w.iq.size


@pytest.mark.parametrize("decoupled", ["0", "1"])
@pytest.mark.parametrize("name,args,kernel", [("header_cr_zero", (), "walker2_kernel_sf7"), ("header_cr_zero", (9, 6), "walker3_kernel_sf9"),
                                              ("mixed_cr_noisy", (), "walker2_kernel_sf8_grad")])
def test_decode_device_on_a_prefix_then_a_fresh_handle_from_the_resume_point(oracle_mod, monkeypatch, name, args, kernel, decoupled):
    """lora_hip_decode_device over iq[:cut], then the rest from the resume point lora_hip_stream_info_ex reports (resume_pos, resume_cr - added for
    this at the end of lora_hip_stream_info_t, behind a struct_size argument) with a fresh handle constructed with that CR.  The first part must be
    the oracle's frames ahead of resume_pos, the second the oracle's frames from there on: positions and the bytes behind the loratap header (the
    power queue is not handed over, so the SNR byte of the first frame of the second part may differ; the work() cases hold it).  With the pending
    packet's own CR instead - what the stitch used to report - the packets behind a CR-0 header come out as other frames."""
    import torch
    from gr_lora_amd import capi
    w, want = _workload(name, *args)
    monkeypatch.setenv("LORA_HIP_DECOUPLED", decoupled)
    dev = torch.from_numpy(w.iq.view(np.float32)).cuda()
    packets = (1, 2, 5) if name == "header_cr_zero" else (3, 6)
    payload_packets = 0
    for k, kind, cut in w.cuts(packets=[p for p in packets if p < len(w.crs)], kinds=["header", "payload"]) + w.cuts(packets=[4], kinds=["preamble", "gap"]):
        for seg in (0, 16):
            h = capi.Handle(sf=w.sf, cr=w.ctor_cr, demod=w.demod, segment_symbols=seg)
            assert h.kernel_name() == kernel, h.kernel_name()
            h.decode_device(dev.data_ptr(), cut, [0], [cut], 0)
            first = [(b[15:], i.header_pos) for b, i in h.drain()]
            si = h.stream_info()
            payload_packets += h.payload_pass()["packets"]
            jobs = h.timing().jobs
            h.close()
            assert jobs >= (4 if seg else 1), (seg, jobs)
            pos, cr = int(si.resume_pos), int(si.resume_cr)
            assert 0 <= pos <= cut
            h = capi.Handle(sf=w.sf, cr=cr, demod=w.demod, segment_symbols=seg)
            h.decode_device(dev.data_ptr() + 8 * pos, w.iq.size - pos, [0], [w.iq.size - pos], 0)
            rest = [(b[15:], i.header_pos + pos) for b, i in h.drain()]
            h.close()
            n = len(first)
            _equal(first, [(b[15:], p) for b, p in want[:n]], (name, args, k, kind, seg, "ahead of the resume point", pos, cr))
            assert all(p >= pos for _, p in want[n:]) and all(p < pos for _, p in want[:n]), (k, kind, pos)
            _equal(rest, [(b[15:], p) for b, p in want[n:]], (name, args, k, kind, seg, "from the resume point", pos, cr))
    assert (payload_packets > 0) == (decoupled == "1"), (decoupled, payload_packets)   # LORA_HIP_DECOUPLED did what the test means it to


def test_mux_channels_chunked_differently_equal_their_own_oracles(oracle_mod):
    """three channels of one mux carry the three SF7 workloads - CR-0 headers, alternating CR under idle noise, and the CR-0 traffic again from its
    third packet on - fed in calls of another size each, one of them in 4096-item calls; every channel must equal its own oracle"""
    from gr_lora_amd import capi
    from oracle import oracle as O
    w0, want0 = _workload("header_cr_zero")
    w1, want1 = _workload("alternating_cr_idle_noise")
    iq2 = w0.iq[w0.frame_starts[2] - 3000:]
    o = O.Oracle(sf=7, cr=4, demod=2)
    o.run(iq2)
    want = [want0, want1, list(zip(o.frames(), o.frame_positions()))]
    chans = [w0.iq, w1.iq, iq2]
    for batch in (19 * 1024 + 5, 47 * 1024 + 301):
        m = capi.Mux(3, sf=7, cr=4, batch_items=batch)
        m.set_latency(0.0)
        got = {c: [] for c in range(3)}
        pos, call = [0, 0, 0], [4096, 30011, 7 * 1024 + 3]
        while any(pos[c] < chans[c].size for c in range(3)):
            for c in range(3):
                if pos[c] < chans[c].size:
                    m.work(c, chans[c][pos[c]:pos[c] + call[c]])
                    pos[c] += call[c]
            for b, i in m.drain():
                got[i.stream].append((b, i.header_pos))
        m.flush()
        for b, i in m.drain():
            got[i.stream].append((b, i.header_pos))
        m.close()
        for c in range(3):
            _equal(got[c], want[c], ("mux", batch, c))


def test_gateway_channels_of_mixed_cr_traffic(oracle_mod):
    """lora.gateway_receiver (filter bank -> one mux, a decoder per channel) on tests/spectrum_cases.py's grid: two emitters' channels carry six packets
    each of mixed CR, CR 0 included, and batch_items ends the passes inside them.  Per channel: what the serial oracle makes of that channel's samples -
    blobs, header positions (taken from the mux behind the receiver: its message ports carry blobs only), no frame twice.  The channel's samples are
    the device filter bank's row over the whole capture in ONE call: this relies on the filter bank's output being bit-identical however its input is
    chunked (every output item is one sum in a fixed order over its own input window), since the receiver runs it in 50000-item calls."""
    import spectrum_cases as sc
    from gr_lora_amd import lora
    from oracle import oracle as O
    y, per_channel = cases.gateway_capture(sc.FS, sc.BANDWIDTH, 200e3)
    fb = lora.filterbank_channelizer(sc.FS, 0.0, sc.GRID_OFFSET, sc.N_GRID, sc.CHANNELS, sc.BANDWIDTH, decimation=2)
    rows = fb.work(y)
    fb.close()
    want = {}
    for k in per_channel:
        o = O.Oracle(sf=7, cr=4, demod=2)
        o.run(np.ascontiguousarray(rows[sc.CHANNELS.index(k)]))
        want[k] = list(zip(o.frames(), o.frame_positions()))
        # (the oracle decides what these samples hold; that the traffic is what it is meant to be: the first packet carries its payload, and a packet
        # behind a CR-0 header reads as the all-zero header)
        tails = [f[15:] for f, _ in want[k]]
        f0 = per_channel[k][0]
        assert len(tails) >= 4 and tails[0] == synth.expected_frame_tail(f0.payload, f0.cfg, f0.crc_bytes), (k, len(tails))
        assert any(t[:3] == bytes(3) for t in tails), (k, [t.hex() for t in tails])
    for batch in (21 * 1024 + 7, 64 * 1024):
        rx = lora.gateway_receiver(sc.FS, 0.0, sc.GRID_OFFSET, sc.N_GRID, sc.CHANNELS, sc.BANDWIDTH, 7, False, 4, True, decimation=2, batch_items=batch,
                                   latency_ms=0)
        seen, infos, drain = [], [], rx.mux.drain
        rx.mux.drain = lambda: [infos.append(x) or x for x in drain()]   # (what the receiver publishes from, with the frames' positions)
        rx.subscribe("channel_frames", seen.append)
        for lo in range(0, y.size, 50000):
            rx.work(y[lo:lo + 50000])
        rx.stop()
        rx.close()
        assert [(int(k), blob) for k, blob in seen] == [(sc.CHANNELS[i.stream], blob) for blob, i in infos]
        got = {k: [(blob, i.header_pos) for blob, i in infos if sc.CHANNELS[i.stream] == k] for k in per_channel}
        assert sum(len(v) for v in got.values()) == len(infos), [sc.CHANNELS[i.stream] for _, i in infos]
        for k in per_channel:
            _equal(got[k], want[k], ("gateway", batch, k))
