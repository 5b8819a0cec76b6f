"""GPU: the multi-SF gateway (include/lora_hip_gateway.h, csrc/lora_gateway.cpp) and the filter bank's many-destination entry
(lora_hip_filterbank_run_device_rows).  Rows: bit for bit what run_device writes, fed the same chunks.  Frames: per (channel,
SF) what the single-SF gateway_receiver and the decoder oracle on that filter-bank row publish, and every transmitted payload."""
import time

import numpy as np
import pytest

from gr_lora_amd import capi, lora, synth

pytestmark = pytest.mark.gpu

SFS = (7, 8, 9, 10, 11, 12)
EU = dict(fs=2e6, M=10, f0=100e3, D=2, ks=list(range(-4, 4)))
US = dict(fs=16e6, M=80, f0=100e3, D=16, ks=list(range(-32, 32)))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU: the HIP path has no CPU fallback")
    return torch


def _noise(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


# ---- rows ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wl", ["a", "b"])
def test_rows_equal_run_device_bit_for_bit(torch_cuda, wl):
    """n_dst = 3 destinations with different row strides, odd (8-byte, not 16-byte aligned) offsets and one in reversed row
    order, streamed in odd chunks (shorter than D, shorter than the filter): every destination holds run_device's bits."""
    torch = torch_cuda
    p = EU if wl == "a" else US
    fs, M, f0, D, ks = p["fs"], p["M"], p["f0"], p["D"], p["ks"]
    nch = len(ks)
    rng = np.random.default_rng(7 if wl == "a" else 9)
    n = 90_001 if wl == "a" else 120_003
    x = _noise(rng, n)
    d_x = torch.from_numpy(x.view(np.float32)).to("cuda")
    ref = capi.FilterBank(fs, f0, M, ks, 125000, D)
    fb = capi.FilterBank(fs, f0, M, ks, 125000, D)
    L = fb.taps().size
    total = fb.output_items(n)
    # destinations (float32 pairs): row c of dst d at base_d + off_d + c * stride_d (dst 2: rows reversed)
    strides = [total + 5, total + 17, total + 3]
    offs = [3, 1, 7]
    bufs = [torch.full((2 * (nch * s + 16),), float("nan"), dtype=torch.float32, device="cuda") for s in strides]
    out_ref = torch.full((nch, 2 * total), float("nan"), dtype=torch.float32, device="cuda")

    def row_base(d, c):
        r = (nch - 1 - c) if d == 2 else c
        return bufs[d].data_ptr() + 8 * (offs[d] + r * strides[d])

    fixed = [1, max(D - 1, 1), L - 1, L // 3, 2 * D + 1, 3]
    pos, got, i = 0, 0, 0
    stream = torch.cuda.current_stream().cuda_stream
    while pos < n:
        c = fixed[i] if i < len(fixed) else int(rng.integers(1, 3 * L))
        c = min(c, n - pos)
        i += 1
        no = fb.output_items(c)
        ptrs = [row_base(d, r) + 8 * got for d in range(3) for r in range(nch)]
        assert fb.run_device_rows(d_x.data_ptr() + 8 * pos, c, ptrs, 3, no, stream) == no
        assert ref.run_device(d_x.data_ptr() + 8 * pos, c, out_ref.data_ptr() + 8 * got, total, stream) == no
        pos += c
        got += no
    assert got == total
    want = out_ref.view(torch.int32).cpu()
    for d in range(3):
        b = bufs[d].view(torch.int32).cpu()
        for r in range(nch):
            rr = (nch - 1 - r) if d == 2 else r
            o = 2 * (offs[d] + rr * strides[d])
            assert torch.equal(b[o:o + 2 * total], want[r]), (d, r)
        # nothing written outside the rows
        mask = torch.ones(b.numel(), dtype=torch.bool)
        for r in range(nch):
            o = 2 * (offs[d] + r * strides[d])
            mask[o:o + 2 * total] = False
        assert torch.isnan(bufs[d].cpu()[mask]).all(), d
    # max_out bounds the call before anything runs
    with pytest.raises(capi.LoraHipError):
        fb.run_device_rows(d_x.data_ptr(), 10 * D, [row_base(0, r) for r in range(nch)], 1, 5, stream)
    ref.close()
    fb.close()


# ---- synthesis -------------------------------------------------------------------------------------------------------

def _tx(sf, payload, fs):
    """One frame at fs: LoRaWAN's LDRO rule, valid header checksum and payload CRC, sync word 0x34 (synth's default)."""
    cfg = synth.TxConfig(sf=sf, cr=4, samp_rate=fs, reduced_rate=lora.lorawan_reduced_rate(sf, 125000),
                         hdr_nibbles=synth.valid_hdr_nibbles(len(payload), 4, True))
    crc = synth.valid_crc_bytes(payload)
    return cfg, crc


def _mixed_capture(p, plan, seed, plen=(4, 12)):
    """Channel ks[i] carries the frames of plan[i] (a list of SFs) one after the other; returns (wide, {(k, sf): [tails]})."""
    fs, M, f0, ks = p["fs"], p["M"], p["f0"], p["ks"]
    rng = np.random.default_rng(seed)
    per, expect = [], {}
    for k, sfs in zip(ks, plan):
        pieces = [np.zeros(int(rng.integers(1000, 40000)), dtype=np.complex64)]
        for sf in sfs:
            pl = bytes(rng.integers(0, 256, int(rng.integers(plen[0], plen[1] + 1)), dtype=np.uint8))
            cfg, crc = _tx(sf, pl, fs)
            st = synth.build_stream([pl], cfg, gaps=[int(rng.integers(2 * cfg.sps, 4 * cfg.sps))], tail_symbols=2.0, crc_bytes=crc)
            pieces.append(st.iq)
            expect.setdefault((k, sf), []).append(synth.expected_frame_tail(pl, cfg, crc))
        per.append(np.concatenate(pieces))
    tail = 3 * (1 << 12) * int(fs / 125000)
    n = max(s.size for s in per) + tail
    wide = np.zeros(n, dtype=np.complex128)
    for k, s in zip(ks, per):
        ph = (f0 + k * fs / M) / fs * np.arange(s.size, dtype=np.float64)
        wide[: s.size] += s * np.exp(2j * np.pi * (ph - np.floor(ph)))
    return wide.astype(np.complex64), expect


EU_PLAN = [[12, 7], [11, 8, 7], [10, 9, 7], [8, 12], [9, 11], [10, 7, 8], [9, 11], [8, 10, 7]]


def _recording(rx):
    """(blob, info) of every frame rx's drain() hands out, in order."""
    rec = []
    inner = rx.gateway.drain

    def drain():
        out = inner()
        rec.extend(out)
        return out
    rx.gateway.drain = drain
    return rec


def _by_pair(rec):
    d = {}
    for blob, info in rec:
        d.setdefault((int(info.grid_index), int(info.sf)), []).append((blob, int(info.header_pos), int(info.end_pos)))
    return d


def _run_multi(p, wide, chunk, device=None, sfs=SFS, latency_ms=None):
    rx = lora.multi_sf_gateway_receiver(p["fs"], 868.0e6, p["f0"], p["M"], p["ks"], 125000, sfs=sfs, decimation=p["D"], latency_ms=latency_ms)
    rec = _recording(rx)
    frames, chan, sff = [], [], []
    rx.subscribe("frames", frames.append)
    rx.subscribe("channel_frames", chan.append)
    rx.subscribe("sf_frames", sff.append)
    src = device if device is not None else wide
    for i in range(0, wide.size, chunk):
        rx.work(src[i:i + chunk])
    rx.stop()
    stats = rx.stats()
    rx.close()
    assert [b for b, _ in rec] == frames == [b for _, b in chan] == [b for _, _, b in sff]
    assert [(k, s) for k, s, _ in sff] == [(int(i.grid_index), int(i.sf)) for _, i in rec]
    return _by_pair(rec), stats


@pytest.fixture(scope="module")
def eu_mixed():
    wide, expect = _mixed_capture(EU, EU_PLAN, seed=868)
    got, stats = _run_multi(EU, wide, 65537)
    return wide, expect, got, stats


def test_eu868_mixed_sf(torch_cuda, eu_mixed, oracle_mod):
    """Per (grid index, SF): every transmitted payload; the decoder oracle on that row of FilterBank.work with the same SF, CR,
    LDRO and demodulator; and gateway_receiver(sf=SF) over the same capture.  Frames one SF's decoder makes of another SF's
    packet are held to the same equalities."""
    wide, expect, got, stats = eu_mixed
    p = EU
    ks = p["ks"]
    for (k, sf), tails in expect.items():
        blobs = [b[15:] for b, _, _ in got.get((k, sf), [])]
        for t in tails:
            assert t in blobs, (k, sf)
    fb = capi.FilterBank(p["fs"], p["f0"], p["M"], ks, 125000, p["D"])
    rows = fb.work(wide)
    fb.close()
    for sf in SFS:
        ldro = lora.lorawan_reduced_rate(sf, 125000)
        gw = lora.gateway_receiver(p["fs"], 868.0e6, p["f0"], p["M"], ks, 125000, sf, False, 4, True, decimation=p["D"], reduced_rate=ldro)
        single = []
        gw.subscribe("channel_frames", single.append)
        for i in range(0, wide.size, 1 << 20):
            gw.work(wide[i:i + (1 << 20)])
        gw.stop()
        gw.close()
        for j, k in enumerate(ks):
            mine = [b for b, _, _ in got.get((k, sf), [])]
            assert mine == [b for kk, b in single if kk == k], (k, sf)
            want = oracle_mod.decode_stream(rows[j], demod=capi.DEMOD_FFT_COMPAT, sf=sf, cr=4, reduced_rate=ldro)
            assert mine == want, (k, sf)
    assert stats["filterbank_calls"] > 0 and stats["items_in"] == wide.size
    assert set(stats["passes"]) == set(SFS) and all(v > 0 for v in stats["passes"].values())
    print("eu868 mixed SF: %d frames, passes %s, filter bank %d calls %.2f ms"
          % (sum(len(v) for v in got.values()), stats["passes"], stats["filterbank_calls"], stats["filterbank_ms"]))


def test_chunking_and_device_input_invariance(torch_cuda, eu_mixed):
    """Host chunks of 65 537 and 1 000 003 and work_device from a torch tensor in chunks of 2^20 + 7: the same blobs and
    positions per (row, SF)."""
    torch = torch_cuda
    wide, expect, got, _ = eu_mixed
    big, _ = _run_multi(EU, wide, 1_000_003)
    assert big == got
    d = torch.from_numpy(wide).to("cuda")
    dev, _ = _run_multi(EU, wide, (1 << 20) + 7, device=d)
    assert dev == got
    d32 = torch.from_numpy(wide.view(np.float32)).to("cuda")
    rx = lora.multi_sf_gateway_receiver(EU["fs"], 868.0e6, EU["f0"], EU["M"], EU["ks"], 125000, sfs=SFS, decimation=EU["D"])
    rec = _recording(rx)
    assert rx.work(d32) == wide.size
    rx.stop()
    rx.close()
    assert _by_pair(rec) == got


def _wideband_sf7(fs, f0, M, ks, payloads_per_channel, seed):
    """test_gpu_filterbank.py's workload: one SF7 transmitter per grid channel, CR 4/8, moved to f0 + kappa fs / M, summed."""
    cfg = synth.TxConfig(sf=7, cr=4, samp_rate=fs)
    rng = np.random.default_rng(seed)
    streams = []
    for k in ks:
        pl = [bytes(rng.integers(0, 256, int(rng.integers(4, 40)), dtype=np.uint8)) for _ in range(payloads_per_channel)]
        streams.append(synth.build_stream(pl, cfg, rng=rng, lead=int(rng.integers(cfg.sps, 6 * cfg.sps))))
    n = max(st.iq.size for st in streams)
    t = np.arange(n, dtype=np.float64)
    wide = np.zeros(n, dtype=np.complex128)
    for k, st in zip(ks, streams):
        ph = (f0 + k * fs / M) / fs * t[: st.iq.size]
        wide[: st.iq.size] += st.iq * np.exp(2j * np.pi * (ph - np.floor(ph)))
    return wide.astype(np.complex64), streams


def test_single_sf_equals_gateway_receiver(torch_cuda):
    """sfs=(7,) on the SF7 EU868-like workload: gateway_receiver(sf=7)'s frames, blob for blob and position for position."""
    p = EU
    wide, streams = _wideband_sf7(p["fs"], p["f0"], p["M"], p["ks"], 4, seed=868)
    gw = lora.gateway_receiver(p["fs"], 868.0e6, p["f0"], p["M"], p["ks"], 125000, 7, False, 4, True, decimation=p["D"])
    rec = []
    inner = gw.mux.drain

    def drain():
        out = inner()
        rec.extend(out)
        return out
    gw.mux.drain = drain
    for i in range(0, wide.size, 65536):
        gw.work(wide[i:i + 65536])
    gw.stop()
    gw.close()
    want = {}
    for blob, info in rec:
        want.setdefault((p["ks"][info.stream], 7), []).append((blob, int(info.header_pos), int(info.end_pos)))
    got, _ = _run_multi(p, wide, 65536, sfs=(7,))
    assert got == want
    assert sum(len(v) for v in got.values()) == 4 * len(p["ks"])


def test_us915_mixed_sf(torch_cuda):
    """64 channels, D 16, one or two frames per channel at random SFs: every payload on its own (grid index, SF), and no
    other CRC-valid frame."""
    rng = np.random.default_rng(915)
    # SF11/12 frames are long at 16 Msps: a few channels carry them, the rest SF7-10
    plan = []
    for i in range(len(US["ks"])):
        if i % 16 == 3:
            plan.append([12])
        elif i % 16 == 9:
            plan.append([11, int(rng.integers(7, 9))])
        else:
            plan.append([int(s) for s in rng.choice([7, 8, 9, 10], size=int(rng.integers(1, 3)), replace=False)])
    wide, expect = _mixed_capture(US, plan, seed=915, plen=(4, 8))
    got, stats = _run_multi(US, wide, 1 << 22)
    valid = {kk: [b[15:] for b, _, _ in v if capi.check_frame(b).crc_ok and capi.check_frame(b).header_checksum_ok] for kk, v in got.items()}
    for kk, tails in expect.items():
        assert valid.get(kk, []) == tails, kk
    assert sum(len(v) for v in valid.values()) == sum(len(t) for t in expect.values())
    print("us915 mixed SF: %d payloads, passes %s" % (sum(len(t) for t in expect.values()), stats["passes"]))


def _latency_run(latency_ms):
    """One SF7 frame on one channel, then silence, three steps in all: less than one batch (2^18 outputs) of every decoder, so
    before stop() only the latency bound launches a pass.  Returns (frames before stop, all frames, stats, the frame's tail)."""
    p = EU
    wide, streams = _wideband_sf7(p["fs"], p["f0"], p["M"], [0], 1, seed=5)
    limit = 3 * capi.GATEWAY_STEP_OUTPUTS * p["D"]
    assert wide.size < limit and limit // p["D"] < 1 << 18
    x = np.concatenate([wide, np.zeros(limit - wide.size, dtype=np.complex64)])
    rx = lora.multi_sf_gateway_receiver(p["fs"], 868.0e6, p["f0"], p["M"], [0], 125000, sfs=(7, 8), decimation=p["D"], latency_ms=latency_ms)
    seen = []
    rx.subscribe("sf_frames", seen.append)
    for i in range(0, limit, 8192):
        rx.work(x[i:i + 8192])
        time.sleep(0.005)
    early = list(seen)
    stats = rx.stats()
    rx.stop()
    rx.close()
    return early, list(seen), stats, synth.expected_frame_tail(streams[0].payloads[0], synth.TxConfig(sf=7, cr=4))


def test_latency_surfaces_a_frame_before_flush(torch_cuda):
    """latency_ms 1: the frame is published while the stream goes on, by a pass the latency bound launched; latency_ms 0 (the
    bound off): nothing before stop(), the same frame at stop()."""
    early, frames, stats, want = _latency_run(1.0)
    assert any(k == 0 and sf == 7 and b[15:] == want for k, sf, b in early), early
    assert stats["passes_by_latency"][7] > 0 and stats["passes"][7] == stats["passes_by_latency"][7], stats
    assert [f for f in frames if f[1] == 7] == [f for f in early if f[1] == 7]   # (nothing more at stop())
    early0, frames0, stats0, _ = _latency_run(0.0)
    assert early0 == [] and stats0["passes"][7] == 0 and stats0["passes_by_latency"][7] == 0, (early0, stats0)
    assert [f for f in frames0 if f[1] == 7] == [f for f in frames if f[1] == 7]


def test_work_after_flush_continues_the_stream(torch_cuda):
    """A flush that launches no pass (less than 2 symbols per row so far) leaves a chunk that is no whole number of steps; the
    stream goes on after it, and every payload behind it is decoded."""
    p = EU
    wide, streams = _wideband_sf7(p["fs"], p["f0"], p["M"], [0], 4, seed=11)
    n = max(wide.size, 6 * capi.GATEWAY_STEP_OUTPUTS * p["D"])
    x = np.concatenate([wide, np.zeros(n - wide.size, dtype=np.complex64)])
    assert not x[:1000].any()
    rx = lora.multi_sf_gateway_receiver(p["fs"], 868.0e6, p["f0"], p["M"], [0], 125000, sfs=(7,), decimation=p["D"], latency_ms=0.0)
    seen = []
    rx.subscribe("sf_frames", seen.append)
    rx.work(x[:1000])
    rx.stop()
    assert rx.stats()["passes"][7] == 0 and seen == []
    for i in range(1000, n, 100_003):
        rx.work(x[i:i + 100_003])
    rx.stop()
    stats = rx.stats()
    rx.close()
    cfg = synth.TxConfig(sf=7, cr=4)
    assert [b[15:] for _, _, b in seen] == [synth.expected_frame_tail(pl, cfg) for pl in streams[0].payloads]
    assert stats["items_in"] == n and stats["step_outputs"] == capi.GATEWAY_STEP_OUTPUTS


def test_device_tensor_checks(torch_cuda):
    """An odd float32 tensor is no whole number of I/Q pairs: refused, nothing consumed."""
    torch = torch_cuda
    rx = lora.multi_sf_gateway_receiver(EU["fs"], 868.0e6, EU["f0"], EU["M"], [0], 125000, sfs=(7,), decimation=EU["D"])
    with pytest.raises(ValueError):
        rx.work(torch.zeros(2 * 4096 + 1, dtype=torch.float32, device="cuda"))
    with pytest.raises(TypeError):
        rx.work(torch.zeros(4096, dtype=torch.float64, device="cuda"))
    assert rx.work(torch.zeros(2 * 4096, dtype=torch.float32, device="cuda")) == 4096
    assert rx.stats()["items_in"] == 4096
    rx.close()
