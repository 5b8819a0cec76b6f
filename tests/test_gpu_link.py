"""GPU: per-frame link metrics (include/lora_hip_link.h; kernel gr_lora_amd/csrc/lora_link.hip) against their float64
definition (gr_lora_amd/linkmetrics.py): lora_hip_link_measure_device at known header positions, windows off the stream, and
the metrics every decoding path attaches to its frames - the batched calls, lora_hip_work's chunk pipeline, the mux, the
multi-SF gateway and the detector path.  Frames carry 4-byte payloads.

Device against model, largest difference seen on the first run and the limit held here, four times it and
never above the cap: see LIMITS."""
import ctypes as C

import numpy as np
import pytest

from gr_lora_amd import capi, linkmetrics as lm, lora, synth

pytestmark = pytest.mark.gpu

BW = 125000
# quantity: limit = four times the largest device-model difference of the first run on an MI355X, which was
#   window powers 1.23e-6 dB, frac 2.02e-7 bin, frame powers 8.62e-7 dB, SNR 1.99e-3 dB where the model's is 40 dB or below and
#   5.94e-3 dB above (total - lobe cancels in fp32 there), CFO 6.07e-8 bin, timing 5.38e-8 bin.
# Caps, never reached: 0.05 dB on powers and SNR (0.5 dB on SNR above 40 dB), 0.01 bin on positions.
LIMITS = dict(window_power_db=4.92e-6, frac=8.08e-7, power_db=3.45e-6, snr_db=7.96e-3, snr_db_high=2.38e-2, cfo_bins=2.43e-7, timing_bins=2.15e-7)
WORST = {k: 0.0 for k in LIMITS}
PAYLOAD = b"\x11\x22\x33\x44"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU: the HIP path has no CPU fallback")
    return torch


def _dev(torch, iq):
    return torch.from_numpy(np.ascontiguousarray(iq, dtype=np.complex64).view(np.float32)).cuda()


def _db(a, b):
    return abs(10.0 * np.log10(a / b)) if a > 0.0 and b > 0.0 else (0.0 if a == b else np.inf)


def _see(name, value, what):
    WORST[name] = max(WORST[name], float(value))
    assert value <= LIMITS[name], (name, value, what)


def _hold_windows(dev_w, model, what):
    """Six device window records against the model's."""
    for i, (g, w) in enumerate(zip(dev_w, model.windows)):
        assert bool(g.valid) == bool(w.valid), (what, i)
        if not w.valid:
            assert (g.peak_bin, g.frac, g.lobe_power, g.total_power, g.peak_power) == (0, 0.0, 0.0, 0.0, 0.0), (what, i)
            continue
        top = np.sort(w.power)[-2:]
        tie = top[1] - top[0] <= 1e-4 * top[1]
        if not tie:
            assert g.peak_bin == w.peak_bin, (what, i, g.peak_bin, w.peak_bin)
        _see("window_power_db", _db(g.total_power, w.total_power), (what, i, "total"))
        if g.peak_bin == w.peak_bin:
            _see("window_power_db", _db(g.lobe_power, w.lobe_power), (what, i, "lobe"))
            _see("window_power_db", _db(g.peak_power, w.peak_power), (what, i, "peak"))
            _see("frac", abs(g.frac - w.frac), (what, i))


def _hold_metrics(g, w, nbins, sps, what):
    """Device metrics (capi.LinkMetrics) against the model's (lm.Metrics)."""
    assert g.flags == w.flags, (what, g.flags, w.flags)
    assert list(g.sync_shift) == w.sync_shift, (what, list(g.sync_shift), w.sync_shift)
    if w.flags & 5:
        _see("power_db", abs(g.rssi_dbfs - w.rssi_dbfs), (what, "rssi"))
        _see("power_db", _db(g.signal_power, w.signal_power), (what, "signal"))
        _see("snr_db_high" if w.snr_db > 40.0 else "snr_db", abs(g.snr_db - w.snr_db), (what, "snr", w.snr_db))
    else:
        assert (g.signal_power, g.noise_power, g.rssi_dbfs, g.snr_db) == (0.0, 0.0, lm.FLOOR_DB, lm.FLOOR_DB), what
    wrap = lambda v: (v + nbins / 2) % nbins - nbins / 2
    _see("cfo_bins", abs(wrap(g.cfo_bins - w.cfo_bins)), (what, "cfo"))
    _see("timing_bins", abs(wrap((g.timing_samples - w.timing_samples) * nbins / sps)), (what, "timing"))
    assert g.cfo_hz == pytest.approx(g.cfo_bins * BW / nbins, rel=1e-12, abs=1e-12)


def _report(name):
    print("\n[link] %s: worst device-model differences so far: %s" % (name, ", ".join("%s %.3g" % kv for kv in WORST.items())))


def _noisy(pieces, sigma, seed):
    iq = np.concatenate(pieces)
    rng = np.random.default_rng(seed)
    return (iq + (rng.standard_normal(iq.size) + 1j * rng.standard_normal(iq.size)) * (sigma / np.sqrt(2.0))).astype(np.complex64)


def _frames(cfg, amps, cfos, gap_symbols=4, tail_symbols=3.0):
    """One frame per (amplitude, cfo), one after the other: (pieces, header positions)."""
    pieces, hdr, pos = [], [], 0
    for a, f in zip(amps, cfos):
        st = synth.build_stream([PAYLOAD], cfg, gaps=[gap_symbols * cfg.sps + 37], tail_symbols=tail_symbols, cfo_hz=f, amplitude=a)
        pieces.append(st.iq)
        hdr.append(pos + st.header_starts[0])
        pos += st.iq.size
    return pieces, hdr


CASES = {
    "sf7_d8": (dict(sf=7, cr=4), 1e6, (1.0, 0.5, 0.25), (-300.0, -300.0, -300.0)),   # the lobe wraps across bin 0
    "sf9_d2": (dict(sf=9, cr=4), 250e3, (0.7, 0.3), (300.0, -5000.0)),
    "sf12_d8": (dict(sf=12, cr=4, reduced_rate=True), 1e6, (0.5,), (1200.0,)),          # LDS above 64 KiB, 16 bins per thread, 4 passes
    "sf6_d8": (dict(sf=6, cr=3, crc=False, implicit=True), 1e6, (0.8, 0.4), (0.0, 700.0)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_measure_device_at_known_headers(torch_cuda, case):
    kw, rate, amps, cfos = CASES[case]
    cfg = synth.TxConfig(samp_rate=rate, **kw)
    pieces, hdr = _frames(cfg, amps, cfos)
    iq = _noisy(pieces, synth.awgn_sigma_for_snr(25.0, cfg), seed=len(case))
    h = capi.Handle(samp_rate=rate, **kw)
    down = h.table(0).view(np.complex64)
    assert down.size == cfg.sps and np.abs(down.astype(np.complex128) - lm.downchirp(cfg.sf, BW, rate)).max() < 1e-5
    dev = _dev(torch_cuda, iq)
    mets, wins = h.measure_link_device(dev.data_ptr(), iq.size, [0], [iq.size], [(0, p) for p in hdr], windows=True)
    st = h.link_stats()
    assert st["launches"] == 1 and st["frames"] == len(hdr) and st["kernel_ms"] > 0.0
    h.close()
    true_cfo = [f * cfg.nbins / BW for f in cfos]
    for i, p in enumerate(hdr):
        want = lm.measure(iq, p, down, cfg.nbins, BW)
        assert want.flags == 7
        _hold_windows(wins[6 * i:6 * i + 6], want, (case, i))
        _hold_metrics(mets[i], want, cfg.nbins, cfg.sps, (case, i))
        # ... and the truth, as far as the model reaches it at 25 dB and below (tests/test_link_model.py)
        assert abs(mets[i].rssi_dbfs - 20.0 * np.log10(amps[i])) <= 1.03, (case, i, mets[i].rssi_dbfs)
        assert abs(mets[i].cfo_bins - true_cfo[i]) <= 0.07 and abs(mets[i].timing_samples) <= 0.45, (case, i, mets[i].cfo_bins, mets[i].timing_samples)
        assert list(mets[i].sync_shift) == [3 * cfg.nbins // 16, cfg.nbins // 4]
    _report(case)


def test_windows_off_the_stream(torch_cuda):
    """Requests whose windows leave the stream at either end: the flags are the model's, nothing outside the stream is read
    (NaN guards either side of it would reach a record) and the guards are as they were."""
    torch = torch_cuda
    cfg = synth.TxConfig(sf=7, cr=4)
    sps = cfg.sps
    pieces, hdr = _frames(cfg, (0.5,), (0.0,))
    iq = _noisy(pieces, synth.awgn_sigma_for_snr(25.0, cfg), seed=3)
    guard = 4 * sps
    buf = torch.full((2 * (iq.size + 2 * guard),), float("nan"), dtype=torch.float32, device="cuda")
    buf[2 * guard:2 * (guard + iq.size)] = torch.from_numpy(iq.view(np.float32)).cuda()
    before = buf.view(torch.int32).clone()
    h = capi.Handle(sf=7, cr=4)
    down = h.table(0).view(np.complex64)
    pos = [3 * sps, iq.size - 2 * sps, hdr[0], iq.size + sps, iq.size + 2 * sps, sps, 0, -5 * sps, iq.size + 100 * sps, 1 << 62, -(1 << 62),
           (25 * sps) // 4, (25 * sps) // 4 - 1, iq.size + sps // 4, iq.size + sps // 4 + 1]
    mets, wins = h.measure_link_device(buf.data_ptr(), iq.size + 2 * guard, [guard], [iq.size], [(0, p) for p in pos], windows=True)
    h.close()
    flags = []
    for i, p in enumerate(pos):
        want = lm.measure(iq, p, down, cfg.nbins, BW)
        flags.append(want.flags)
        assert mets[i].flags == want.flags, (p, mets[i].flags, want.flags)
        for g in wins[6 * i:6 * i + 6]:
            assert np.isfinite([g.frac, g.lobe_power, g.total_power, g.peak_power]).all()
        _hold_windows(wins[6 * i:6 * i + 6], want, ("off", p))
        _hold_metrics(mets[i], want, cfg.nbins, sps, ("off", p))
    assert flags[:2] == [4, 7] and flags[2] == 7 and flags[3] == 3 and 0 in flags and flags[11:] == [7, 6, 7, 3]
    assert torch.equal(buf.view(torch.int32), before)
    _report("off the stream")


def _six_frames(seed=11):
    cfg = synth.TxConfig(sf=7, cr=4, hdr_nibbles=synth.valid_hdr_nibbles(4, 4, True))
    # (the standard decoder acquires from about 35 dB up and decodes within about +-0.4 bin of carrier offset: 40 dB for the weakest frame)
    amps = (1.0, 0.7, 0.5, 0.6, 0.85, 0.9)
    cfos = (0.0, 300.0, -300.0, 150.0, -220.0, 90.0)
    pieces, hdr = _frames(cfg, amps, cfos, gap_symbols=5)
    return cfg, amps, cfos, _noisy(pieces, synth.awgn_sigma_for_snr(40.0, cfg, min(amps)), seed), hdr


def _work_run(iq, chunk, link, **kw):
    h = capi.Handle(sf=7, cr=4, batch_items=8192, **kw)
    if link:
        h.enable_link(True)
    out = []
    for i in range(0, iq.size, chunk):
        h.work(iq[i:i + chunk])
        out += h.drain_link()
    h.flush()
    out += h.drain_link()
    st = h.link_stats()
    h.close()
    return out, st


def _key(m):
    return bytes(m)


def test_work_pipeline_with_link_on(torch_cuda):
    """lora_hip_work in two odd chunkings with a small batch: frames straddle chunks and tail areas (and outgrow the tail area: the
    buffers are reallocated).  Same frames as with link off, every flag set, metrics bit-identical between the chunkings and the
    model's on the whole stream at the reported header positions."""
    cfg, amps, cfos, iq, hdr = _six_frames()
    off, st_off = _work_run(iq, 4099, link=False)
    a, st_a = _work_run(iq, 4099, link=True)
    b, st_b = _work_run(iq, 10007, link=True)
    assert len(off) == 6 and st_off == dict(launches=0, frames=0, kernel_ms=0.0)
    assert all(m.flags == 0 for _, _, m in off)
    for run, st in ((a, st_a), (b, st_b)):
        assert [(f, i.stream, i.header_pos, i.end_pos) for f, i, _ in run] == [(f, i.stream, i.header_pos, i.end_pos) for f, i, _ in off]
        assert all(m.flags == 7 for _, _, m in run)
        assert st["frames"] == 6 and 1 <= st["launches"] <= 6 and st["kernel_ms"] > 0.0
    assert [_key(m) for _, _, m in a] == [_key(m) for _, _, m in b]
    down = lm.downchirp(7)
    for k, (f, info, m) in enumerate(a):
        assert f[15:] == synth.expected_frame_tail(PAYLOAD, cfg)
        assert abs(info.header_pos - hdr[k]) <= 4 * cfg.decim * (1 + abs(cfos[k]) * cfg.nbins / BW)   # (a carrier offset moves the symbol clock the decoder settles on)
        _hold_metrics(m, lm.measure(iq, info.header_pos, down, cfg.nbins, BW), cfg.nbins, cfg.sps, ("work", k))
        assert abs(m.rssi_dbfs - 20.0 * np.log10(amps[k])) <= 0.5
        assert abs(m.cfo_hz - cfos[k]) <= 0.07 * BW / cfg.nbins
    _report("lora_hip_work")


def _mux_run(rows, chunk, link):
    m = capi.Mux(len(rows), sf=7, cr=4, batch_items=8192)
    if link:
        m.enable_link(True)
    out = []
    n = max(r.size for r in rows)
    for i in range(0, n, chunk):
        for c, r in enumerate(rows):
            if i < r.size:
                m.work(c, r[i:i + chunk])
        out += m.drain_link()
    m.flush()
    out += m.drain_link()
    m.close()
    return sorted(out, key=lambda t: (t[1].stream, t[1].header_pos))


def test_mux_with_link_on(torch_cuda):
    cfg = synth.TxConfig(sf=7, cr=4)
    amps = (1.0, 0.4, 0.15)
    rows = []
    for c, a in enumerate(amps):   # (40 dB on every channel: the standard decoder acquires from about 35 dB up)
        pieces, _ = _frames(cfg, (a, a), (100.0 * (c + 1), -120.0 * c), gap_symbols=3 + c)
        rows.append(_noisy(pieces, synth.awgn_sigma_for_snr(40.0, cfg, a), seed=20 + c))
    off = _mux_run(rows, 4099, link=False)
    a = _mux_run(rows, 4099, link=True)
    b = _mux_run(rows, 10007, link=True)
    assert len(off) == 6 and all(m.flags == 0 for _, _, m in off)
    for run in (a, b):
        assert [(f, i.stream, i.header_pos, i.end_pos) for f, i, _ in run] == [(f, i.stream, i.header_pos, i.end_pos) for f, i, _ in off]
        assert all(m.flags == 7 for _, _, m in run)
    assert [_key(m) for _, _, m in a] == [_key(m) for _, _, m in b]
    down = lm.downchirp(7)
    for f, info, m in a:
        _hold_metrics(m, lm.measure(rows[info.stream], info.header_pos, down, cfg.nbins, BW), cfg.nbins, cfg.sps, ("mux", info.stream, info.header_pos))
        assert abs(m.rssi_dbfs - 20.0 * np.log10(amps[info.stream])) <= 0.5
    _report("mux")


def test_multi_sf_gateway_with_link_on(torch_cuda):
    """SF7 and SF9 on two channels of a wide-band capture, 6 dB apart: the "link" messages against the model on the filter bank's rows."""
    fs, M, f0, D, ks = 2e6, 10, 100e3, 2, [0, 2]
    plan = [(7, ks[0], 1.0, 20000), (9, ks[1], 0.5, 30001)]
    frames = []
    for sf, k, amp, start in plan:
        cfg = synth.TxConfig(sf=sf, cr=4, samp_rate=fs, reduced_rate=False, hdr_nibbles=synth.valid_hdr_nibbles(4, 4, True))
        frames.append(synth.WidebandFrame(PAYLOAD, cfg, start, freq_hz=f0 + k * fs / M, amplitude=amp, crc_bytes=synth.valid_crc_bytes(PAYLOAD)))
    n = 30001 + 40 * 512 * 16 + 3 * 512 * 16
    rng = np.random.default_rng(5)
    wide = (synth.build_wideband(frames, fs, 0, n) + (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (0.025 / np.sqrt(2.0))).astype(np.complex64)   # 38 dB in-band for the weaker frame
    rx = lora.multi_sf_gateway_receiver(fs, 868.0e6, f0, M, ks, BW, sfs=(7, 9), decimation=D, reduced_rate=False, link_metrics=True)
    links, blobs = [], []
    rx.subscribe("link", links.append)
    rx.subscribe("frames", blobs.append)
    for i in range(0, n, 65537):
        rx.work(wide[i:i + 65537])
    rx.stop()
    rx.close()
    fbk = lora.filterbank_channelizer(fs, 868.0e6, f0, M, ks, BW, D)
    rows = fbk.work(wide)
    fbk.close()
    assert [l["blob"] for l in links] == blobs
    good = {(l["grid_index"], l["sf"]): l for l in links if l["blob"][15:] == synth.expected_frame_tail(PAYLOAD, frames[0].cfg, frames[0].crc_bytes)}
    assert set(good) >= {(ks[0], 7), (ks[1], 9)}, [(l["grid_index"], l["sf"]) for l in links]
    rssi = {}
    for (k, sf), l in good.items():
        if (k, sf) not in {(ks[0], 7), (ks[1], 9)}:
            continue
        N = 1 << sf
        assert l["row"] == ks.index(k) and l["freq_hz"] == pytest.approx(868.0e6 + f0 + k * fs / M) and l["flags"] == 7
        want = lm.measure(rows[l["row"]], l["header_pos"], lm.downchirp(sf), N, BW)
        got = capi.LinkMetrics(flags=l["flags"], signal_power=l["signal_power"], noise_power=l["noise_power"], rssi_dbfs=l["rssi_dbfs"], snr_db=l["snr_db"],
                               cfo_bins=l["cfo_bins"], cfo_hz=l["cfo_hz"], timing_samples=l["timing_samples"], sync_shift=(C.c_int32 * 2)(*l["sync_shift"]))
        _hold_metrics(got, want, N, 8 * N, ("gateway", k, sf))
        rssi[sf] = l["rssi_dbfs"]
    assert abs((rssi[7] - rssi[9]) - 20.0 * np.log10(2.0)) <= 0.5, rssi
    _report("multi-SF gateway")


def test_detector_path_at_zero_db(torch_cuda):
    """SF9 at 0 dB in-band: acquired by lora_hip_detect_preambles_device, decoded by lora_hip_decode_at_headers_device with link on."""
    cfg = synth.TxConfig(sf=9, cr=4)
    pieces, hdr = _frames(cfg, (1.0, 1.0, 1.0), (0.0, 400.0, -700.0))
    iq = _noisy(pieces, synth.awgn_sigma_for_snr(0.0, cfg), seed=9)
    dev = _dev(torch_cuda, iq)
    h = capi.Handle(sf=9, cr=4, demod=capi.DEMOD_FFT)
    h.enable_link(True)
    det = h.detect_preambles_device(dev.data_ptr(), iq.size, [0], [iq.size])
    assert len(det) == 3
    h.decode_at_headers_device(dev.data_ptr(), iq.size, [0], [iq.size], det)
    out = h.drain_link()
    assert h.link_stats()["launches"] == 1 and h.link_stats()["frames"] == len(out) == 3
    down = h.table(0).view(np.complex64)
    h.close()
    for f, info, m in out:
        print("[link] detector path: header_pos %d snr_db %.3f rssi_dbfs %.3f" % (info.header_pos, m.snr_db, m.rssi_dbfs))
        assert m.flags == 7
        _hold_metrics(m, lm.measure(iq, info.header_pos, down, cfg.nbins, BW), cfg.nbins, cfg.sps, ("detector", info.header_pos))
        assert abs(m.snr_db - 0.0) <= 1.5, m.snr_db
    _report("detector path")


def test_link_off_changes_nothing(torch_cuda):
    import torch
    cfg = synth.TxConfig(sf=7, cr=4)
    pieces, hdr = _frames(cfg, (1.0, 0.5), (0.0, 0.0))
    iq = np.concatenate(pieces)
    dev = _dev(torch, iq)
    h = capi.Handle(sf=7, cr=4)
    h.decode_device(dev.data_ptr(), iq.size, [0], [iq.size], torch.cuda.current_stream().cuda_stream)
    assert h.link_stats() == dict(launches=0, frames=0, kernel_ms=0.0)
    assert h.frames_available() == 2
    blob, info, met = h.poll_frame_link()
    assert blob[15:] == synth.expected_frame_tail(PAYLOAD, cfg) and info.header_pos == hdr[0] and met.flags == 0 and bytes(met) == bytes(80)
    # turned on, the same decode measures; the plain drain hands the frames out as before
    h.enable_link(True)
    h.decode_device(dev.data_ptr(), iq.size, [0], [iq.size], torch.cuda.current_stream().cuda_stream)
    assert h.link_stats()["launches"] == 1 and h.link_stats()["frames"] == 2
    rest = h.drain()
    assert [i.header_pos for _, i in rest] == [hdr[1], hdr[0], hdr[1]]
    # ... and off again
    h.enable_link(False)
    h.decode_device(dev.data_ptr(), iq.size, [0], [iq.size], torch.cuda.current_stream().cuda_stream)
    assert h.link_stats()["launches"] == 1 and all(m.flags == 0 for _, _, m in h.drain_link())
    h.close()
