"""The float64 definition of the link metrics (gr_lora_amd/linkmetrics.py) against the truth of synthesised frames, and
lora_hip_link_combine (host only) against the model's combination.  No GPU.

Limits are twice the worst error of the model over this grid (DESIGN.md 4.14 lists the worst cases: signal power 0.514 dB and
SNR 0.900 dB, both SF7 at 4 dB; CFO 0.035 bin and timing 0.197 sample, both SF7 at 10 dB): signal power 1.03 dB, SNR 1.8 dB for a
true in-band SNR of 4 .. 30 dB, CFO 0.07 bin and timing 0.45 sample from 10 dB up, sync shifts exact."""
import ctypes as C

import numpy as np
import pytest

from gr_lora_amd import linkmetrics as lm
from gr_lora_amd import synth

BW = 125000
CFOS = (0.0, 300.0, -5000.0, 12000.0)
SNRS = (4.0, 10.0, 14.0, 30.0)
AMP = 0.5


def _clean(sf, D, cfo):
    cfg = synth.TxConfig(sf=sf, cr=4, bw=BW, samp_rate=float(BW * D))
    st = synth.build_stream([b"\x01\x02\x03\x04"], cfg, lead=3 * cfg.sps, cfo_hz=cfo, amplitude=AMP)
    hp = st.header_starts[0]
    return cfg, st.iq[:hp + cfg.sps].astype(np.complex128), hp


@pytest.mark.parametrize("D", [8, 2])
@pytest.mark.parametrize("sf", [7, 9, 12])
def test_model_against_truth(sf, D):
    N = 1 << sf
    down = lm.downchirp(sf, BW, float(BW * D))
    worst = dict(power=0.0, snr=0.0, cfo=0.0, timing=0.0)
    for cfo in CFOS:
        cfg, clean, hp = _clean(sf, D, cfo)
        assert cfg.sps == len(down) == N * D
        for snr in SNRS:
            sigma = synth.awgn_sigma_for_snr(snr, cfg, AMP)
            for seed in (1, 2):
                rng = np.random.default_rng(1000 * seed + sf)
                x = clean + (rng.standard_normal(clean.size) + 1j * rng.standard_normal(clean.size)) * (sigma / np.sqrt(2.0))
                for tau in (0, 1, -1, D // 2):
                    m = lm.measure(x, hp + tau, down, N, BW)
                    assert m.flags == 7
                    e_p = abs(m.rssi_dbfs - 20.0 * np.log10(AMP))
                    e_s = abs(m.snr_db - snr)
                    worst["power"], worst["snr"] = max(worst["power"], e_p), max(worst["snr"], e_s)
                    assert e_p <= 1.03, (sf, D, cfo, snr, seed, tau, m.rssi_dbfs)
                    assert e_s <= 1.8, (sf, D, cfo, snr, seed, tau, m.snr_db)
                    assert m.sync_shift == [3 * N // 16, N // 4], (sf, D, cfo, snr, seed, tau, m.sync_shift)
                    if snr >= 10.0:
                        e_c = abs(m.cfo_bins - cfo * N / BW)
                        e_t = abs(m.timing_samples - tau)
                        worst["cfo"], worst["timing"] = max(worst["cfo"], e_c), max(worst["timing"], e_t)
                        assert e_c <= 0.07, (sf, D, cfo, snr, seed, tau, m.cfo_bins)
                        assert e_t <= 0.45, (sf, D, cfo, snr, seed, tau, m.timing_samples)
                        assert m.cfo_hz == pytest.approx(m.cfo_bins * BW / N)
    print("SF%d D%d worst errors: power %.3f dB, SNR %.3f dB, CFO %.4f bin, timing %.3f sample" % (sf, D, worst["power"], worst["snr"], worst["cfo"], worst["timing"]))


def test_snr_estimate_saturates_above_forty_db():
    """Without noise the estimate is the window's leakage floor: it levels off, it does not diverge."""
    cfg, clean, hp = _clean(7, 8, 300.0)
    m = lm.measure(clean, hp, lm.downchirp(7), 128, BW)
    assert 38.0 <= m.snr_db <= 60.0
    assert abs(m.rssi_dbfs - 20.0 * np.log10(AMP)) <= 0.1


def test_validity_flags_at_the_streams_ends():
    sf, N = 7, 128
    cfg, clean, hp = _clean(sf, 8, 0.0)
    down, sps = lm.downchirp(sf), cfg.sps
    starts = lm.window_starts(hp, sps)
    assert starts == [hp - (25 * sps) // 4, hp - (25 * sps) // 4 + sps, hp - (17 * sps) // 4, hp - (17 * sps) // 4 + sps,
                      hp - (9 * sps) // 4, hp - (9 * sps) // 4 + sps]
    # the stream begins inside the preamble pair / the sync pair / the SFD pair: the pairs in front go
    for cut, flags in ((starts[0], 7), (starts[0] + 1, 6), (starts[2], 6), (starts[2] + 1, 4), (starts[4], 4), (starts[4] + 1, 0)):
        m = lm.measure(clean[cut:], hp - cut, down, N, BW)
        assert m.flags == flags, (cut, m.flags)
        if not flags & 1:
            assert m.cfo_bins == 0.0 and m.timing_samples == 0.0 and m.sync_shift == [0, 0]
        if flags == 0:
            assert m.signal_power == 0.0 and m.rssi_dbfs == lm.FLOOR_DB and m.snr_db == lm.FLOOR_DB
        for w, s in zip(m.windows, starts):
            assert bool(w.valid) == (s - cut >= 0)
    # the stream ends inside the SFD pair (a header two symbols before the end and further)
    for end, flags in ((starts[5] + sps, 7), (starts[5] + sps - 1, 3), (starts[3] + sps - 1, 1), (starts[1] + sps - 1, 0)):
        assert lm.measure(clean[:end], hp, down, N, BW).flags == flags
    # ... and a header right at the start: nothing in front of it
    assert lm.measure(clean, 3 * sps, down, N, BW).flags == 4
    assert lm.measure(clean, 0, down, N, BW).flags == 0


def _lib():
    from gr_lora_amd import build, capi
    build.build_library()
    return capi, capi.load()


def _c_combine(capi, lib, recs, sps, N, bw):
    arr = (capi.LinkWindow * 6)()
    for i, w in enumerate(recs):
        arr[i] = capi.LinkWindow(w.peak_bin, w.frac, w.lobe_power, w.total_power, w.peak_power, w.valid)
    out = capi.LinkMetrics()
    assert lib.lora_hip_link_combine(arr, sps, N, float(bw), C.byref(out)) == 0
    return out


def _f32(w):
    """A model record as the device's struct holds it."""
    f = lambda v: float(np.float32(v))
    return lm.WindowRecord(w.peak_bin, f(w.frac), f(w.lobe_power), f(w.total_power), f(w.peak_power), w.valid)


@pytest.mark.parametrize("sf,D,cfo,cut", [(7, 8, -300.0, 0), (9, 2, 12000.0, 0), (12, 8, -5000.0, 0), (7, 8, 300.0, 1), (7, 8, 300.0, 2)])
def test_c_combine_matches_the_model(sf, D, cfo, cut):
    capi, lib = _lib()
    N = 1 << sf
    cfg, clean, hp = _clean(sf, D, cfo)
    rng = np.random.default_rng(sf)
    x = clean + (rng.standard_normal(clean.size) + 1j * rng.standard_normal(clean.size)) * (synth.awgn_sigma_for_snr(12.0, cfg, AMP) / np.sqrt(2.0))
    starts = lm.window_starts(hp, cfg.sps)
    off = 0 if cut == 0 else starts[0] + 1 if cut == 1 else starts[2] + 1   # nothing / the preamble pair / preamble and sync pairs invalid
    m = lm.measure(x[off:], hp - off, lm.downchirp(sf, BW, float(BW * D)), N, BW)
    recs = [_f32(w) for w in m.windows]
    want = lm.combine(recs, cfg.sps, N, BW)
    got = _c_combine(capi, lib, recs, cfg.sps, N, BW)
    assert got.flags == want.flags == m.flags
    for name in ("signal_power", "noise_power", "rssi_dbfs", "snr_db", "cfo_bins", "cfo_hz", "timing_samples"):
        assert getattr(got, name) == pytest.approx(getattr(want, name), rel=1e-9, abs=1e-12), name
    assert list(got.sync_shift) == want.sync_shift


def test_c_combine_wraps_like_the_model():
    """Positions either side of the +-N/2 wrap, and a lobe that is all there is (no noise: the levels stay finite)."""
    capi, lib = _lib()
    N, sps = 128, 1024
    mk = lambda b, f, lobe=1000.0, tot=1100.0: lm.WindowRecord(b, f, lobe, tot, 0.6 * lobe, 1)
    recs = [_f32(r) for r in (mk(63, 0.4), mk(64, -0.3), mk(87, 0.2), mk(96, -0.45), mk(64, 0.1), mk(64, 0.3))]
    want, got = lm.combine(recs, sps, N, BW), _c_combine(capi, lib, recs, sps, N, BW)
    for name in ("signal_power", "noise_power", "rssi_dbfs", "snr_db", "cfo_bins", "cfo_hz", "timing_samples"):
        assert getattr(got, name) == pytest.approx(getattr(want, name), rel=1e-9, abs=1e-12), name
    assert list(got.sync_shift) == want.sync_shift
    assert abs(want.cfo_bins) < 1.0 and abs(abs(want.timing_samples) - 64 * 8) < 8.0
    quiet = [mk(0, 0.0, 500.0, 500.0)] * 6
    want, got = lm.combine(quiet, sps, N, BW), _c_combine(capi, lib, quiet, sps, N, BW)
    assert got.snr_db == want.snr_db == 200.0 and got.noise_power == 0.0
    none = [lm.WindowRecord()] * 6
    got = _c_combine(capi, lib, none, sps, N, BW)
    assert got.flags == 0 and got.rssi_dbfs == got.snr_db == -200.0 and got.signal_power == 0.0
