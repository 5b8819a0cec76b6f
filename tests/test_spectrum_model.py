"""CPU: the spectral scan's float64 definition (gr_lora_amd/spectrum.py, include/lora_hip_spectrum.h) against known answers."""
import numpy as np
import pytest

import spectrum_cases as sc
from gr_lora_amd import spectrum


def _tone(n, k0, nfft):
    return np.exp(2j * np.pi * k0 * np.arange(n) / nfft)


@pytest.mark.parametrize("nfft,hop,n_avg,window", [(64, 64, 1, "hann"), (256, 129, 3, "hann"), (1024, 512, 4, "rect"), (128, 1, 5, "hann")])
def test_parseval_per_row(nfft, hop, n_avg, window):
    """A row sums to the windowed mean power of its samples: sum_s sum_n |w[n] x[s hop + n]|^2 / (n_avg sum w^2)."""
    rng = np.random.default_rng(nfft + hop)
    n = (3 * n_avg - 1) * hop + nfft + min(5, n_avg * hop - 1)      # (a partial fourth row)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    psd, peak, band, first = spectrum.welch_rows(x, nfft, hop, n_avg, window)
    w = spectrum.window_table(nfft, window).astype(np.float64)
    assert psd.shape == (3, nfft) and list(first) == [0, n_avg * hop, 2 * n_avg * hop]
    for r in range(3):
        want = sum(np.sum(np.abs(w * x[s * hop:s * hop + nfft]) ** 2) for s in range(r * n_avg, (r + 1) * n_avg)) / (n_avg * np.sum(w * w))
        assert abs(psd[r].sum() - want) <= 1e-12 * want
        assert np.all(peak[r] >= psd[r] * (1 - 1e-12))


@pytest.mark.parametrize("k0", [5, 100, -7, -128])
def test_hann_tone_on_a_bin_centre(k0):
    """A unit tone on bin k0: 2/3 at k0, 1/6 at k0 +- 1 (Hann's three-bin main lobe over sum w^2 = 3 nfft / 8), nothing elsewhere; it
    lands at centred index k0 + nfft / 2, so a negative frequency lands below nfft / 2."""
    nfft = 256
    psd, _, _, _ = spectrum.welch_rows(_tone(4 * nfft, k0, nfft), nfft, nfft // 2, 2)
    i0 = k0 + nfft // 2
    for row in psd:
        assert abs(row[i0] - 2.0 / 3.0) < 1e-6
        for i in ((i0 - 1) % nfft, (i0 + 1) % nfft):
            assert abs(row[i] - 1.0 / 6.0) < 1e-6
        rest = np.delete(row, [(i0 - 1) % nfft, i0, (i0 + 1) % nfft])
        assert rest.max() < 1e-12
    assert (i0 < nfft // 2) == (k0 < 0)
    assert spectrum.freqs(2e6, nfft)[i0] == k0 * 2e6 / nfft and spectrum.freqs(2e6, nfft)[nfft // 2] == 0.0


@pytest.mark.parametrize("nfft", [64, 512, 4096])
def test_rect_tone_is_one_bin_of_one(nfft):
    k0 = nfft // 8 + 3
    psd, peak, _, _ = spectrum.welch_rows(_tone(2 * nfft, k0, nfft), nfft, nfft, 2, "rect")
    assert psd.shape == (1, nfft)
    assert abs(psd[0, k0 + nfft // 2] - 1.0) < 1e-9 and abs(peak[0, k0 + nfft // 2] - 1.0) < 1e-9
    assert np.delete(psd[0], k0 + nfft // 2).max() < 1e-18
    assert np.all(spectrum.window_table(nfft, "rect") == 1.0)


def test_window_table_is_periodic_hann_in_float32():
    w = spectrum.window_table(64)
    assert w.dtype == np.float32 and w[0] == 0.0 and w[32] == 1.0 and w[1] == w[63]
    assert abs(float(np.sum(w.astype(np.float64) ** 2)) - 3 * 64 / 8) < 1e-5
    with pytest.raises(ValueError):
        spectrum.window_table(64, "blackman")


def test_band_bins_edges_are_half_open():
    fs, nfft = 1024e3, 1024                       # 1 kHz per bin, exact
    assert spectrum.band_bins(fs, nfft, 0.0, 1000.0) == (512, 1)           # the centre on f_lo is in, the one on f_hi is out
    assert spectrum.band_bins(fs, nfft, -1000.0, 1000.0) == (511, 2)
    assert spectrum.band_bins(fs, nfft, 0.5, 1000.5) == (513, 1)
    assert spectrum.band_bins(fs, nfft, -3000.0, -1000.0) == (509, 2)      # -3, -2 kHz; -1 kHz sits on f_hi: out
    assert spectrum.band_bins(fs, nfft, -1e9, 1e9) == (0, 1024)            # clipped to the capture
    with pytest.raises(ValueError):
        spectrum.band_bins(fs, nfft, 100.0, 900.0)                         # no bin centre inside
    got = spectrum.grid_bands(2e6, 1024, 0.0, 10, [-2, 0, 1], 125000)
    assert got == [spectrum.band_bins(2e6, 1024, f - 62500.0, f + 62500.0) for f in (-400e3, 0.0, 200e3)]
    assert all(n == 64 for _, n in got)


def test_rows_and_partial_tails():
    """Row r needs (n_avg - 1) hop + nfft samples from r n_avg hop on; a trailing partial row is not emitted."""
    nfft, hop, n_avg = 64, 24, 3
    span = (n_avg - 1) * hop + nfft
    for n, rows in [(0, 0), (span - 1, 0), (span, 1), (span + n_avg * hop - 1, 1), (span + n_avg * hop, 2)]:
        assert spectrum.output_rows(n, nfft, hop, n_avg) == rows
        assert spectrum.welch_rows(np.ones(n), nfft, hop, n_avg)[0].shape[0] == rows
    for bad in [(48, 24, 1), (8192, 1, 1), (64, 0, 1), (64, 65, 1), (64, 64, 0), (64, 64, 1025)]:
        with pytest.raises(ValueError):
            spectrum.check_params(*bad)


def test_to_dbfs():
    assert spectrum.to_dbfs(1.0) == 0.0 and abs(spectrum.to_dbfs(0.0625) + 12.0412) < 1e-3 and spectrum.to_dbfs(0.0) == -200.0


def test_physical_meaning_on_a_gateway_capture():
    """Two SF7 frames on a grid of 10 at 2 Msps (tests/spectrum_cases.py), nfft 1024, hop 512, n_avg 4, bands grid +- 62.5 kHz: for
    every row wholly inside both frames the occupied bands read 10 log10(A^2) within 0.5 dB, every idle band is at least 25 dB
    below the strong emitter, and a row before any frame is exactly 0."""
    x = sc.capture()
    psd, peak, band, first = spectrum.welch_rows(x, sc.NFFT, sc.HOP, sc.N_AVG, bands=sc.bands())
    inside, before = sc.rows_inside_all(first), sc.rows_before_any(first)
    assert len(inside) >= 20 and len(before) >= 1
    db = spectrum.to_dbfs(band[inside])
    amps = [e[3] for e in sc.EMITTERS]
    print("strong %.2f .. %.2f dB, weak %.2f .. %.2f dB" % (db[:, sc.STRONG].min(), db[:, sc.STRONG].max(), db[:, sc.WEAK].min(), db[:, sc.WEAK].max()))
    assert np.abs(db[:, sc.STRONG] - 20 * np.log10(amps[0])).max() <= 0.5
    assert np.abs(db[:, sc.WEAK] - 20 * np.log10(amps[1])).max() <= 0.5
    idle = [c for c in range(len(sc.CHANNELS)) if c not in (sc.STRONG, sc.WEAK)]
    rel = db[:, idle] - db[:, [sc.STRONG]]
    print("worst idle band %.1f dB below the strong emitter" % -rel.max())
    assert rel.max() <= -25.0
    assert np.all(psd[before] == 0.0) and np.all(band[before] == 0.0) and np.all(peak[before] == 0.0)
