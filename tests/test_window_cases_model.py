"""No GPU: the three float64 definitions of the pruned dechirp spectrum agree with one another at all 35 shapes, and the window streams of
tests/window_cases.py meet the conditions tests/test_gpu_window_space.py relies on under the committed LIMIT_R."""
import numpy as np
import pytest

import window_cases as WC
from gr_lora_amd import linkmetrics as LM, softdecode as SD
from oracle import preamble_oracle as PO


def _close(a, b):
    return abs(a - b) <= 1e-12 * max(abs(a), abs(b))


@pytest.mark.parametrize("sf,decim", WC.SHAPES)
def test_the_three_definitions_agree_on_the_shared_spectrum(monkeypatch, sf, decim):
    down = WC.model_downchirp(sf, decim)
    st = WC.build(sf, decim, down)
    N, cfg = st.nbins, WC.cfg_of(sf)
    assert len(st.starts) == WC.N_WINDOWS == 13 and st.starts[0] == 3 and all(p & 1 for p in st.starts) and st.iq.dtype == np.complex64
    monkeypatch.setattr(LM, "hann", lambda sps: np.ones(sps))                  # a rectangular window in place of Hann
    for i, pos in enumerate(st.starts):
        x = st.window(i)
        m = SD.magnitudes(st.iq, pos, cfg, down)
        mu = SD.magnitudes(np.conj(x), 0, cfg, down)                           # the "up" half: the spectrum of the conjugate
        assert m.shape == mu.shape == (N,)
        bd, pd, td, bu, pu, tu = PO.window_stats(st.iq, pos, down, N)
        assert _close(pd, m.max() ** 2) and _close(td, (m * m).sum()) and bd == int(np.argmax(m)), (i, pd, m.max() ** 2)
        assert _close(pu, mu.max() ** 2) and _close(tu, (mu * mu).sum()) and bu == int(np.argmax(mu)), (i, pu, mu.max() ** 2)
        for conj, mm in ((False, m), (True, mu)):
            X = LM.window_spectrum(x, down, N, conj)
            assert np.abs(np.abs(X) - mm).max() <= 1e-12 * max(mm.max(), 1e-300), (i, conj)
            rec = LM.window_record(x, down, N, conj)
            assert rec.peak_bin == int(np.argmax(mm)) and _close(rec.peak_power, mm.max() ** 2) and _close(rec.total_power, (mm * mm).sum())
        L, k, peak, tot, _second = SD.llr_window(st.iq, pos, cfg, WC.soft_reduced(i), down)
        assert k == bd and _close(peak * peak, pd) and _close(tot, td) and L.size == (sf - 2 if WC.soft_reduced(i) else sf)


@pytest.mark.parametrize("sf,decim", WC.SHAPES)
def test_on_bin_tones_peak_on_their_bin_and_the_dechirped_window_is_the_stated_signal(sf, decim):
    down = WC.model_downchirp(sf, decim)
    for link in (False, True):
        st = WC.build(sf, decim, down, link)
        assert len(st.starts) == (18 if link else 13) and st.iq.size == 3 + len(st.starts) * st.sps + 2
        assert [b - a for a, b in zip(st.starts, st.starts[1:])] == [st.sps] * (len(st.starts) - 1)           # back to back
        if link:
            assert [LM.window_starts(st.header_pos(f), st.sps) for f in range(3)] == [st.starts[6 * f:6 * f + 6] for f in range(3)]
        assert not st.window(0).any()
        n = np.arange(st.sps)
        for i, k in enumerate(st.tone_k):
            if k is None:
                continue
            assert st.kinds[i] == "on-bin"
            v = st.window(i).astype(np.complex128)
            s = (np.conj(v) if st.conj(i) else v) * down.astype(np.complex128)
            assert np.abs(s - 0.5 * np.exp(2j * np.pi * k * n / st.sps)).max() < 4e-7                          # (complex64 roundings of x and down)
            rec = LM.window_record(st.window(i), down, st.nbins, st.conj(i))
            assert rec.peak_bin == k % st.nbins, (i, k, rec.peak_bin)
            if not link:
                w = PO.window_stats(st.iq, st.starts[i], down, st.nbins)
                assert w[0] == k % st.nbins and abs(np.sqrt(w[1]) - 0.5 * st.sps) < 1e-5 * st.sps
                assert SD.llr_window(st.iq, st.starts[i], WC.cfg_of(sf), WC.soft_reduced(i), down)[1] == k % st.nbins
                # on a tone window sqrt(sps) ||m||_2 is the peak amplitude: err / U counts log2(sps) roundings of the peak
                assert abs(WC.unit_plain(st.window(i), down) / (2.0 ** -24 * np.log2(st.sps)) - 0.5 * st.sps) < 1e-5 * st.sps
        ks = {k % st.nbins for k in st.tone_k if k is not None}
        assert {0, 1, st.nbins - 1, st.nbins // 2 - 1, st.nbins // 2} <= ks


def test_limit_r_is_four_times_the_measured_maximum_and_under_the_cap():
    for kern in WC.KERNELS:
        assert WC.MEASURED_R[kern] is not None and 0.0 < WC.MEASURED_R[kern] * 4.0 <= WC.CAP_R, kern
        assert WC.LIMIT_R[kern] == pytest.approx(4.0 * WC.MEASURED_R[kern], rel=0.01) and WC.LIMIT_R[kern] <= WC.CAP_R == 16.0


@pytest.mark.parametrize("kernel", WC.KERNELS)
def test_set_aside_share_is_under_one_in_ten_and_no_tone_is_set_aside(kernel):
    R = WC.LIMIT_R[kernel]
    total = aside = 0
    per_kind = {}
    for sf, decim in WC.SHAPES:
        down = WC.model_downchirp(sf, decim)
        st = WC.build(sf, decim, down, link=(kernel == "link"))
        for i, (kind, n, a, a_tone) in enumerate(WC.set_aside_census(kernel, st, down, R)):
            total += n
            aside += a
            c = per_kind.setdefault(kind, [0, 0])
            c[0] += n
            c[1] += a
            assert a_tone == 0, (kernel, sf, decim, i, kind)
    print("\n[window cases] %s, R = %.3g: %d of %d index / frac comparisons set aside (%s)"
          % (kernel, R, aside, total, ", ".join("%s %d of %d" % (k, v[1], v[0]) for k, v in per_kind.items())))
    assert total >= 35 * 12 and 10 * aside < total, (kernel, aside, total)
