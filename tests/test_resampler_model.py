"""CPU: the rational resampler's float64 definition (gr_lora_amd/resampler.py, include/lora_hip_resampler.h) - the prototype
filter's quality, the output count, a tone through it, a real frame up and down again on the oracle decoder, the ratio helper.

Measured with the default design (Z = 16, beta = 8, c = 0.8), worst of the six ratios below: passband ripple 0.0007 dB, stop band
-81.5 dB, DC gain error 1.1e-5."""
import numpy as np
import pytest

from gr_lora_amd import resampler, synth

RATIOS = [(5, 12), (125, 256), (25, 24), (12, 5), (1, 2), (3, 1)]


def _response_db(L, M):
    """|H| / L of the prototype on a fine grid, in dB, with the grid in units of the lower Nyquist rate."""
    h = resampler.design(L, M).astype(np.float64)
    R = max(L, M)
    nfft = 1 << int(np.ceil(np.log2(h.size * 64)))
    H = np.abs(np.fft.rfft(h, nfft)) / L
    f = np.arange(H.size) / nfft * 2.0 * R          # 1.0 = the lower of the two Nyquist rates
    return f, 20.0 * np.log10(np.maximum(H, 1e-30)), float(h.sum()) / L


@pytest.mark.parametrize("L,M", RATIOS)
def test_filter_quality(L, M):
    f, db, dc = _response_db(L, M)
    ripple = float(np.abs(db[f <= 0.6]).max())
    stop = float(db[f >= 1.0].max())
    print("resampler filter %d/%d: ripple %.4f dB, stop band %.1f dB, DC gain error %.2g" % (L, M, ripple, stop, abs(dc - 1.0)))
    assert ripple <= 0.01
    assert stop <= -80.0
    assert abs(dc - 1.0) <= 1e-4
    h = resampler.design(L, M)
    assert h.dtype == np.float32 and h.size == 2 * 16 * max(L, M) + 1 == resampler.n_taps(L, M)
    assert np.array_equal(h, h[::-1]) and h.argmax() == 16 * max(L, M)        # linear phase: the delay is Z R taps


@pytest.mark.parametrize("L,M,chunks", [
    (5, 6, [1, 1, 1, 4, 0, 6, 7919]),
    (125, 128, [127, 1, 128, 0, 129, 5000]),
    (125, 256, [255, 1, 1, 257, 100000]),
    (12, 5, [1] * 7 + [4, 5, 6, 4999]),
    (1, 31, [30, 1, 1, 31, 62, 1000, 7]),
    (512, 511, [510, 1, 1, 511, 20000]),
    (10, 12, [5, 1, 6, 77]),                                                   # (given unreduced)
])
def test_output_items_against_the_brute_force_count(L, M, chunks):
    """After N items every m with m M < N L exists, and a chunk emits what its items complete."""
    l, m = resampler.reduce(L, M)
    total, seen = 0, 0
    for c in chunks:
        total += c
        brute = 0
        while brute * m < total * l:
            brute += 1
        n = resampler.output_items(total, L, M)
        assert n == brute == -(-total * l // m) and n >= seen
        seen = n
    x = np.ones(sum(chunks), dtype=np.complex128)
    y, bound = resampler.resample(x, L, M, resampler.design(L, M))
    assert y.size == bound.size == seen


@pytest.mark.parametrize("L,M", RATIOS)
def test_a_tone_comes_out_at_its_new_frequency_after_the_delay(L, M):
    f_in = 0.3 * 0.5 * min(1.0, L / M)                                         # cycles per input item: 0.3 of the lower Nyquist
    n = 40 * 16 * max(L, M) // L + 4000
    x = np.exp(2j * np.pi * f_in * np.arange(n))
    y, _ = resampler.resample(x, L, M, resampler.design(L, M))
    assert y.size == resampler.output_items(n, L, M)
    d = resampler.delay(L, M, 16)
    assert d == 16 * max(L, M) / M
    m = np.arange(int(np.ceil(2 * d)) + 1, y.size)
    assert m.size > 1000
    want = np.exp(2j * np.pi * f_in * (M / L) * (m - d))
    err = float(np.abs(y[m] - want).max())
    print("resampler tone %d/%d: max error %.3g" % (L, M, err))
    assert err <= 1e-3


@pytest.mark.parametrize("up,down", [((12, 5), (5, 12)), ((128, 125), (125, 128))])
def test_a_frame_survives_the_round_trip(up, down):
    """synth.build_stream (SF7, CR 4, the three smoke payloads) up and down again by the model decodes on the oracle to the
    original frame tails, in both demodulators."""
    from oracle import oracle as O
    cfg = synth.TxConfig(sf=7, cr=4)
    payloads = [bytes.fromhex("deadbeef"), b"MI355X LoRa smoke", bytes(range(32))]
    st = synth.build_stream(payloads, cfg, rng=np.random.default_rng(7))
    x = np.concatenate([st.iq, np.zeros(2048, dtype=np.complex64)])
    hi, _ = resampler.resample(x, *up, resampler.design(*up))
    assert hi.size == resampler.output_items(x.size, *up)
    back, _ = resampler.resample(hi, *down, resampler.design(*down))
    assert back.size in (x.size, x.size + 1)
    want = [synth.expected_frame_tail(p, cfg) for p in payloads]
    for demod in (O.DEMOD_GRAD, O.DEMOD_FFT_COMPAT):
        got = O.decode_stream(back.astype(np.complex64), demod=demod, sf=7, cr=4)
        assert [g[15:] for g in got] == want, (demod, [g.hex() for g in got])


def test_ratio_helper():
    assert resampler.ratio(2.4e6, 2e6) == (5, 6)
    assert resampler.ratio(2.048e6, 1e6) == (125, 256)
    assert resampler.ratio(2.048e6, 2e6) == (125, 128) and resampler.ratio(2.56e6, 2e6) == (25, 32)
    assert resampler.ratio(1.92e6, 2e6) == (25, 24) and resampler.ratio(2.4e6, 1e6) == (5, 12)
    assert resampler.ratio(1e6, 1e6) == (1, 1) and resampler.ratio(1e6, 3e6) == (3, 1)
    with pytest.raises(ValueError):
        resampler.ratio(2.4e6, 2.000001e6)
    with pytest.raises(ValueError):
        resampler.ratio(1e6, 1e6 * np.pi)
    with pytest.raises(ValueError):
        resampler.ratio(1e6, 600e6)                                            # 600 / 1: outside the limits
    with pytest.raises(ValueError):
        resampler.ratio(0.0, 1e6)


def test_the_limits_of_the_design():
    for bad in (dict(L=0, M=1), dict(L=513, M=1), dict(L=1, M=513), dict(L=1, M=2, zero_crossings=1), dict(L=1, M=2, zero_crossings=33),
                dict(L=1, M=2, beta=-1.0), dict(L=1, M=2, beta=float("nan")), dict(L=1, M=2, cutoff=0.0), dict(L=1, M=2, cutoff=1.5),
                dict(L=1, M=40), dict(L=511, M=512, zero_crossings=32)):
        with pytest.raises(ValueError):
            resampler.design(**bad)
    assert resampler.taps_per_output(1, 31) == 993 and resampler.taps_per_output(512, 511) == 33
    assert np.array_equal(resampler.design(10, 12), resampler.design(5, 6))    # (given in any terms)
