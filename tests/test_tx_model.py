"""CPU: synth.build_wideband, the float64 definition of the traffic synthesiser's capture, against the construction the gateway
benchmark has used so far (per-channel build_stream, mixed on the absolute sample index, summed)."""
import numpy as np
import pytest

FS, M, F0 = 2e6, 10, 100e3          # workload (a)'s grid: channels 200 kHz apart, offset 100 kHz


@pytest.fixture(scope="module")
def capture():
    from gr_lora_amd import synth
    rng = np.random.default_rng(11)
    frames, wide = [], None
    per = []
    for k, sf, lead in ((-4, 7, 3000), (3, 8, 1234)):
        pl = bytes(rng.integers(0, 256, 9, dtype=np.uint8))
        cfg = synth.TxConfig(sf=sf, cr=4, samp_rate=FS, hdr_nibbles=synth.valid_hdr_nibbles(len(pl), 4, True))
        crc = synth.valid_crc_bytes(pl)
        st = synth.build_stream([pl, pl[::-1]], cfg, gaps=[lead, 5000], tail_symbols=2.0, crc_bytes=crc)
        per.append((k, st.iq))
        for p, start in zip((pl, pl[::-1]), st.frame_starts):
            frames.append(synth.WidebandFrame(p, cfg, start, F0 + k * FS / M, 1.0, crc))
    n = max(s.size for _, s in per) + 4096
    wide = np.zeros(n, dtype=np.complex128)
    for k, s in per:                                        # tools/bench_gateway.py synthesise
        ph = (F0 + k * FS / M) / FS * np.arange(s.size, dtype=np.float64)
        wide[: s.size] += s * np.exp(2j * np.pi * (ph - np.floor(ph)))
    return frames, wide


def test_equals_the_per_channel_construction(capture):
    from gr_lora_amd import synth
    frames, wide = capture
    y = synth.build_wideband(frames, FS, 0, wide.size)
    assert y.dtype == np.complex128 and y.shape == wide.shape
    assert np.abs(y - wide).max() <= 1e-12
    assert np.abs(wide).max() > 1.5                         # the two channels do overlap in time


def test_gaps_are_exactly_zero(capture):
    from gr_lora_amd import synth
    frames, wide = capture
    y = synth.build_wideband(frames, FS, 0, wide.size)
    active = np.zeros(wide.size, dtype=bool)
    for f in frames:
        active[f.start:f.start + synth.wideband_waveform(f, FS).size] = True
    assert (~active).sum() > 4096 and active.sum() > 0
    assert np.all(np.abs(y[active]) > 0)
    assert np.array_equal(y[~active].view(np.float64), np.zeros(2 * int((~active).sum())))


@pytest.mark.parametrize("n0,n", [(0, 1), (2999, 3), (3000, 4097), (12345, 70001), (10 ** 6, 100)])
def test_any_window_is_the_slice_of_the_whole(capture, n0, n):
    from gr_lora_amd import synth
    frames, wide = capture
    whole = synth.build_wideband(frames, FS, 0, max(wide.size, n0 + n))
    assert np.array_equal(synth.build_wideband(frames, FS, n0, n), whole[n0:n0 + n])


def test_amplitude_order_and_decimations_that_are_no_power_of_two():
    from gr_lora_amd import synth
    cfg = synth.TxConfig(sf=7, cr=1, bw=125000)
    a = synth.WidebandFrame(b"one", cfg, 10, 1234.5, 0.3)
    b = synth.WidebandFrame(b"two", cfg, 500, -50e3, 0.7)
    y = synth.build_wideband([a, b], 375e3, 0, 20000)
    ya = synth.build_wideband([a], 375e3, 0, 20000)
    yb = synth.build_wideband([b], 375e3, 0, 20000)
    assert np.array_equal(y, ya + yb)
    c = synth.wideband_waveform(a, 375e3)
    assert c.dtype == np.complex64 and c.size == (8 + 4 + 8) * 384 + 96 + len(synth.encode_shifts(b"one", cfg)[1]) * 384
    assert abs(abs(ya[10 + 777]) - 0.3) < 1e-7 and ya[9] == 0
    with pytest.raises(ValueError):
        synth.build_wideband([a], 1e6 + 1, 0, 10)
    with pytest.raises(ValueError):
        synth.build_wideband([synth.WidebandFrame(b"x", synth.TxConfig(sf=12), 0)], 125000.0 * 1025, 0, 10)


def test_existing_transmit_model_is_untouched():
    """The additions sit behind the functions the receiver's tests have always used: the golden capture still comes out."""
    import os
    from gr_lora_amd import synth
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sf7_cr4_deadbeef_x2.cf32")
    gold = np.fromfile(path, dtype=np.complex64)
    cfg = synth.TxConfig(sf=7, cr=4)
    fr = synth.modulate_frame(*synth.encode_shifts(bytes.fromhex("deadbeef"), cfg), cfg)
    w = synth.build_wideband([synth.WidebandFrame(bytes.fromhex("deadbeef"), cfg, 0)], 1e6, 0, fr.size)
    assert np.array_equal(w, fr.astype(np.complex128))
    assert np.array_equal(gold[3000:3000 + fr.size], fr)      # (tests/golden/make_golden.py: gaps 3000, 2500)
