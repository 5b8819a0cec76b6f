"""CPU: tests/tx_exact.py, the exact-phase reference tests/test_gpu_tx_space.py holds lora_tx.hip to - against synth.build_wideband
where that model can be built, against itself across windows, able to tell a rounded oscillator product from an unrounded one at
the far position, and its Philox against the Random123 known answers."""
from dataclasses import replace
from fractions import Fraction

import numpy as np
import pytest

import tx_exact
from gr_lora_amd import synth

FS = 375e3
N_ITEMS = 200000


def _payload(n, seed):
    return bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


# tests/test_gpu_tx.py's EMITTERS: (payload, sf, cr, bandwidth, start, freq_hz, amplitude, implicit, reduced_rate)
EMITTERS = [
    (_payload(17, 1), 7, 4, 125000, 0, 31000.0, 1.0, False, False),
    (_payload(17, 2), 6, 3, 93750, 4099, -100123.456789, 0.25, True, False),
    (_payload(8, 3), 9, 2, 125000, 7001, 50000.0, 0.5, False, True),
    (_payload(5, 4), 7, 1, 125000, 9003, -62500.0, 0.75, False, False),
    (_payload(9, 5), 7, 4, 125000, 120011, -125000.0 / 3.0, 0.5, False, False),
    (_payload(30, 6), 7, 2, 125000, 190003, 7.0, 1.0, False, False),
]


def _frames(emitters=EMITTERS):
    out = []
    for pl, sf, cr, bw, start, f, a, imp, rr in emitters:
        cfg = synth.TxConfig(sf=sf, cr=cr, bw=bw, implicit=imp, reduced_rate=rr, hdr_nibbles=synth.valid_hdr_nibbles(len(pl), cr, True))
        out.append(synth.WidebandFrame(pl, cfg, start, f, a, synth.valid_crc_bytes(pl)))
    return out


@pytest.fixture(scope="module")
def whole():
    frames = _frames()
    return frames, tx_exact.exact_capture(frames, FS, 0, N_ITEMS)


def test_exact_against_build_wideband(whole):
    """|exact - build_wideband| <= 1.0 * 2^-24 * (sum of the active amplitudes): the model rounds its unit phasor to complex64,
    2^-25 per component, 0.71 units of 2^-24 in magnitude; everything else on either side is float64.  Both exactly 0 where
    nothing is active.  Measured: 0.63 units at the worst sample."""
    frames, exact = whole
    model = synth.build_wideband(frames, FS, 0, N_ITEMS)
    amp = tx_exact.active_amplitude(frames, FS, 0, N_ITEMS)
    want = np.zeros(N_ITEMS)
    for f in frames:
        want[f.start:f.start + synth.wideband_waveform(f, FS).size] += f.amplitude
    assert np.array_equal(amp, want[:N_ITEMS])
    for f in frames:
        assert tx_exact.frame_items(f, FS) == synth.wideband_waveform(f, FS).size
    active = amp > 0
    err = np.abs(exact - model)
    print("exact against build_wideband: worst %.3f units of 2^-24 x active amplitude" % float((err[active] / amp[active]).max() * 2.0 ** 24))
    assert active.sum() > 90000 and (~active).sum() > 40000 and amp.max() > 2.0
    assert np.all(err <= 1.0 * 2.0 ** -24 * amp)
    assert not exact[~active].view(np.uint64).any() and not model[~active].view(np.uint64).any()


def test_windows_are_slices_bit_for_bit(whole):
    """A window that starts inside each part of a frame (preamble, sync symbols, downchirps, the quarter downchirp, header,
    payload, behind the end; emitter 2 is SF9 at decimation 3, symbols of 1536 items, starting at 7001) is the same slice of the
    whole capture, bit for bit, and so is one that starts before the capture's first frame or runs past its last."""
    frames, exact = whole
    s, sps = 7001, 1536
    starts = tx_exact.frame_symbol_starts(frames[2], FS)
    assert starts[1] == sps and starts[13] == 12 * sps + sps // 4 and starts[-1] == tx_exact.frame_items(frames[2], FS)
    n0s = [0, 1, s - 5, s, s + 3 * sps + 77, s + 8 * sps + 5, s + 9 * sps + 1000, s + 10 * sps + 3, s + 11 * sps + 1535, s + 12 * sps + 100,
           s + 12 * sps + sps // 4, s + 15 * sps, s + 22 * sps + 700, s + int(starts[-1]) - 10, 119000, 190003 + 17]
    for n0 in n0s:
        for n in (1, 2048, 5000):
            w = tx_exact.exact_capture(frames, FS, n0, n)
            ref = exact[n0:n0 + n]
            assert np.array_equal(w[:ref.size].view(np.uint64), ref.view(np.uint64)), (n0, n)
    # and before index 0 there is nothing
    w = tx_exact.exact_capture(frames, FS, -100, 300)
    assert not w[:100].view(np.uint64).any() and np.array_equal(w[100:].view(np.uint64), exact[:200].view(np.uint64))


def test_preamble_len_and_sync_shifts_reach_the_reference():
    """preamble_len and sync_shifts come through the frame's TxConfig: a longer preamble moves everything behind it, and the sync
    symbols are upchirps advanced by the given shifts."""
    pl = b"abc"
    base = dict(sf=7, cr=4, bw=125000, hdr_nibbles=synth.valid_hdr_nibbles(3, 4, True))
    a = synth.WidebandFrame(pl, synth.TxConfig(**base), 0, 0.0, 1.0, synth.valid_crc_bytes(pl))
    b = synth.WidebandFrame(pl, synth.TxConfig(preamble_len=3, sync_shifts=(127, 0), **base), 0, 0.0, 1.0, synth.valid_crc_bytes(pl))
    ya, yb = (tx_exact.exact_capture([f], 125e3, 0, tx_exact.frame_items(f, 125e3)) for f in (a, b))
    assert ya.size - yb.size == 5 * 128
    assert np.array_equal(ya[10 * 128:], yb[5 * 128:])                       # from the downchirps on
    up = ya[:128]
    assert np.array_equal(yb[3 * 128:4 * 128], np.roll(up, -127)) and np.array_equal(yb[4 * 128:5 * 128], up)
    assert np.array_equal(ya[8 * 128:9 * 128], np.roll(up, -24)) and np.array_equal(ya[9 * 128:10 * 128], np.roll(up, -32))
    assert np.allclose(ya[10 * 128:11 * 128], np.conj(up), atol=1e-12)
    assert np.abs(synth.build_wideband([b], 125e3, 0, yb.size) - yb).max() <= 2.0 ** -24


def test_far_position_separates_a_rounded_product():
    """At m = 2^34 + 12345 .. + 4000 with f = 0.49 fs the oscillator's turn as the definition rounds it (one division, one multiply,
    both to float64) differs from the unrounded product of the same rounded quotient by more than 32 * 2^-24 rad somewhere: a kernel
    that contracts the product into the subtraction, or reassociates it, cannot pass a 16-unit bound there.  At 2^33 and 2^32 it
    could (24 and 12 units), hence 2^34."""
    fs, f = 375e3, 0.49 * 375e3
    q = Fraction(f / fs)

    def worst(base):
        m = np.arange(base + 12345, base + 12345 + 4000, dtype=np.int64)
        got = tx_exact.oscillator_turn(f, fs, m)
        d = np.array([float((Fraction(float(g)) - (q * int(k)) % 1 + Fraction(1, 2)) % 1 - Fraction(1, 2)) for g, k in zip(got, m)])
        return float(np.abs(d).max() * 2 * np.pi * 2.0 ** 24)
    w34, w33, w32 = worst(1 << 34), worst(1 << 33), worst(1 << 32)
    print("rounded against unrounded oscillator turn: %.1f units of 2^-24 rad at 2^34, %.1f at 2^33, %.1f at 2^32" % (w34, w33, w32))
    assert w34 > 32.0
    assert w33 < 32.0 and w32 < 16.0
    # the capture carries it: one frame there, against the same with the unrounded turn
    pl = b"far"
    fr = synth.WidebandFrame(pl, synth.TxConfig(sf=7, cr=4, hdr_nibbles=synth.valid_hdr_nibbles(3, 4, True)), (1 << 34) + 12345, f, 1.0, synth.valid_crc_bytes(pl))
    y = tx_exact.exact_capture([fr], fs, fr.start, 4000)
    y0 = tx_exact.exact_capture([replace(fr, freq_hz=0.0)], fs, fr.start, 4000)
    m = np.arange(fr.start, fr.start + 4000)
    unrounded = y0 * np.exp(2j * np.pi * np.array([float((q * int(k)) % 1) for k in m]))
    assert np.abs(y - unrounded).max() > 32 * 2.0 ** -24


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32_10."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tx_exact.philox4x32_10(ctr, key) == want
    # the array form is the same function
    ctr = [np.array([k[0][i] for k in kat], dtype=np.uint64) for i in range(4)]
    key = [np.array([k[1][i] for k in kat], dtype=np.uint64) for i in range(2)]
    got = tx_exact.philox4x32_10(ctr, key)
    for i in range(4):
        assert got[i].dtype == np.uint64 and [int(v) for v in got[i]] == [k[2][i] for k in kat]


def test_noise_words_use_the_whole_index_and_seed():
    """counter = (m low, m high, 0, 0), key = (seed low, seed high): each half changes the words."""
    seed = 0x1234567800abcdef
    m = np.array([5, 5 + (1 << 32)], dtype=np.uint64)
    w0, w1 = tx_exact.noise_words(seed, m)
    assert (int(w0[0]), int(w1[0])) == tx_exact.philox4x32_10((5, 0, 0, 0), (0x00abcdef, 0x12345678))[:2]
    assert (int(w0[1]), int(w1[1])) == tx_exact.philox4x32_10((5, 1, 0, 0), (0x00abcdef, 0x12345678))[:2]
    assert int(w0[0]) != int(w0[1])
    assert int(tx_exact.noise_words(seed & 0xffffffff, m)[0][0]) != int(w0[0])
    g, rad, u = tx_exact.noise_reference(seed, 1.0, np.arange(1 << 16))
    assert u.dtype == np.float32 and u.min() > 0 and u.max() <= 1
    assert abs(np.mean(np.abs(g) ** 2) - 1.0) < 0.02
