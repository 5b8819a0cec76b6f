"""The exact-phase statement of include/lora_hip_tx.h, for windows anywhere in a capture, and the documented noise generator.

synth.build_wideband makes every frame's whole complex64 waveform; this evaluates the same definition per sample on the window
asked for (memory scales with the window, never with a frame's length), with the chirp's turn taken in integers before its one
division, so it is the reference where lora_tx.hip claims exactness: symbols of 2^22 items, positions beyond 2^34.

    exact_capture(frames, samp_rate, n0, n)   complex128[n]: the capture on absolute indices n0 .. n0 + n - 1
    active_amplitude(frames, samp_rate, n0, n) float64[n]: sum of |a_e| over the emitters active at each sample
    frame_items / frame_symbol_starts         a frame's length and where each of its symbols starts, in items
    philox4x32_10(counter4, key2)             Philox-4x32-10 (Random123) on Python ints or numpy uint64 arrays
    noise_reference(seed, sigma, m)           the noise of lora_tx.hip at absolute indices m, float64
"""
from dataclasses import replace

import numpy as np

from gr_lora_amd import synth


def _plan(frame, samp_rate):
    """(D, sps, kind[k], shift[k], first item of symbol k ... and the frame's end [k + 1]) of one synth.WidebandFrame."""
    D = synth.wideband_decimation(frame.cfg, samp_rate)
    cfg = replace(frame.cfg, samp_rate=float(samp_rate))
    sps = D << cfg.sf
    assert cfg.sps == sps
    plan = synth.frame_shift_plan(*synth.encode_shifts(frame.payload, cfg, frame.crc_bytes), cfg)
    kind = np.array([p[0] for p in plan], dtype=np.int64)
    shift = np.array([p[1] for p in plan], dtype=np.int64)
    bounds = np.concatenate(([0], np.cumsum(np.array([p[2] for p in plan], dtype=np.int64))))
    return D, sps, kind, shift, bounds


def frame_items(frame, samp_rate) -> int:
    return int(_plan(frame, samp_rate)[4][-1])


def frame_symbol_starts(frame, samp_rate):
    """int64[symbols + 1]: frame position of each symbol's first item (preamble, sync0, sync1, two downchirps, the quarter
    downchirp, header and payload symbols), then the frame's length."""
    return _plan(frame, samp_rate)[4]


def frame_shifts(frame, samp_rate):
    """int64[symbols]: the shift of each symbol of frame_symbol_starts (0 for preamble and downchirps)."""
    return _plan(frame, samp_rate)[3]


def _window(frame, bounds, n0, n):
    lo, hi = max(int(frame.start), int(n0)), min(int(frame.start) + int(bounds[-1]), int(n0) + int(n))
    return lo, hi


def oscillator_turn(freq_hz, samp_rate, m):
    """frac(x), x = (freq_hz / samp_rate) * float64(m): one rounded division, then one rounded multiply (the definition's)."""
    x = (float(freq_hz) / float(samp_rate)) * np.asarray(m).astype(np.float64)
    return x - np.floor(x)


def exact_capture(frames, samp_rate, n0, n):
    n0, n = int(n0), int(n)
    y = np.zeros(n, dtype=np.complex128)
    for fr in frames:
        D, sps, kind, shift, bounds = _plan(fr, samp_rate)
        lo, hi = _window(fr, bounds, n0, n)
        if lo >= hi:
            continue
        m = np.arange(lo, hi, dtype=np.int64)
        p = m - int(fr.start)
        k = np.searchsorted(bounds, p, side="right") - 1
        r = p - bounds[k]
        i = (r + shift[k] * D) % sps
        den = 2 * D * sps
        tc = ((i * (i - sps)) % den).astype(np.float64) / float(den)     # |i (i - sps)| <= 2^42: exact in int64
        tc = np.where(kind[k] == 1, -tc, tc)
        t = oscillator_turn(fr.freq_hz, samp_rate, m) + tc
        t -= np.rint(t)
        y[lo - n0:hi - n0] += float(fr.amplitude) * np.exp(2j * np.pi * t)
    return y


def active_amplitude(frames, samp_rate, n0, n):
    n0, n = int(n0), int(n)
    amp = np.zeros(n, dtype=np.float64)
    for fr in frames:
        lo, hi = _window(fr, _plan(fr, samp_rate)[4], n0, n)
        if lo < hi:
            amp[lo - n0:hi - n0] += abs(float(fr.amplitude))
    return amp


# ---- the noise ---------------------------------------------------------------------------------------------------------

_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox4x32_10(counter4, key2):
    """Philox-4x32-10 of Random123 (Salmon et al., SC'11): four 32-bit counter words, two key words -> four output words.
    Python ints, or numpy uint64 arrays holding 32-bit values (every product stays below 2^64)."""
    c0, c1, c2, c3 = counter4
    k0, k1 = key2
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _MASK, (p0 >> 32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def noise_words(seed, m):
    """(w0, w1) as uint64 arrays: the first two words of philox4x32_10((m & 0xffffffff, m >> 32, 0, 0), (seed lo, seed hi))."""
    m = np.asarray(m).astype(np.uint64)
    z = np.zeros_like(m)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = z + np.uint64(seed & _MASK), z + np.uint64(seed >> 32)
    w = philox4x32_10((m & np.uint64(_MASK), m >> np.uint64(32), z, z), (k0, k1))
    return w[0], w[1]


def noise_reference(seed, sigma, m):
    """-> (noise complex128[len(m)], rad float64, u float32): Box-Muller on w0, w1 as lora_tx.hip documents it.
    u = fl32(fl32(w0) 2^-32 + 2^-33), capped at 1; rad = fl32(sigma / sqrt 2) sqrt(-2 ln u); angle fl32(w1) 2^-31 half-turns."""
    w0, w1 = noise_words(seed, m)
    u = (w0.astype(np.float32).astype(np.float64) * 2.0 ** -32 + 2.0 ** -33).astype(np.float32)
    u = np.minimum(u, np.float32(1.0))
    rad = float(np.float32(float(sigma) / np.sqrt(2.0))) * np.sqrt(-2.0 * np.log(u.astype(np.float64)))
    ang = np.pi * (w1.astype(np.float32).astype(np.float64) * 2.0 ** -31)
    return rad * (np.cos(ang) + 1j * np.sin(ang)), rad, u
