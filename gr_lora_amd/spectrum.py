"""The spectral scan's definition in float64 (include/lora_hip_spectrum.h): Welch power-spectrum rows and band powers.

    window   w[k] = float32(0.5 - 0.5 cos(2 pi k / nfft)) (periodic Hann) or ones;  norm = 1 / (nfft * sum w[k]^2)
    segment  s covers x[s hop .. s hop + nfft - 1];   P_s[k] = |sum_n w[n] x[s hop + n] e^{-2 pi j k n / nfft}|^2
    row      r covers segments r n_avg .. (r + 1) n_avg - 1:   psd[r][i] = norm / n_avg * sum_s P_s[k],  peak[r][i] = norm * max_s P_s[k]
             stored centred, i = (k + nfft / 2) mod nfft: index i is frequency (i - nfft / 2) fs / nfft
    band     (first_bin, n_bins) in centred indices:  band[r][b] = sum of psd[r][i] over the band

welch_rows works on the whole stream at once (no chunks, no state): it is what the device handle is held to, whatever the
chunking.  Units are full-scale^2 per bin: by Parseval a row sums to the windowed mean power of its samples.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

HANN, RECT = 0, 1
WINDOWS = {"hann": HANN, "rect": RECT}
MIN_NFFT, MAX_NFFT, MAX_AVG, MAX_BANDS = 64, 4096, 1024, 256


def window_id(window) -> int:
    if isinstance(window, str):
        if window.lower() not in WINDOWS:
            raise ValueError("unknown window %r (hann, rect)" % (window,))
        return WINDOWS[window.lower()]
    if int(window) not in (HANN, RECT):
        raise ValueError("unknown window %r (hann, rect)" % (window,))
    return int(window)


def window_table(nfft: int, window="hann") -> np.ndarray:
    """The float32 table the handle hands out (lora_hip_spectrum_window): formed in double, rounded once."""
    if window_id(window) == RECT:
        return np.ones(int(nfft), dtype=np.float32)
    k = np.arange(int(nfft), dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * k / float(nfft))).astype(np.float32)


def check_params(nfft: int, hop: int, n_avg: int):
    nfft, hop, n_avg = int(nfft), int(hop), int(n_avg)
    if nfft < MIN_NFFT or nfft > MAX_NFFT or nfft & (nfft - 1):
        raise ValueError("nfft %d must be a power of two in %d..%d" % (nfft, MIN_NFFT, MAX_NFFT))
    if not 1 <= hop <= nfft:
        raise ValueError("hop %d must be in 1..nfft" % hop)
    if not 1 <= n_avg <= MAX_AVG:
        raise ValueError("n_avg %d must be in 1..%d" % (n_avg, MAX_AVG))
    return nfft, hop, n_avg


def output_rows(n_items: int, nfft: int, hop: int, n_avg: int) -> int:
    """Rows whose last sample is among the first n_items of the stream."""
    segs = (int(n_items) - nfft) // hop + 1 if n_items >= nfft else 0
    return segs // n_avg


def freqs(samp_rate: float, nfft: int) -> np.ndarray:
    """Frequency (Hz from the capture's centre) of every centred index."""
    return (np.arange(int(nfft), dtype=np.float64) - nfft // 2) * float(samp_rate) / int(nfft)


def welch_rows(x, nfft: int, hop: int, n_avg: int, window="hann", bands: Optional[Sequence[Tuple[int, int]]] = None, w: Optional[np.ndarray] = None):
    """(psd[rows, nfft], peak[rows, nfft], band[rows, len(bands)] or None, first_sample[rows]) in float64.
    x: the stream as complex (already converted: iqformat.to_cf32 for integer items).  w: the window's float32 values (as
    handed out by the handle); None: window_table(nfft, window)."""
    nfft, hop, n_avg = check_params(nfft, hop, n_avg)
    x = np.asarray(x).astype(np.complex128).reshape(-1)
    wt = (window_table(nfft, window) if w is None else np.asarray(w, dtype=np.float32)).astype(np.float64)
    if wt.shape != (nfft,):
        raise ValueError("the window table must hold nfft values")
    norm = 1.0 / (nfft * float(np.sum(wt * wt)))
    rows = output_rows(x.size, nfft, hop, n_avg)
    psd = np.zeros((rows, nfft), dtype=np.float64)
    peak = np.zeros((rows, nfft), dtype=np.float64)
    for r in range(rows):
        starts = (r * n_avg + np.arange(n_avg)) * hop
        seg = x[starts[:, None] + np.arange(nfft)[None, :]] * wt[None, :]
        p = np.abs(np.fft.fft(seg, axis=1)) ** 2
        psd[r] = np.fft.fftshift(p.sum(axis=0)) * (norm / n_avg)
        peak[r] = np.fft.fftshift(p.max(axis=0)) * norm
    band = None
    if bands is not None and len(bands):
        band = np.zeros((rows, len(bands)), dtype=np.float64)
        for b, (first, n) in enumerate(bands):
            if n < 1 or first < 0 or first + n > nfft:
                raise ValueError("band %d = (%d, %d) is empty or outside [0, nfft)" % (b, first, n))
            band[:, b] = psd[:, first:first + n].sum(axis=1)
    first_sample = np.arange(rows, dtype=np.int64) * (n_avg * hop)
    return psd, peak, band, first_sample


def band_bins(samp_rate: float, nfft: int, f_lo: float, f_hi: float) -> Tuple[int, int]:
    """(first_bin, n_bins): the centred indices whose centre frequency lies in [f_lo, f_hi), clipped to the capture."""
    nfft = int(nfft)
    df = float(samp_rate) / nfft
    lo = int(np.ceil(float(f_lo) / df - 1e-9)) + nfft // 2       # (the tolerance keeps an edge that is a bin centre up to rounding on its side)
    hi = int(np.ceil(float(f_hi) / df - 1e-9)) + nfft // 2
    lo, hi = max(lo, 0), min(hi, nfft)
    if hi <= lo:
        raise ValueError("no bin centre of a %d-point spectrum at %g Hz lies in [%g, %g) Hz" % (nfft, samp_rate, f_lo, f_hi))
    return lo, hi - lo


def grid_bands(samp_rate: float, nfft: int, grid_offset: float, n_grid: int, channels: Sequence[int], bandwidth: float) -> List[Tuple[int, int]]:
    """One band per filter-bank channel: f = grid_offset + channels[c] * samp_rate / n_grid, [f - bandwidth / 2, f + bandwidth / 2)."""
    out = []
    for k in channels:
        f = float(grid_offset) + int(k) * float(samp_rate) / int(n_grid)
        out.append(band_bins(samp_rate, nfft, f - bandwidth / 2.0, f + bandwidth / 2.0))
    return out


def to_dbfs(p, floor_db: float = -200.0) -> np.ndarray:
    """10 log10(p) with p in full-scale^2: 0 dBFS is a unit-amplitude complex tone.  Zero power reads floor_db."""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.maximum(10.0 * np.log10(np.maximum(p, 0.0)), floor_db)
