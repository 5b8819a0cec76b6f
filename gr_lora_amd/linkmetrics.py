"""Per-frame link metrics: the float64 definition (include/lora_hip_link.h).

RSSI, SNR, carrier frequency offset, timing offset and sync word of a frame, measured on six one-symbol windows in front
of its header: the last two preamble upchirps, the two sync-word symbols, the two whole SFD downchirps.  Numpy only, no
torch and no device: this is what the window kernel (gr_lora_amd/csrc/lora_link.hip) and lora_hip_link_combine are held to.

Positions are relative to the frame's header_pos (first header symbol); sps = samples per symbol, N = 2^sf, D = sps / N.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

WINDOWS = 6
LOBE = 3                      # the lobe is peak_bin - 3 .. peak_bin + 3 (mod N): the Hann main lobe and one bin either side
FLAG_PREAMBLE, FLAG_SYNC, FLAG_SFD = 1, 2, 4
FLOOR_DB = -200.0
HANN_POWER_GAIN = 0.375       # mean of w^2
DOWN_POWER = 2.0              # |d_downchirp|^2: the decoder's table carries the reference's factor (1 + 1j)
_QUARTERS = (25, 17, 9)       # the pairs start 25/4, 17/4 and 9/4 symbols before the header


def downchirp(sf: int, bandwidth: int = 125000, samp_rate: float = 1e6) -> np.ndarray:
    """d_downchirp as the decoder builds it (table 0 of lora_hip_get_table), up to the last bit of its float32 cos / sin."""
    sps_rate = np.uint32(samp_rate)
    dt = np.float64(np.float32(1.0) / np.float32(sps_rate))
    sym_rate = float(bandwidth) / float(1 << sf)
    sps = int(np.uint32(np.float64(sps_rate) / sym_rate))
    t = dt * np.arange(sps, dtype=np.float64)
    ph = (2.0 * np.pi * t * (bandwidth / 2.0 - 0.5 * bandwidth * sym_rate * t)).astype(np.float32).astype(np.float64)
    return ((1.0 + 1.0j) * np.exp(1j * ph)).astype(np.complex64)


def hann(sps: int) -> np.ndarray:
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(sps, dtype=np.float64) + 0.5) / sps)


def window_starts(header_pos: int, sps: int) -> List[int]:
    """Start of the six windows, relative to the stream."""
    return [int(header_pos) - (q * sps) // 4 + k * sps for q in _QUARTERS for k in (0, 1)]


def window_valid(start: int, sps: int, stream_len: int) -> bool:
    return start >= 0 and start + sps <= stream_len


@dataclass
class WindowRecord:
    peak_bin: int = 0
    frac: float = 0.0
    lobe_power: float = 0.0
    total_power: float = 0.0
    peak_power: float = 0.0
    valid: int = 0
    power: Optional[np.ndarray] = None    # |X|^2 of the N bins (index k mod N); not part of the device's record


def window_spectrum(x: np.ndarray, down: np.ndarray, nbins: int, conj: bool) -> np.ndarray:
    """X[k], k in [-N/2, N/2) stored at index k mod N: the pruned sps-point DFT of v * down * hann."""
    sps = len(down)
    v = np.asarray(x, dtype=np.complex128)
    m = (np.conj(v) if conj else v) * down.astype(np.complex128) * hann(sps)
    F = np.fft.fft(m)
    return np.concatenate([F[:nbins // 2], F[sps - nbins // 2:]])


def window_record(x: np.ndarray, down: np.ndarray, nbins: int, conj: bool) -> WindowRecord:
    N = nbins
    pw = np.abs(window_spectrum(x, down, N, conj)) ** 2
    pk = int(np.argmax(pw))   # first maximum
    lobe = float(sum(pw[(pk + o) % N] for o in range(-LOBE, LOBE + 1)))
    a, b, c = np.sqrt(pw[(pk - 1) % N]), np.sqrt(pw[(pk + 1) % N]), np.sqrt(pw[pk])
    frac = 0.0
    if c > 0.0:
        alpha = max(a, b) / c
        d = (2.0 * alpha - 1.0) / (alpha + 1.0)
        frac = d if b >= a else -d
    return WindowRecord(pk, float(frac), lobe, float(pw.sum()), float(pw[pk]), 1, pw)


@dataclass
class Metrics:
    flags: int = 0
    signal_power: float = 0.0
    noise_power: float = 0.0
    rssi_dbfs: float = FLOOR_DB
    snr_db: float = FLOOR_DB
    cfo_bins: float = 0.0
    cfo_hz: float = 0.0
    timing_samples: float = 0.0
    sync_shift: List[int] = field(default_factory=lambda: [0, 0])
    windows: List[WindowRecord] = field(default_factory=list)


def _wrap(v: float, N: int) -> float:
    v = np.fmod(v + 0.5 * N, N)
    if v < 0.0:
        v += N
    return float(v - 0.5 * N)


def combine(windows: Sequence[WindowRecord], sps: int, nbins: int, bandwidth: float) -> Metrics:
    """The per-frame combination of six window records (lora_hip_link_combine)."""
    N, D = nbins, sps / nbins
    norm = HANN_POWER_GAIN * DOWN_POWER * float(sps) * float(sps)
    out = Metrics(windows=list(windows))
    pair, pos, mid = [False] * 3, [0.0] * 6, [0.0] * 3
    for p in range(3):
        pair[p] = bool(windows[2 * p].valid) and bool(windows[2 * p + 1].valid)
        if not pair[p]:
            continue
        out.flags |= 1 << p
        for k in (0, 1):
            w = windows[2 * p + k]
            pos[2 * p + k] = _wrap(float(w.peak_bin) + float(w.frac), N)
        mid[p] = _wrap(pos[2 * p] + 0.5 * _wrap(pos[2 * p + 1] - pos[2 * p], N), N)   # the mean, safe either side of the wrap
    s_sum, nb_sum, cnt = 0.0, 0.0, 0
    for p in (0, 2):
        if not pair[p]:
            continue
        for k in (0, 1):
            w = windows[2 * p + k]
            nb = max((float(w.total_power) - float(w.lobe_power)) / (N - 7.0), 0.0)
            s_sum += max(float(w.lobe_power) - 7.0 * nb, 0.0)
            nb_sum += nb
            cnt += 1
    if cnt:
        out.signal_power = s_sum / cnt / norm
        out.noise_power = nb_sum * N / cnt / norm
        if out.signal_power > 0.0:
            out.rssi_dbfs = max(10.0 * np.log10(out.signal_power), FLOOR_DB)
            out.snr_db = min(max(10.0 * np.log10(out.signal_power / out.noise_power), FLOOR_DB), -FLOOR_DB) if out.noise_power > 0.0 else -FLOOR_DB
    if pair[0] and pair[2]:
        half = 0.5 * _wrap(mid[0] - mid[2], N)
        out.cfo_bins = _wrap(half, N)
        out.cfo_hz = out.cfo_bins * bandwidth / N
        out.timing_samples = _wrap(mid[2] + half, N) * D
    if pair[0] and pair[1]:
        out.sync_shift = [int(np.floor(_wrap(pos[2 + k] - mid[0], N) + 0.5)) % N for k in (0, 1)]
    return out


def measure(stream: np.ndarray, header_pos: int, down: np.ndarray, nbins: int, bandwidth: float) -> Metrics:
    """The metrics of the frame whose first header symbol is stream[header_pos]; windows outside the stream are not read."""
    sps = len(down)
    recs = []
    for i, s in enumerate(window_starts(header_pos, sps)):
        if window_valid(s, sps, len(stream)):
            recs.append(window_record(stream[s:s + sps], down, nbins, conj=i >= 4))
        else:
            recs.append(WindowRecord())
    return combine(recs, sps, nbins, bandwidth)
