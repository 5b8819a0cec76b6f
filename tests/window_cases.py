"""Window streams for the three copies of the pruned dechirp spectrum, shared by tests/test_window_cases_model.py (no GPU)
and tests/test_gpu_window_space.py.  Numpy only.

The operation: the N = 2^sf bins k in [-N/2, N/2), stored at index k mod N, of the sps-point DFT of x * d_downchirp (no N/2 fold).  Three
kernels compute it in a copy of the generic polyphase FFT; each is held to its committed float64 definition:

  kernel  "detect"  detect_windows_kernel  capi.Handle.window_stats_device            oracle/preamble_oracle.py: window_stats
          "link"    link_windows_kernel    capi.Handle.measure_link_device(windows)   gr_lora_amd/linkmetrics.py: window_record
          "soft"    soft_symbols_kernel    capi.Handle.soft_symbols_device            gr_lora_amd/softdecode.py: llr_window

A shape is (sf, D), D = sps / N the decimation, rate = 125e3 * D; build_tables accepts SF 6 .. 12 and D in {1, 2, 4, 8, 16}: 35 shapes.

The stream of a shape (build): complex64, seeded by [sf, D], windows back to back, the first at item 3 (so that windows start on odd items).
Every window is made from the decoder's own downchirp table so that what the kernel dechirps is the stated signal s: x[n] = s[n] conj(down[n]) / 2
(|down[n]|^2 = 2).  For the link kernel's windows 4 and 5 of each frame x is the conjugate of that: the kernel conjugates first.  The 13 windows:

   0      zeros
   1 - 6  on-bin tones s[n] = 0.5 exp(2 pi j k n / sps), k = 0, 1, -1, N/2 - 1, -N/2 and one seeded k: bin-index sign, the wrap of the link
          lobe across bin 0, the FFT demodulator's b = (k - 1) mod N and the reduced-rate word ((b + 2) >> 2) mod N/4 at its wrap
   7 - 8  off-bin tones at k + 0.37 and k - 0.21, k seeded: leakage into every bin, the link frac away from 0 and from +-0.5
   9 - 11 unit-variance complex Gaussian noise: every row, pass and twiddle contributes to every bin
  12      amplitude 0.5 on bin k + 0.1 (k seeded) in noise of variance 0.05

For the link entry the same list is laid out as frames of six contiguous windows (linkmetrics.window_starts: a frame's windows begin 25/4
symbols before header_pos), padded with noise windows to a multiple of six: 18 windows, 3 frames.

The unit every tolerance is stated in (unit):  U = 2^-24 log2(sps) sqrt(sps) ||m||_2,  m the sequence the kernel transforms (x down for detect
and soft, conj(x) down for the detect "up" half, v down hann for link): the norm-wise rounding bound of an sps-point fp32 FFT (Higham, Accuracy and
Stability of Numerical Algorithms, thm 24.2) without its constant.  For an on-bin tone sqrt(sps) ||m||_2 is the peak amplitude, so on tone windows
err / U is the relative error in units of log2(sps) roundings.

What may be set aside, decided by the definition alone (never by what a device returned), R being the limit in force:
  index   an arg-max index is compared unless the definition's two largest magnitudes differ by at most 2 R U
  frac    (link) compared under 6 R U / |X[peak]| where the index was compared and the definition's two neighbour magnitudes a, b differ by more than
          2 R U.  Where they do not, the sign of frac (b >= a) is within rounding of a coin toss; then |frac_dev - frac_model| <= 6 R U / |X[peak]| +
          2 |frac_model| still holds (a flipped sign moves frac by 2 |d|), and is asserted.  An on-bin tone under the Hann window is such a window by
          construction - a = b = |X[peak]| / 2 in exact arithmetic, alpha = 1/2, d = 0 - and that bound is as tight there as the plain one; the check
          counts as SET ASIDE only where 2 |frac_model| exceeds 6 R U / |X[peak]|, i.e. where the allowance for the sign is the larger part.
  An index that is not compared for equality is still held (near_max): the bin the device names must be one whose magnitude in the definition is
  within 2 R U of the largest.
Over the whole sweep at most 1 comparison in 10 per kernel may be set aside, and none on a tone window's tone.  For the detect kernel that is the
"down" half.  The "up" half of a tone window transforms conj(s) down^2 / 2, a chirp of twice the rate: its spectrum is FLAT (at SF6, D = 1 the three
largest of 64 magnitudes are 5.656861, 5.656862, 5.656865), the arg-max of the definition is decided in the seventh digit on 188 of the sweep's 210
on-bin "up" halves at R = 16, and no stream can put a tone in both halves of one window.  Those 315 "up" indices stay out of the census and are
held by near_max; their peak and total are compared like every other.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from types import SimpleNamespace
from typing import List, Optional

import numpy as np

from gr_lora_amd import linkmetrics as LM, softdecode as SD
from oracle import preamble_oracle as PO

BW = 125000
SFS = (6, 7, 8, 9, 10, 11, 12)
DECIMS = (1, 2, 4, 8, 16)
SHAPES = [(sf, d) for sf in SFS for d in DECIMS]
KERNELS = ("detect", "link", "soft")
FIRST = 3                       # the first window starts here: windows start on odd items
CAP_R = 16.0                    # the cap of DESIGN.md 4.20; no limit may be above it

# LIMIT_R[kernel] = 4 x the largest err / U of the first whole sweep on an MI355X (all 35 shapes, all quantities; DESIGN.md 4.20 and the
# docstring of tests/test_gpu_window_space.py hold the per-shape figures), never above CAP_R.  The factor is for nothing but another seed.
# All three maxima are ONE unit in the last place of an on-bin tone's peak at SF6, D = 1 (sps = 64; peak 32: 2^-18 / U = 0.3464; under the Hann
# window peak 16: 2^-19 / U = 0.2796): the limits are four such units there and, U growing with log2(sps), eleven at SF12, D = 16.
MEASURED_R = {"detect": 0.3464, "link": 0.2796, "soft": 0.3464}
LIMIT_R = {k: min(4.0 * v, CAP_R) for k, v in MEASURED_R.items()}     # detect 1.386, link 1.118, soft 1.386

KINDS = ("zeros", "on-bin", "on-bin", "on-bin", "on-bin", "on-bin", "on-bin", "off-bin", "off-bin", "noise", "noise", "noise", "tone in noise")
N_WINDOWS = len(KINDS)          # 13
TONE_KINDS = ("on-bin", "off-bin", "tone in noise")


def rate(decim: int) -> float:
    return 125e3 * decim


def structure(sf: int, decim: int) -> dict:
    """How build_tables (lora_runtime.cpp) and soft_stride (lora_soft.inc.hip) lay the transform out at this shape."""
    N, budget = 1 << sf, 64 * 1024 + 64
    G = 1
    while (decim // G) * (N + 1) * 8 > budget and G < decim:
        G <<= 1
    rows = decim // G
    return dict(rows=rows, passes=G, stride=N + 1 if rows > 1 else N, soft_stride=N + (16 // rows if rows >= 2 else 0),
                bins_per_thread=max(N // 256, 1), idle_waves=max(4 - N // 64, 0), odd_log=bool(sf & 1))


@dataclass
class Stream:
    sf: int
    decim: int
    sps: int
    nbins: int
    iq: np.ndarray                 # complex64
    starts: List[int]
    kinds: List[str]
    tone_k: List[Optional[int]]    # the k of an on-bin tone, else None
    link: bool

    def window(self, i: int) -> np.ndarray:
        return self.iq[self.starts[i]:self.starts[i] + self.sps]

    def conj(self, i: int) -> bool:
        return self.link and i % 6 >= 4

    def header_pos(self, frame: int) -> int:
        return self.starts[6 * frame] + (25 * self.sps) // 4


def _noise(rng, n, var=1.0):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(var / 2.0)


def build(sf: int, decim: int, down: np.ndarray, link: bool = False) -> Stream:
    """The stream of shape (sf, decim) from the decoder's downchirp table (complex64, sps items)."""
    N, sps = 1 << sf, decim << sf
    down = np.asarray(down).view(np.complex64) if np.asarray(down).dtype != np.complex64 else np.asarray(down)
    assert down.size == sps
    rng = np.random.default_rng([sf, decim])
    k_on, k_off, k_tn = (int(v) for v in rng.integers(-N // 2 + 2, N // 2 - 2, 3))
    n = np.arange(sps, dtype=np.float64)
    tone = lambda f: 0.5 * np.exp(2j * np.pi * f * n / sps)
    on = [0, 1, -1, N // 2 - 1, -N // 2, k_on]
    s = [np.zeros(sps, dtype=np.complex128)] + [tone(k) for k in on] + [tone(k_off + 0.37), tone(k_off - 0.21)]
    s += [_noise(rng, sps) for _ in range(3)]
    s.append(tone(k_tn + 0.1) + _noise(rng, sps, 0.05))
    kinds, tone_k = list(KINDS), [None] + on + [None] * 6
    if link:
        while len(s) % 6:
            s.append(_noise(rng, sps))
            kinds.append("noise")
            tone_k.append(None)
    cd = np.conj(down.astype(np.complex128)) / 2.0
    iq = np.zeros(FIRST + len(s) * sps + 2, dtype=np.complex128)
    iq[:FIRST] = _noise(rng, FIRST)
    iq[-2:] = _noise(rng, 2)
    starts = []
    for i, si in enumerate(s):
        x = si * cd
        starts.append(FIRST + i * sps)
        iq[starts[-1]:starts[-1] + sps] = np.conj(x) if (link and i % 6 >= 4) else x
    return Stream(sf, decim, sps, N, iq.astype(np.complex64), starts, kinds, tone_k, link)


def unit(m: np.ndarray) -> float:
    """U of the sequence m the kernel transforms."""
    m = np.asarray(m, dtype=np.complex128)
    return float(2.0 ** -24 * np.log2(m.size) * np.sqrt(m.size) * np.sqrt((m.real ** 2 + m.imag ** 2).sum()))


def unit_plain(x, down, conj=False):
    v = np.asarray(x, dtype=np.complex128)
    return unit((np.conj(v) if conj else v) * down.astype(np.complex128))


def unit_link(x, down, conj):
    v = np.asarray(x, dtype=np.complex128)
    return unit((np.conj(v) if conj else v) * down.astype(np.complex128) * LM.hann(down.size))


def _top_two_gap(mag: np.ndarray) -> float:
    top = np.partition(mag, -2)[-2:]
    return float(top[1] - top[0])


def cfg_of(sf: int):
    return SimpleNamespace(sf=sf, nbins=1 << sf)


@dataclass
class DetectModel:
    rec: tuple          # preamble_oracle.window_stats
    U: tuple            # (down half, up half)
    gap: tuple          # top-two gap of the magnitudes, both halves
    mag: tuple          # the magnitudes, both halves


@dataclass
class LinkModel:
    rec: LM.WindowRecord
    U: float
    gap: float
    nb_gap: float       # | |X[peak - 1]| - |X[peak + 1]| |
    peak: float         # |X[peak]|
    mag: np.ndarray


@dataclass
class SoftModel:
    L: np.ndarray
    k: int
    peak: float
    U: float
    gap: float
    reduced: bool
    mag: np.ndarray


def detect_model(iq: np.ndarray, pos: int, down: np.ndarray, nbins: int) -> DetectModel:
    x = iq[pos:pos + down.size]
    cfg = cfg_of(nbins.bit_length() - 1)
    md, mu = SD.magnitudes(x, 0, cfg, down), SD.magnitudes(np.conj(x), 0, cfg, down)   # (the same spectrum: tests/test_window_cases_model.py)
    return DetectModel(PO.window_stats(iq, pos, down, nbins), (unit_plain(x, down), unit_plain(x, down, True)), (_top_two_gap(md), _top_two_gap(mu)), (md, mu))


def link_model(x: np.ndarray, down: np.ndarray, nbins: int, conj: bool) -> LinkModel:
    rec = LM.window_record(x, down, nbins, conj)
    mag = np.sqrt(rec.power)
    pk = rec.peak_bin
    return LinkModel(rec, unit_link(x, down, conj), _top_two_gap(mag), float(abs(mag[(pk - 1) % nbins] - mag[(pk + 1) % nbins])), float(mag[pk]), mag)


def soft_model(iq: np.ndarray, pos: int, down: np.ndarray, nbins: int, reduced: bool) -> SoftModel:
    cfg = cfg_of(nbins.bit_length() - 1)
    L, k, peak, _tot, second = SD.llr_window(iq, pos, cfg, reduced, down)
    return SoftModel(L, k, peak, unit_plain(iq[pos:pos + down.size], down), peak - second, reduced, SD.magnitudes(iq, pos, cfg, down))


def index_compared(gap: float, U: float, R: float) -> bool:
    return gap > 2.0 * R * U


def near_max(mag: np.ndarray, idx: int, U: float, R: float) -> bool:
    """the bin idx is one whose magnitude in the definition is within 2 R U of the largest"""
    return 0 <= idx < mag.size and mag[idx] >= mag.max() - 2.0 * R * U


def frac_bound(m: LinkModel, R: float):
    """(bound on |frac_dev - frac_model|, set aside) of a link window whose index was compared and equal; None, True where the peak is zero"""
    if not m.peak > 0.0:
        return None, True
    plain = 6.0 * R * m.U / m.peak
    if m.nb_gap > 2.0 * R * m.U:
        return plain, False
    return plain + 2.0 * abs(m.rec.frac), 2.0 * abs(m.rec.frac) > plain


def soft_reduced(i: int) -> bool:
    """reduced and full word tables on alternate windows"""
    return bool(i & 1)


def set_aside_census(kernel: str, st: Stream, down: np.ndarray, R: float):
    """Per window of st: (kind, comparisons, set aside, set aside on the window's tone) by the definition alone."""
    out = []
    for i, pos in enumerate(st.starts):
        kind = st.kinds[i]
        if kind == "zeros":
            out.append((kind, 0, 0, 0))
            continue
        tone = kind in TONE_KINDS
        if kernel == "detect":
            m = detect_model(st.iq, pos, down, st.nbins)
            a = [not index_compared(m.gap[0], m.U[0], R), not index_compared(m.gap[1], m.U[1], R)]
            if tone:                                              # (the "up" half of a tone window is flat: see the module docstring)
                out.append((kind, 1, int(a[0]), int(a[0])))
            else:
                out.append((kind, 2, sum(a), 0))
        elif kernel == "soft":
            m = soft_model(st.iq, pos, down, st.nbins, soft_reduced(i))
            a = not index_compared(m.gap, m.U, R)
            out.append((kind, 1, int(a), int(tone and a)))
        else:
            m = link_model(st.window(i), down, st.nbins, st.conj(i))
            a = not index_compared(m.gap, m.U, R)
            f = True if a else frac_bound(m, R)[1]
            out.append((kind, 2, int(a) + int(f), (int(a) + int(f)) if tone else 0))
    return out


@functools.lru_cache(maxsize=None)
def model_downchirp(sf: int, decim: int) -> np.ndarray:
    return LM.downchirp(sf, BW, rate(decim))


def grid_stream(sf: int, decim: int, down: np.ndarray, n_windows: int, step: int = 61):
    """Noise plus tones for the grid-stride cases: n_windows windows, one every `step` items -> (iq complex64, offsets)."""
    N, sps = 1 << sf, decim << sf
    n = (n_windows - 1) * step + sps + 5
    rng = np.random.default_rng([sf, decim, n_windows])
    t = np.arange(n, dtype=np.float64)
    s = _noise(rng, n, 0.5)
    for k in rng.integers(-N // 2, N // 2, 3):
        s = s + 0.4 * np.exp(2j * np.pi * (float(k) + float(rng.uniform(-0.5, 0.5))) * t / sps)
    cd = np.conj(np.asarray(down).astype(np.complex128)) / 2.0
    iq = (s * np.resize(cd, n)).astype(np.complex64)
    return iq, [2 + i * step for i in range(n_windows)]
