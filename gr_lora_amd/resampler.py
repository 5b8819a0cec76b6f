"""The rational resampler's definition in float64 (include/lora_hip_resampler.h restated; csrc/lora_resampler.hip is held to it).

The stream is x[n], n = 0, 1, ..., x[n < 0] = 0.  L / M is the ratio in lowest terms, R = max(L, M).
    filter   ntaps = 2 Z R + 1;  h[k] = fl32(L (c / R) sinc((k - Z R) c / R) kaiser_beta(k)), formed in double, rounded once;
             kaiser_beta = numpy.kaiser(ntaps, beta).  Q = ceil(ntaps / L) taps per output, h[k >= ntaps] = 0.
    output   m:  t = m M, p = t mod L, n0 = t div L;  y[m] = sum_{j < Q} h[p + j L] x[n0 - j]
    count    after N input items exactly ceil(N L / M) outputs exist (every m with m M < N L)
    delay    Z R / M output items
This is the project's own definition, not a restatement of another library's resampler.
"""
from __future__ import annotations

from fractions import Fraction
from math import gcd

import numpy as np

MAX_RATIO = 512                 # include/lora_hip_resampler.h
MIN_ZERO_CROSSINGS, MAX_ZERO_CROSSINGS = 2, 32
MAX_BETA = 20
MAX_TAPS = 16385
MAX_Q = 1024
DEFAULT_ZERO_CROSSINGS, DEFAULT_BETA, DEFAULT_CUTOFF = 16, 8.0, 0.8


def reduce(L, M):
    """(L, M) in lowest terms."""
    L, M = int(L), int(M)
    if L < 1 or M < 1:
        raise ValueError("interpolation %d and decimation %d must be at least 1" % (L, M))
    g = gcd(L, M)
    return L // g, M // g


def ratio(in_rate, out_rate):
    """The reduced (L, M) with out_rate / in_rate = L / M, both within 1 .. MAX_RATIO; ValueError when no such pair meets the
    quotient to 1e-9 relative."""
    fi, fo = float(in_rate), float(out_rate)
    if not (np.isfinite(fi) and np.isfinite(fo) and fi > 0.0 and fo > 0.0):
        raise ValueError("rates must be positive and finite, not %r -> %r" % (in_rate, out_rate))
    want = Fraction(fo) / Fraction(fi)
    got = want.limit_denominator(MAX_RATIO)
    if got.numerator < 1 or got.numerator > MAX_RATIO or abs(got - want) > Fraction(1, 10 ** 9) * want:
        raise ValueError("%r -> %r is no ratio L / M with L, M <= %d" % (in_rate, out_rate, MAX_RATIO))
    return got.numerator, got.denominator


def n_taps(L, M, zero_crossings=DEFAULT_ZERO_CROSSINGS):
    L, M = reduce(L, M)
    return 2 * int(zero_crossings) * max(L, M) + 1


def taps_per_output(L, M, zero_crossings=DEFAULT_ZERO_CROSSINGS):
    """Q = ceil(ntaps / L)."""
    L, M = reduce(L, M)
    return -(-n_taps(L, M, zero_crossings) // L)


def check(L, M, zero_crossings=DEFAULT_ZERO_CROSSINGS, beta=DEFAULT_BETA, cutoff=DEFAULT_CUTOFF):
    """The limits of the header (on L and M as given, like the library); ValueError outside them.  -> the reduced (L, M)."""
    if not (1 <= int(L) <= MAX_RATIO and 1 <= int(M) <= MAX_RATIO):
        raise ValueError("interpolation %r and decimation %r must lie in 1 .. %d" % (L, M, MAX_RATIO))
    if not MIN_ZERO_CROSSINGS <= int(zero_crossings) <= MAX_ZERO_CROSSINGS:
        raise ValueError("zero_crossings %r must lie in %d .. %d" % (zero_crossings, MIN_ZERO_CROSSINGS, MAX_ZERO_CROSSINGS))
    if not 0.0 <= float(beta) <= MAX_BETA:
        raise ValueError("beta %r must lie in 0 .. %d" % (beta, MAX_BETA))
    if not 0.0 < float(cutoff) <= 1.0:
        raise ValueError("cutoff %r must lie in (0, 1]" % (cutoff,))
    l, m = reduce(L, M)
    if n_taps(l, m, zero_crossings) > MAX_TAPS:
        raise ValueError("%d taps: at most %d" % (n_taps(l, m, zero_crossings), MAX_TAPS))
    if taps_per_output(l, m, zero_crossings) > MAX_Q:
        raise ValueError("%d taps per output: at most %d (deep decimation is the channeliser's job)" % (taps_per_output(l, m, zero_crossings), MAX_Q))
    return l, m


def design(L, M, zero_crossings=DEFAULT_ZERO_CROSSINGS, beta=DEFAULT_BETA, cutoff=DEFAULT_CUTOFF) -> np.ndarray:
    """The prototype filter: float32[2 Z R + 1]."""
    L, M = check(L, M, zero_crossings, beta, cutoff)
    Z, R, c = int(zero_crossings), max(L, M), float(cutoff)
    ntaps = 2 * Z * R + 1
    k = np.arange(ntaps, dtype=np.float64)
    gain = L * (c / R)
    h = gain * np.sinc((k - Z * R) * c / R) * np.kaiser(ntaps, float(beta))
    return h.astype(np.float32)


def output_items(total_in, L, M) -> int:
    """Outputs that exist after total_in input items: ceil(total_in L / M)."""
    L, M = reduce(L, M)
    return -(-int(total_in) * L // M)


def delay(L, M, zero_crossings=DEFAULT_ZERO_CROSSINGS) -> float:
    """The group delay in output items: Z R / M."""
    L, M = reduce(L, M)
    return int(zero_crossings) * max(L, M) / M


def resample(x, L, M, taps):
    """-> (y complex128[ceil(N L / M)], bound float64): the definition on the whole of x, and bound[m] = sum_j |h[p + j L]| |x[n0 - j]|,
    what a rounding bound of the Q-term sum scales with."""
    L, M = reduce(L, M)
    x = np.asarray(x, dtype=np.complex128).reshape(-1)
    h = np.asarray(taps, dtype=np.float64).reshape(-1)
    Q = -(-h.size // L)
    hp = np.zeros(Q * L + L, dtype=np.float64)
    hp[:h.size] = h
    n_out = output_items(x.size, L, M)
    t = np.arange(n_out, dtype=np.int64) * M
    p, n0 = t % L, t // L
    xz = np.concatenate([np.zeros(Q, dtype=np.complex128), x])      # xz[Q + n] = x[n], zeros in front
    ax = np.abs(xz)
    y = np.zeros(n_out, dtype=np.complex128)
    bound = np.zeros(n_out, dtype=np.float64)
    for j in range(Q):
        hj = hp[p + j * L]
        idx = n0 - j + Q
        y += hj * xz[idx]
        bound += np.abs(hj) * ax[idx]
    return y, bound
