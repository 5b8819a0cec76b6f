"""float64 numpy model of the polyphase DFT filter bank (gr_lora_amd/csrc/lora_filterbank.hip, include/lora_hip_filterbank.h).

Definition: row kappa is the channeliser's output (include/lora_hip_channelizer.h) for the frequency f = f0 + kappa fs / M,
    y_kappa[m] = sum_n h[n] x[mD - n] e^{-j 2 pi f (mD - n) / fs},     x[n < 0] = 0.
The steps the kernel takes, restated here one for one:
    1. premix      x'[n] = x[n] e^{-j 2 pi f0 n / fs}                         (n: absolute stream index)
    2. branches    v_r[m] = sum_q h[qM + r] x'[mD - qM - r],  r = 0 .. M-1    (h padded with zeros to a multiple of M)
    3. DFT         y_kappa[m] = sum_s e^{-j 2 pi kappa s / M} v_{(mD - s) mod M}[m]
Step 3 is step 2's e^{-j 2 pi kappa (mD - r) / M} with the grid part of the rotator as a cyclic shift of the branches by
mD mod M (exact integers).  Streaming as the device: history, absolute index and decimation phase carry over.

    python tools/filterbank_model.py      # checks the model against the direct formula on a short random stream
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gr_lora_amd.lora import low_pass_taps  # noqa: E402


class FilterBankModel:
    def __init__(self, samp_rate, grid_offset, n_grid, channels, bandwidth, decimation=1, cutoff_hz=0.0, transition_hz=0.0):
        self.fs = float(samp_rate)
        self.f0 = float(grid_offset)
        self.M = int(n_grid)
        self.channels = [int(k) for k in channels]
        self.D = int(decimation)
        cutoff = float(cutoff_hz) if cutoff_hz > 0 else float(int(bandwidth) // 2) + 15000.0
        transition = float(transition_hz) if transition_hz > 0 else 10000.0
        self.taps = low_pass_taps(1.0, self.fs, cutoff, transition)
        self.Q = -(-self.taps.size // self.M)
        self.Lp = self.Q * self.M
        self.h = np.zeros(self.Lp)
        self.h[: self.taps.size] = self.taps
        k = np.asarray(self.channels, dtype=np.int64)
        self.E = np.exp(-2j * np.pi * ((k[:, None] * np.arange(self.M)[None, :]) % self.M) / self.M)   # [n_sel, M]
        self._hist = np.zeros(self.Lp - 1, dtype=np.complex128)   # premixed input history
        self._n = 0

    def _premix(self, x, n0):
        t = (self.f0 / self.fs) * (n0 + np.arange(x.size, dtype=np.float64))
        return x * np.exp(-2j * np.pi * (t - np.floor(t)))

    def work(self, x) -> np.ndarray:
        """complex64/128[n_in] -> complex128[n_sel, n_out]."""
        x = np.asarray(x).astype(np.complex128)
        buf = np.concatenate([self._hist, self._premix(x, self._n)])             # buf[i] <-> absolute n - (Lp - 1) + i
        first = (-self._n) % self.D
        pos = np.arange(first, x.size, self.D, dtype=np.int64)                   # local index of each output's newest input
        out = np.zeros((len(self.channels), pos.size), dtype=np.complex128)
        hq = self.h.reshape(self.Q, self.M)
        for b in range(0, pos.size, 1024):
            p = pos[b:b + 1024]
            win = buf[(p + self.Lp - 1)[:, None] - np.arange(self.Lp)[None, :]]  # win[m, j] = x'[mD - j]
            v = (win.reshape(p.size, self.Q, self.M) * hq[None]).sum(axis=1)      # v[m, r]
            shift = (self._n + p) % self.M                                        # mD mod M, exact
            s = np.arange(self.M)
            u = v[np.arange(p.size)[:, None], (shift[:, None] - s[None, :]) % self.M]   # u[m, s] = v_{(mD - s) mod M}
            out[:, b:b + p.size] = self.E @ u.T
        self._hist = buf[buf.size - (self.Lp - 1):] if self.Lp > 1 else buf[:0]
        self._n += x.size
        return out


def direct(samp_rate, freq, taps, decimation, x):
    """The definition, one channel, one shot: y[m] = sum_n h[n] x[mD - n] e^{-j 2 pi f (mD - n) / fs}."""
    n = np.arange(x.size, dtype=np.float64)
    t = freq / samp_rate * n
    xm = x.astype(np.complex128) * np.exp(-2j * np.pi * (t - np.floor(t)))
    return np.convolve(xm, taps.astype(np.float64))[: x.size][::decimation]


if __name__ == "__main__":
    rng = np.random.default_rng(1)
    x = rng.standard_normal(20000) + 1j * rng.standard_normal(20000)
    m = FilterBankModel(2e6, 100e3, 10, range(-5, 5), 125000, 3)
    y = np.concatenate([m.work(x[:777]), m.work(x[777:])], axis=1)
    err = max(float(np.abs(y[i] - direct(2e6, 100e3 + k * 2e5, m.taps, 3, x)).max()) for i, k in enumerate(m.channels))
    print("max |model - direct| = %.2e (max |y| = %.2f)" % (err, float(np.abs(y).max())))
