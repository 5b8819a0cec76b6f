"""CPU: the float64 model of the polyphase filter bank (tools/filterbank_model.py: premix, branch sums, shifted DFT) equals the
channeliser's oracle (oracle/channelizer_oracle.Channelizer) on every selected grid channel, under streaming chunks."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from filterbank_model import FilterBankModel  # noqa: E402

# (fs, M, D, n_in): the oracle's offset is float32 truncated to whole Hz, so fs / M and f0 are whole Hz
CASES = [(2e6, 10, 2, 20000), (2e6, 10, 3, 20000), (2e6, 8, 8, 20000), (1.75e6, 7, 16, 20000), (16e6, 80, 16, 24000)]


def _grid(M):
    return list(range(-(M // 2), (M + 1) // 2))     # [-floor(M/2), ceil(M/2) - 1]


@pytest.mark.parametrize("fs,M,D,n", CASES)
@pytest.mark.parametrize("f0", [0.0, 100e3])
def test_model_equals_oracle_per_channel(fs, M, D, n, f0):
    from oracle import channelizer_oracle as co
    rng = np.random.default_rng(M * 100 + D)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    ks = _grid(M)
    if M > 16:   # the 3855-tap oracle is slow: both grid ends, the middle, and three more
        ks = [ks[0], ks[1], -1, 0, 1, ks[-1]]
    model = FilterBankModel(fs, f0, M, ks, 125000, D)
    oracles = [co.Channelizer(fs, 0.0, f0 + k * fs / M, 125000, D) for k in ks]
    assert np.array_equal(model.taps, oracles[0].taps)
    sizes = [1, D - 1 if D > 1 else 2, 5, model.taps.size - 3, 4097, 333]
    got, want = [], [[] for _ in ks]
    pos, i = 0, 0
    while pos < n:
        c = min(sizes[i % len(sizes)], n - pos) or 1
        i += 1
        got.append(model.work(x[pos:pos + c]))
        for j, o in enumerate(oracles):
            want[j].append(o.work(x[pos:pos + c]) if c else np.zeros(0))
        pos += c
    y = np.concatenate(got, axis=1)
    for j, k in enumerate(ks):
        w = np.concatenate(want[j])
        assert y[j].shape == w.shape
        err = np.abs(y[j] - w).max() / np.abs(w).max()
        assert err <= 1e-9, (k, err)


def test_grid_edges_and_non_dividing_decimation():
    """kappa = +-M/2 (both signs of the Nyquist bin on an even grid) and a D that neither divides M nor is divided by it."""
    from oracle import channelizer_oracle as co
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(9000) + 1j * rng.standard_normal(9000)).astype(np.complex64)
    for ks in ([-5, 4], [-4, 5]):
        model = FilterBankModel(2e6, 37.0, 10, ks, 125000, 3)
        y = model.work(x)
        for j, k in enumerate(ks):
            w = co.Channelizer(2e6, 0.0, 37.0 + k * 2e5, 125000, 3).work(x)
            assert np.abs(y[j] - w).max() <= 1e-9 * np.abs(w).max(), k
