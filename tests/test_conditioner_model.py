"""CPU: the IQ conditioner's float64 definition (gr_lora_amd/conditioner.py) - the estimator on known impairments, the guards, the
summation order, and end to end through the CPU oracle on impaired captures."""
import numpy as np
import pytest

import conditioner_cases as cc
from gr_lora_amd import conditioner as cd
from oracle import oracle as O

B, W = 4096, 16


@pytest.mark.parametrize("gain_db,phase_deg,dbc", [(0.0, 0.0, -6.0), (0.0, 0.0, 10.0), (2.0, 10.0, None), (2.0, 10.0, -6.0), (3.0, 15.0, 0.0)])
def test_estimator_recovers_known_impairments(gain_db, phase_deg, dbc):
    """Circular Gaussian noise of power P = 2 s^2 behind y = I + j g (Q cos phi + I sin phi) + d; the last block's window holds
    N = W B items.  Variances of the estimates over N independent items (Gaussian fourth moments):
        d:    var(mI) = s^2 / N, var(mQ) = g^2 s^2 / N              |d^ - d| has deviation s sqrt((1 + g^2) / N)
        g:    q = cQQ / cII, var(ln q) = (4 / N) cos^2 phi           ln g^ has deviation cos phi / sqrt(N) <= 1 / sqrt(N)
        phi:  sin phi^ is the sample correlation, variance cos^4 phi / N   phi^ has deviation cos phi / sqrt(N) <= 1 / sqrt(N) rad
    The test allows five deviations of each (plus the O(1 / N) bias, 4 / N): with N = 65536 that is 0.17 dB and 1.12 degrees."""
    n = W * B
    rng = np.random.default_rng(11)
    s = 0.25 / np.sqrt(2.0)
    z = s * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    d = cc.dc_offset(dbc) if dbc is not None else 0.0
    y = cd.impair(z, gain_db, phase_deg, d).astype(np.complex64)
    _, mom, par = cd.condition(y, B, W)
    S, nw = cd.window_sums(mom, W)
    assert nw[-1] == W
    est = cd.estimate(S[-1], float(n))
    g = 10.0 ** (gain_db / 20.0)
    k = 5.0 / np.sqrt(n) + 4.0 / n
    assert abs(est["dc"] - d) <= 5.0 * s * np.sqrt((1.0 + g * g) / n) + 2.0 ** -24
    assert abs(est["gain_db"] - gain_db) <= 20.0 / np.log(10.0) * k
    assert abs(est["phase_deg"] - phase_deg) <= np.degrees(k)
    if abs(d) > 0:
        assert abs(est["dc_dbfs"] - 20.0 * np.log10(abs(d))) <= 20.0 / np.log(10.0) * 5.0 * s * np.sqrt((1.0 + g * g) / n) / abs(d) * 1.1
    # the parameters are the model's: a = -tan phi, b = 1 / (g cos phi), to the same five deviations (first order in both)
    phi = np.radians(phase_deg)
    assert abs(par[-1, 2] + np.tan(phi)) <= k / np.cos(phi) ** 2 + 2.0 ** -23
    assert abs(par[-1, 3] * g * np.cos(phi) - 1.0) <= k * (1.0 + abs(np.tan(phi))) + 2.0 ** -23


def test_summation_order_is_the_stated_one():
    """block_moments against a scalar restatement: 64 ascending chains from +0, then the halving tree."""
    rng = np.random.default_rng(3)
    x = ((rng.standard_normal(512) + 1j * rng.standard_normal(512)) * 1e3 + 7.0).astype(np.complex64)
    got = cd.block_moments(x, 256)
    assert got.shape == (2, 5)
    for k in range(2):
        I, Q = x[256 * k:256 * (k + 1)].real.astype(np.float64), x[256 * k:256 * (k + 1)].imag.astype(np.float64)
        for c, term in enumerate((I, Q, I * I, Q * Q, I * Q)):
            t = [0.0] * 64
            for i in range(256):
                t[i % 64] = t[i % 64] + float(term[i])
            s = 32
            while s:
                for i in range(s):
                    t[i] = t[i] + t[i + s]
                s //= 2
            assert np.float64(t[0]).view(np.uint64) == got[k, c].view(np.uint64)
    S, nw = cd.window_sums(got, 3)
    assert list(nw) == [1, 2] and np.array_equal(S[1], (np.zeros(5) + got[0]) + got[1])


@pytest.mark.parametrize("value", [0.0, complex(cc.CONSTANT), 0.1 + 0.7j, -1e-20 + 3e4j])
def test_zeros_and_a_constant_come_out_finite(value):
    """cII is 0 (or rounding dust): the guard gives a = 0, b = 1 where the sums are exact, and the output is finite everywhere."""
    x = np.full(3 * 256 + 17, value, dtype=np.complex64)
    y, mom, par = cd.condition(x, 256, 2)
    assert np.isfinite(y.view(np.float32)).all() and np.isfinite(par).all() and np.isfinite(mom).all()
    if value in (0.0, complex(cc.CONSTANT)):
        assert np.array_equal(par[:, 2:], np.tile(np.float32([0.0, 1.0]), (3, 1)))
        assert np.array_equal(par[:, 0], np.full(3, x[0].real)) and np.array_equal(par[:, 1], np.full(3, x[0].imag))
        assert not y.view(np.uint32).any()                                          # (c - c = +0)
    y2, _, par2 = cd.condition(x, 256, 2, dc=False, iq=False)
    assert np.array_equal(y2.view(np.uint32), x.view(np.uint32)) and np.array_equal(par2, np.tile(np.float32(cd.IDENTITY), (3, 1)))


def test_a_stream_shorter_than_a_block_is_the_identity():
    x = (np.arange(100) * (0.01 + 0.02j) + 0.5).astype(np.complex64)
    y, mom, par = cd.condition(x, 256, 4)
    assert mom.shape == (0, 5) and par.shape == (0, 4) and np.array_equal(y.view(np.uint32), x.view(np.uint32))


def test_limits():
    for bad in (dict(block=128), dict(block=131072), dict(block=4097), dict(block=3000), dict(window=0), dict(window=257)):
        with pytest.raises(ValueError):
            cd.check(**bad)
    assert cd.check(256, 1) == (256, 1) and cd.check(65536, 256) == (65536, 256) and cd.check() == (4096, 16)


@pytest.mark.parametrize("gain_db,phase_deg,dbc", cc.IMPAIRMENTS)
@pytest.mark.parametrize("sf", [7, 8, 10])
def test_end_to_end_through_the_oracle(sf, gain_db, phase_deg, dbc):
    """The impaired capture decodes to fewer than the 8 transmitted payloads as it is and to all 8 behind the conditioner."""
    y = cc.impaired_capture(sf, gain_db, phase_deg, dbc)
    want = cc.tails(sf)
    raw = [f[15:] for f in O.decode_stream(y, sf=sf, cr=4)]
    assert sum(t in raw for t in want) < len(want)
    z, _, _ = cd.condition(y, B, W)
    got = [f[15:] for f in O.decode_stream(z, sf=sf, cr=4)]
    assert got == want
