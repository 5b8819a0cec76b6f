"""Shared by the conditioner's CPU and GPU tests: the impaired captures of the end-to-end cases and the synthetic inputs, each
made once and never changed."""
import functools

import numpy as np

from gr_lora_amd import conditioner, synth

AMPLITUDE = 0.25
SNR_DB = 50.0
N_FRAMES, PAYLOAD_BYTES = 8, 16
DC_ANGLE = 0.7
# (gain mismatch in dB, phase mismatch in degrees, DC level in dB relative to the signal)
IMPAIRMENTS = [(2.0, 10.0, -6.0), (3.0, 15.0, 0.0)]


@functools.lru_cache(maxsize=None)
def payloads():
    rng = np.random.default_rng(5)
    return tuple(bytes(rng.integers(0, 256, PAYLOAD_BYTES, dtype=np.uint8)) for _ in range(N_FRAMES))


def dc_offset(dbc, amplitude=AMPLITUDE):
    return amplitude * 10.0 ** (dbc / 20.0) * np.exp(1j * DC_ANGLE)


@functools.lru_cache(maxsize=None)
def clean_capture(sf):
    """8 frames of 16 bytes, CR 4, amplitude 0.25, gaps of 8 .. 12 symbols, AWGN 50 dB under the signal in its band."""
    cfg = synth.TxConfig(sf=sf, cr=4)
    st = synth.build_stream(list(payloads()), cfg, rng=np.random.default_rng(1), gap_symbols=(8, 12), amplitude=AMPLITUDE,
                            noise_sigma=synth.awgn_sigma_for_snr(SNR_DB, cfg, AMPLITUDE))
    st.iq.setflags(write=False)
    return cfg, st.iq


@functools.lru_cache(maxsize=None)
def impaired_capture(sf, gain_db, phase_deg, dbc):
    """The clean capture behind y = I + j g (Q cos phi + I sin phi) + d, complex64."""
    _, x = clean_capture(sf)
    y = conditioner.impair(x, gain_db, phase_deg, dc_offset(dbc)).astype(np.complex64)
    y.setflags(write=False)
    return y


def tails(sf):
    cfg, _ = clean_capture(sf)
    return [synth.expected_frame_tail(p, cfg) for p in payloads()]


INPUTS = ["impaired", "zeros", "constant", "dc40"]
CONSTANT = np.complex64(0.375 - 0.8125j)      # short mantissas: every sum and every square of the definition is exact


@functools.lru_cache(maxsize=None)
def synthetic(kind, n):
    """complex64[n]: circular noise of power 0.01 behind (2 dB, 10 degrees, DC at -6 dBc); exact zeros; one constant; the same
    noise with a DC offset 40 dB over it."""
    rng = np.random.default_rng([INPUTS.index(kind), n])
    noise = 0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    if kind == "impaired":
        x = conditioner.impair(noise, 2.0, 10.0, dc_offset(-6.0, 0.1))
    elif kind == "zeros":
        x = np.zeros(n)
    elif kind == "constant":
        x = np.full(n, CONSTANT)
    else:
        x = noise + dc_offset(40.0, 0.1)
    x = x.astype(np.complex64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def capture_at_2400k():
    """The clean SF7 capture plus 4096 zeros taken up 12/5 to 2.4 Msps by the resampler's float64 model, then impaired there by
    (2 dB, 10 degrees, DC at -6 dBc): complex64."""
    from gr_lora_amd import resampler
    _, x = clean_capture(7)
    hi, _ = resampler.resample(np.concatenate([x, np.zeros(4096, dtype=np.complex64)]), 12, 5, resampler.design(12, 5))
    y = conditioner.impair(hi, 2.0, 10.0, dc_offset(-6.0)).astype(np.complex64)
    y.setflags(write=False)
    return y
