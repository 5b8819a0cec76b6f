"""The capture the spectral-scan tests share (tests/test_spectrum_model.py, test_spectrum_tool.py, test_gpu_spectrum.py): two SF7
emitters on a gateway grid of 10 at 2 Msps, a strong one at -400 kHz and one 12 dB down at +200 kHz, silence before and after."""
import numpy as np

from gr_lora_amd import spectrum, synth

FS = 2e6
N_GRID = 10
GRID_OFFSET = 0.0
CHANNELS = list(range(-4, 5))          # -800 kHz .. +800 kHz, 200 kHz apart
BANDWIDTH = 125000
NFFT, HOP, N_AVG = 1024, 512, 4
N_ITEMS = 163840
# (payload, start, freq_hz, amplitude): starts that are no multiple of the hop
EMITTERS = [
    (bytes(range(1, 17)), 6001, -400e3, 1.0),
    (bytes(range(101, 117)), 11003, 200e3, 0.25),
]
STRONG, WEAK = CHANNELS.index(-2), CHANNELS.index(1)


def frames():
    out = []
    for pl, start, f, a in EMITTERS:
        cfg = synth.TxConfig(sf=7, cr=4, bw=BANDWIDTH, hdr_nibbles=synth.valid_hdr_nibbles(len(pl), 4, True))
        out.append(synth.WidebandFrame(pl, cfg, start, f, a, synth.valid_crc_bytes(pl)))
    return out


def frame_spans():
    """[start, end) of every emitter in samples."""
    return [(f.start, f.start + synth.wideband_waveform(f, FS).size) for f in frames()]


def capture():
    """The float64 model of the capture (complex128[N_ITEMS])."""
    return synth.build_wideband(frames(), FS, 0, N_ITEMS)


def bands():
    return spectrum.grid_bands(FS, NFFT, GRID_OFFSET, N_GRID, CHANNELS, BANDWIDTH)


def rows_inside_all(first_sample):
    """Rows lying wholly inside every emitter's frame."""
    span = (N_AVG - 1) * HOP + NFFT
    lo = max(s for s, _ in frame_spans())
    hi = min(e for _, e in frame_spans())
    return [r for r, s in enumerate(first_sample) if s >= lo and s + span <= hi]


def rows_before_any(first_sample):
    span = (N_AVG - 1) * HOP + NFFT
    lo = min(s for s, _ in frame_spans())
    return [r for r, s in enumerate(first_sample) if s + span <= lo]
