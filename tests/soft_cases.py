"""Streams shared by tests/test_soft_model.py (CPU) and tests/test_gpu_soft.py (device): the noisy frames of the gain cases, and the hard
chain - tests/chain_model.py on the words (L < 0) - that the soft decoder is compared with on the CPU."""
import functools

import numpy as np

import chain_model as CM
from gr_lora_amd import softdecode as SD, synth


@functools.lru_cache(None)
def gain_stream(sf, cr, length, n, snr_db, reduced=False, cfo_hz=0.0, valid=False, seed=None):
    """n frames of `length` random bytes, rng = default_rng(1000 + 10 sf + cr) (or `seed`).  valid: header checksum and payload CRC hold (one
    frame per stream call, so that each carries its own CRC bytes) -> (cfg, payloads, iq, header_starts, wanted frame bodies)"""
    rng = np.random.default_rng(1000 + 10 * sf + cr if seed is None else seed)
    payloads = [bytes(rng.integers(0, 256, length, dtype=np.uint8)) for _ in range(n)]
    sigma = synth.awgn_sigma_for_snr(snr_db, synth.TxConfig(sf=sf)) if snr_db is not None else 0.0
    if not valid:
        cfg = synth.TxConfig(sf=sf, cr=cr, reduced_rate=reduced)
        st = synth.build_stream(payloads, cfg, rng=rng, noise_sigma=sigma, cfo_hz=cfo_hz)
        return cfg, payloads, st.iq, list(st.header_starts), [synth.expected_frame_tail(p, cfg) for p in payloads]
    cfg = synth.TxConfig(sf=sf, cr=cr, reduced_rate=reduced, hdr_nibbles=synth.valid_hdr_nibbles(length, cr, True))
    pieces, starts, want, pos = [], [], [], 0
    for p in payloads:
        crc = synth.valid_crc_bytes(p)
        st = synth.build_stream([p], cfg, rng=rng, tail_symbols=0.0, crc_bytes=crc)
        pieces.append(st.iq)
        starts.append(pos + st.header_starts[0])
        want.append(synth.expected_frame_tail(p, cfg, crc))
        pos += st.iq.size
    pieces.append(np.zeros(3 * cfg.sps, dtype=np.complex64))
    iq = np.concatenate(pieces)
    if cfo_hz:
        iq = (iq * np.exp(2j * np.pi * cfo_hz * np.arange(iq.size, dtype=np.float64) / cfg.samp_rate)).astype(np.complex64)
    noise = rng.standard_normal((iq.size, 2)).astype(np.float32) * np.float32(sigma / np.sqrt(2.0))
    return cfg, payloads, (iq + noise[:, 0] + 1j * noise[:, 1]).astype(np.complex64), starts, want


def hard_frame(iq, header_pos, cfg, down):
    """the integer chain at header_pos on the arg-max words: the frame body, or None where the header asks for more than the capture holds"""
    sf, sps = cfg.sf, cfg.sps
    if header_pos + 9 * sps > iq.size:
        return None
    word = lambda k, red: sum(int(v < 0) << i for i, v in enumerate(SD.llr_window(iq, header_pos + k * sps, cfg, red, down)[0]))
    hw = [word(k, True) for k in range(8)]
    phdr = CM.header_bytes(CM.deinterleave(hw, sf - 2)[:5], cfg.cr)
    cr = min(phdr[1] >> 5, 4)
    if cr == 0:
        return None
    n_sym = CM.payload_symbol_count(phdr[0] + 2 * ((phdr[1] >> 4) & 1), sf, cr, cfg.reduced_rate)
    if header_pos + (8 + max(n_sym, 1) + 1) * sps > iq.size:
        return None
    pw = [word(8 + k, cfg.reduced_rate) for k in range(n_sym)]
    return CM.chain_decode(hw, pw, sf, cfg.cr, cfg.reduced_rate, demod=1)[0]
