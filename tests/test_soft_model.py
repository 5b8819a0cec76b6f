"""CPU: the float64 definition of the soft-decision decoder (gr_lora_amd/softdecode.py) against the bit-level model of the integer chain
(tests/chain_model.py) where the two must agree - clean frames, unit LLRs, the tie rule - and what it adds: erasure decoding at 4/5 .. 4/7 and
about 2 dB of decoding sensitivity."""
import functools

import numpy as np
import pytest

import chain_model as CM
import soft_cases as SC
from gr_lora_amd import softdecode as SD, synth


def _frame(cfg, payload, snr_db=None, seed=0):
    rng = np.random.default_rng(seed)
    sigma = synth.awgn_sigma_for_snr(snr_db, cfg) if snr_db is not None else 0.0
    return synth.build_stream([payload], cfg, gaps=[2 * cfg.sps + 77], rng=rng, noise_sigma=sigma)


CLEAN = [(sf, sf > 10) for sf in range(7, 13)] + [(9, True)]


@pytest.mark.parametrize("sf,reduced", CLEAN)
def test_clean_frames_equal_the_integer_chain(sf, reduced):
    down = SD._down(synth.TxConfig(sf=sf))
    for cr in (1, 2, 3, 4):
        for length in (1, 16, 255):
            cfg = synth.TxConfig(sf=sf, cr=cr, reduced_rate=reduced)
            payload = bytes(np.random.default_rng(sf * 1000 + cr * 10 + length).integers(0, 256, length, dtype=np.uint8))
            st = _frame(cfg, payload)
            hs, ps = st.shifts[0]
            N = cfg.nbins
            hw = CM.bins_to_words([(s - 1) % N for s in hs], sf, True, demod=1)
            pw = CM.bins_to_words([(s - 1) % N for s in ps], sf, reduced, demod=1)
            want, (_, cr_dec, n_sym, _) = CM.chain_decode(hw, pw, sf, cr, reduced, demod=1)
            got, rep = SD.decode_frame(st.iq, st.header_starts[0], cfg, down=down)
            assert got == want == synth.expected_frame_tail(payload, cfg), (sf, cr, length)
            assert (rep["status"], rep["cr"], rep["payload_symbols"], rep["changed"]) == (SD.STATUS_FRAME, cr_dec, n_sym, 0)
            assert rep["end_pos"] == st.header_starts[0] + (8 + len(ps)) * cfg.sps and rep["min_margin"] > 0
            assert rep["words"] == hw + pw, (sf, cr, length)                   # the hard words (L < 0) of every symbol
            for k in (0, 7, 8, 7 + len(ps)):                                    # (and no LLR of a clean symbol is exactly 0)
                assert (SD.llr_window(st.iq, st.header_starts[0] + k * cfg.sps, cfg, k < 8 or reduced, down)[0] != 0).all(), (sf, cr, length, k)


def test_hard_word_is_the_word_of_the_argmax():
    rng = np.random.default_rng(3)
    for sf, reduced in ((7, False), (7, True), (9, False), (10, True)):
        for _ in range(20):
            m = rng.random(1 << sf)
            L = SD.llr_of_magnitudes(m, sf, reduced)
            k = int(np.argmax(m))
            assert sum(int(v < 0) << i for i, v in enumerate(L)) == CM.bins_to_words([(k - 1) % (1 << sf)], sf, reduced, demod=1)[0]


def _unit_llrs(word_bits, n_w=8):
    """LLRs of one block (ppm = 1 codeword position used: x = 0 of a ppm-wide block) such that D[j] = +-1 by the bits of `word_bits`"""
    ppm = 8
    L = np.ones((n_w, ppm))
    for j in range(8):
        i = CM.SHUFFLE[j]
        if i < n_w:
            L[i][(0 - i) % ppm] = -1.0 if (word_bits >> j) & 1 else 1.0
    return L


def test_tie_rule_equals_hamming84_on_unit_llrs():
    for c in range(256):
        for dtype in (np.float64, np.float32):
            nib, mar, hard, _ = SD.soft_block(_unit_llrs(c), 8, 8, [0], dtype)
            assert nib[0] == CM.H84[c] and hard[0] == c and mar[0] >= 0
    for c in range(0, 256, 7):                                                  # and behind a whitening byte
        nib, _, hard, _ = SD.soft_block(_unit_llrs(c), 8, 8, [0x5a])
        assert nib[0] == CM.H84[c ^ 0x5a] and hard[0] == c ^ 0x5a


@pytest.mark.parametrize("n_w", [5, 6, 7])
def test_erasures_decode_every_nibble(n_w):
    for s in range(16):
        nib, mar, _, _ = SD.soft_block(_unit_llrs(CM.ENC[s], n_w), 8, n_w, [0])
        assert nib[0] == s and mar[0] > 0
    if n_w == 5:                                                                # 4/5: one weak, wrong data bit under the parity bit (b0, b1, b2) is put right by it
        for s in range(16):
            for j in (1, 2, 3):
                L = _unit_llrs(CM.ENC[s], 5)
                i = CM.SHUFFLE[j]
                L[i][(0 - i) % 8] *= -0.2
                nib, _, hard, _ = SD.soft_block(L, 8, 5, [0])
                assert nib[0] == s and SD.hard_nibble(hard[0], 1) != s


@functools.lru_cache(None)
def gain_counts(sf, cr, length, n, snr_db, reduced=False):
    """(hard_ok, soft_ok) of n frames at their true header positions; hard: the integer chain on the words (L < 0)"""
    cfg, _payloads, iq, starts, want = SC.gain_stream(sf, cr, length, n, snr_db, reduced)
    down = SD._down(cfg)
    soft_ok = sum(SD.decode_frame(iq, hp, cfg, down=down)[0] == w for hp, w in zip(starts, want))
    hard_ok = sum(SC.hard_frame(iq, hp, cfg, down) == w for hp, w in zip(starts, want))
    return hard_ok, soft_ok


def test_gain_sf7_cr48():
    hard, soft = gain_counts(7, 4, 16, 40, -8.0)
    print("SF7 4/8 16 B -8 dB: hard %d soft %d of 40" % (hard, soft))
    assert soft >= hard + 10


def test_gain_sf7_cr45():
    hard, soft = gain_counts(7, 1, 64, 30, -2.5)
    print("SF7 4/5 64 B -2.5 dB: hard %d soft %d of 30" % (hard, soft))
    assert soft >= hard + 30 / 4


@pytest.mark.parametrize("cr", [1, 4])
def test_high_snr_decodes_everything_both_ways(cr):
    assert gain_counts(7, cr, 16, 12, 30.0) == (12, 12)


def test_fp32_chain_equals_float64_outside_near_ties():
    """soft_chain(dtype=float32) on the float64 LLRs cast to fp32 decides every codeword as float64 does wherever the float64 margin exceeds 1e-5 * peak."""
    cfg, _p, iq, starts, _want = SC.gain_stream(7, 2, 24, 8, -6.0, seed=77)
    down = SD._down(cfg)
    checked = 0
    for hp in starts:
        Lh = np.array([SD.llr_window(iq, hp + k * cfg.sps, cfg, True, down)[0] for k in range(8)])
        _, r64 = SD.soft_chain(Lh, None, cfg)
        n_sym = r64["payload_symbols"]
        if r64["status"] != SD.STATUS_TRUNCATED or hp + (9 + max(n_sym, 1)) * cfg.sps > iq.size:
            continue
        W = [SD.llr_window(iq, hp + (8 + k) * cfg.sps, cfg, False, down) for k in range(n_sym)]
        Lp = np.array([w[0] for w in W]).reshape(n_sym, 7)
        peak = max(w[2] for w in W)
        b64, r64 = SD.soft_chain(Lh, Lp, cfg)
        b32, r32 = SD.soft_chain(Lh.astype(np.float32), Lp.astype(np.float32), cfg, np.float32)
        assert r32["margins"][0].dtype == np.float32 and len(r64["nibbles"]) == r64["codewords"]
        sure = [m > 1e-5 * peak for m in r64["margins"]]
        if all(sure[:5]):                                                       # (the same header: the same codewords behind it)
            assert r32["nibbles"][:5] == r64["nibbles"][:5] and len(r32["nibbles"]) == len(r64["nibbles"])
            for a, b, ok in zip(r64["nibbles"], r32["nibbles"], sure):
                if ok:
                    assert a == b
                    checked += 1
            if all(sure):
                assert b32 == b64 and r32["changed"] == r64["changed"]
    assert checked > 200
