"""CPU: the definition of the CRC-aided repair (gr_lora_amd/softdecode.py crc_repair) - the syndrome's linearity that the pattern
search rests on, the tie rules on hand-made margins, what a failed repair leaves alone, and what the repair gains on noisy frames."""
import functools

import numpy as np
import pytest

import soft_cases as SC
import soft_repair_cases as RC
from gr_lora_amd import softdecode as SD, synth

TODAY = {"status", "cr", "payload_length", "payload_symbols", "header_checksum_ok", "has_crc", "crc_ok", "codewords", "changed", "min_margin",
         "mean_abs_llr", "nibbles", "margins", "peak", "end_pos", "words"}          # the report of decode_frame for a published frame


def test_syndrome_is_the_frame_check():
    from gr_lora_amd import capi
    rng = np.random.default_rng(5)
    for length in (0, 1, 2, 3, 17, 255):
        for valid in (True, False):
            payload = bytes(rng.integers(0, 256, length, dtype=np.uint8))
            body = payload + (synth.valid_crc_bytes(payload) if valid else bytes(rng.integers(0, 256, 2, dtype=np.uint8)))
            fc = capi.check_frame(bytes(15) + bytes([length, (4 << 5) | 0x10, 0]) + body)
            assert fc.has_crc and SD.syndrome(list(body), length) == fc.crc_calc ^ fc.crc_rx
            assert (SD.syndrome(list(body), length) == 0) == bool(fc.crc_ok) and (not valid or fc.crc_ok)


@pytest.mark.parametrize("length", [0, 1, 2, 3, 17, 255])
def test_linearity(length):
    """the XOR of the candidates' fixed effects predicts the syndrome of the changed body, for every pattern of 8 candidates"""
    rng = np.random.default_rng(100 + length)
    n_cw = 2 * (length + 2)
    for trial in range(3):
        body = [int(b) for b in rng.integers(0, 256, length + 2)]
        nib = [(b >> (4 * t)) & 15 for b in body for t in (0, 1)]
        must = [n_cw - 1, n_cw - 4] + ([0, 1] if n_cw >= 8 else [])          # inside the CRC bytes; two in one byte
        rest = [c for c in range(n_cw) if c not in must]
        cand = must + [int(c) for c in rng.choice(rest, size=min(8, n_cw) - len(must), replace=False)]
        delta = [int(rng.integers(1, 16)) for _ in cand]
        e = [SD.syndrome_effect(c, d, length) for c, d in zip(cand, delta)]
        syn = SD.syndrome(body, length)
        for p in range(1 << len(cand)):
            new, x = list(nib), 0
            for i, (c, d) in enumerate(zip(cand, delta)):
                if (p >> i) & 1:
                    new[c] ^= d
                    x ^= e[i]
            assert SD.syndrome(SD.body_bytes(new, length + 2), length) == syn ^ x, (length, trial, p)


def _run(case, dtype=np.float32):
    _name, length, nib, sec, mar, L = case
    return SD.crc_repair(nib, sec, mar, length + 2, L, dtype)


def _by_name(name):
    return next(c for c in RC.edge_cases() if c[0] == name)


EXPECT = {  # name -> (status, codewords or their first ones, pattern)
    "crc holds": (SD.REPAIR_CRC_HELD, [], 0),
    "equal margins, error inside": (SD.REPAIR_REPAIRED, [0, 1, 2, 3], 0b100),
    "equal margins, error outside": (SD.REPAIR_FAILED, [0, 1, 2, 3], 0),
    "signed zeros": (SD.REPAIR_REPAIRED, [1, 6], 0b11),
    "length 0": (SD.REPAIR_REPAIRED, [3, 1, 0, 2], 0b1),
    "length 0, all wrong": (SD.REPAIR_REPAIRED, [3, 1, 0, 2], 0b1111),
    "two in one byte": (SD.REPAIR_REPAIRED, [10, 11], 0b11),
    "inside the CRC bytes": (SD.REPAIR_REPAIRED, [37, 35, 36, 34], 0b110),
    "equal penalties": (SD.REPAIR_REPAIRED, [0, 2], 0b1),
    "equal sums": (SD.REPAIR_REPAIRED, [2, 4, 1, 7], 0b101),
    "failed, not a candidate": (SD.REPAIR_FAILED, [0, 1, 2, 3, 4, 5, 6, 7], 0),
    "failed, runner-up wrong": (SD.REPAIR_FAILED, [3], 0),
    "length 255": (SD.REPAIR_REPAIRED, [511, 255, 256, 513, 0], 0b1010),
    "length 254": (SD.REPAIR_REPAIRED, [510, 300, 7], 0b111),
    "length 2": (SD.REPAIR_REPAIRED, [7, 0], 0b11),
}


def test_every_edge_case_has_an_expectation():
    assert {c[0] for c in RC.edge_cases()} == set(EXPECT)


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_tie_rules_and_edges(name):
    case = _by_name(name)
    _n, length, nib, sec, mar, L = case
    status, first, pattern = EXPECT[name]
    for dtype in (np.float32, np.float64):
        new, rec = _run(case, dtype)
        assert (rec["status"], rec["pattern"], rec["changed"]) == (status, pattern, bin(pattern).count("1")), rec
        assert rec["codewords"][:len(first)] == first and len(rec["codewords"]) == rec["candidates"], rec
        syn = SD.syndrome(SD.body_bytes(nib, length + 2), length)
        if status == SD.REPAIR_CRC_HELD:
            assert syn == 0 and new == nib and rec == SD.no_repair(SD.REPAIR_CRC_HELD, dtype)
            continue
        assert rec["syndrome"] == syn != 0 and rec["candidates"] == min(L, len(nib)) and type(rec["penalty"]) is dtype
        if status == SD.REPAIR_FAILED:
            assert new == nib and rec["penalty"] == 0                          # a failed repair leaves every byte alone
        else:
            want = list(nib)
            pen = dtype(0.0)
            for i, c in enumerate(rec["codewords"]):
                if (pattern >> i) & 1:
                    want[c] = sec[c]
                    pen = dtype(pen + dtype(mar[c]))
            assert new == want and SD.syndrome(SD.body_bytes(new, length + 2), length) == 0
            assert rec["penalty"] == pen
    assert nib == list(case[2])                                                # (the input is not written to)


def test_equal_penalties_take_the_smaller_pattern_even_where_it_is_wrong():
    """the CRC's weak tail: the last payload byte and the low CRC byte enter the syndrome alike, so a wrong pattern can hold the CRC"""
    _n, length, nib, sec, mar, L = _by_name("equal penalties")
    new, rec = SD.crc_repair(nib, sec, mar, length + 2, L, np.float32)
    sent = list(nib)
    sent[2] = sec[2]
    assert SD.syndrome(SD.body_bytes(sent, 3), 1) == 0 and new != sent and SD.syndrome(SD.body_bytes(new, 3), 1) == 0
    assert SD.syndrome_effect(0, 5, 1) == SD.syndrome_effect(2, 5, 1) == 5


def test_random_frames_repair_or_fail_consistently():
    repaired = 0
    for case in RC.random_cases():
        _n, length, nib, sec, mar, L = case
        new, rec = _run(case)
        syn = SD.syndrome(SD.body_bytes(nib, length + 2), length)
        assert (rec["status"] == SD.REPAIR_CRC_HELD) == (syn == 0)
        if rec["status"] == SD.REPAIR_REPAIRED:
            assert SD.syndrome(SD.body_bytes(new, length + 2), length) == 0 and new != nib
            assert [c for c in range(len(nib)) if new[c] != nib[c]] == sorted(c for i, c in enumerate(rec["codewords"]) if (rec["pattern"] >> i) & 1)
            repaired += 1
        elif rec["status"] == SD.REPAIR_FAILED:
            assert new == nib
        if syn:
            keys = [(float(mar[c]), c) for c in rec["codewords"]]
            assert len(keys) == min(L, len(nib)) and keys == sorted(keys)
            assert all(k > keys[-1] for k in ((float(mar[c]), c) for c in range(len(nib)) if c not in rec["codewords"]))
    assert repaired >= 40


@functools.lru_cache(None)
def repair_counts(sf, cr, length, n, snr_db, L):
    """(frames right with repair off, right with L candidates, frames REPAIRED, of them to bytes that were not sent), float64, true header positions"""
    cfg, _p, iq, starts, want = SC.gain_stream(sf, cr, length, n, snr_db, valid=True, seed=99)
    down = SD._down(cfg)
    before = after = repaired = wrong = 0
    for hp, w in zip(starts, want):
        b0, r0 = SD.decode_frame(iq, hp, cfg, down=down)
        b1, r1 = SD.decode_frame(iq, hp, cfg, down=down, crc_repair=L)
        before += b0 == w
        after += b1 == w
        assert "repair" not in r0 and (b0 is None or set(r0) == TODAY)        # repair off: today's report, key for key
        assert set(r1) == set(r0) | {"repair"}
        for key in r0:
            if key != "crc_ok":
                assert np.array_equal(r0[key], r1[key]), key                   # every other key: the decision before repair
        st = r1["repair"]["status"]
        if b1 is None or not r1["has_crc"]:
            assert st == SD.REPAIR_NOT_ATTEMPTED and b1 == b0
        elif r0["crc_ok"]:
            assert st == SD.REPAIR_CRC_HELD and b1 == b0 and r1["crc_ok"] == 1
        else:
            assert st in (SD.REPAIR_REPAIRED, SD.REPAIR_FAILED) and r1["crc_ok"] == int(st == SD.REPAIR_REPAIRED) and (b1 != b0) == r1["crc_ok"]
            assert b1[:3] == b0[:3]                                            # the header bytes are never touched
        if st == SD.REPAIR_REPAIRED:
            repaired += 1
            wrong += b1 != w
    return before, after, repaired, wrong


@pytest.mark.parametrize("sf,cr,length,snr_db", [(7, 1, 16, -7.0), (8, 4, 24, -11.5)])
def test_gain(sf, cr, length, snr_db):
    before, after, repaired, wrong = repair_counts(sf, cr, length, 60, snr_db, 8)
    print("SF%d 4/%d %d B %.1f dB: %d of 60 right, %d with repair (L = 8); %d repaired, %d of them to bytes not sent" %
          (sf, 4 + cr, length, snr_db, before, after, repaired, wrong))
    assert after >= before + 10
    assert 4 * wrong <= repaired
