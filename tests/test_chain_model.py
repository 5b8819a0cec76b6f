"""CPU: the bit-level model of the integer decode chain (tests/chain_model.py) against the oracle - its parts against the oracle's exported
primitives, exhaustively, and EVERY crafted frame of case_sets() through oracle.Oracle.run: exactly one frame per packet sent, bytes equal to
chain_decode's.  A condition, not a statistic: a symbol the reference does not decode deterministically is kept out of case_sets() by an input rule
stated in chain_model's docstring, never skipped by outcome.  Then the coverage the case sets claim, computed from the model alone.
tests/test_gpu_chain.py holds the device's five copies of the chain to the same frames."""
import numpy as np
import pytest

import chain_model as M
from gr_lora_amd import synth


def test_tables_are_the_ones_the_kernels_read():
    import os
    a = open(os.path.join(M.ROOT, "oracle", "whitening_data.inc")).read()
    b = open(os.path.join(M.ROOT, "gr_lora_amd", "csrc", "whitening_data.inc")).read()
    assert a == b
    w = M.whitening()
    assert (len(w["HEADER"]), len(w["CR56"]), len(w["CR78"])) == (13, 516, 518)


def test_parts_against_the_oracle_primitives(oracle_mod):
    L = oracle_mod.lib()
    for v in range(256):
        assert M.H84[v] == L.lora_oracle_hamming84_decode(v), v
        assert M.deshuffle(v) == L.lora_oracle_deshuffle_byte(v), v
        assert M.deshuffle(M.shuffle_tx(v)) == v
    for n in range(16):
        assert M.ENC[n] == L.lora_oracle_hamming_encode(n) and M.H84[M.ENC[n]] == n and M.data_bits(M.ENC[n]) == n
        for bit in range(8):                                             # every single-bit error is corrected
            assert M.H84[M.ENC[n] ^ (1 << bit)] == n
    rng = np.random.default_rng(1)
    for size in range(4, 13):
        for count in range(0, 2 * size + 1):
            for bits in [0, 1, (1 << size) - 1, 1 << (size - 1)] + [int(v) for v in rng.integers(0, 1 << size, 8)]:
                assert M.rotl(bits, count, size) == L.lora_oracle_rotl(bits, count, size), (bits, count, size)
    for n_words in range(5, 9):
        for ppm in range(4, 13):
            blocks = [[int(v) for v in rng.integers(0, 1 << ppm, n_words)] for _ in range(24)]
            blocks.append([(1 << ppm) - 1] * n_words)
            blocks += [[(1 << b) if i == j else 0 for i in range(n_words)] for j in range(n_words) for b in range(ppm)]
            for words in blocks:
                arr = np.array(words, dtype=np.uint32)
                out = np.zeros(16, dtype=np.uint8)
                L.lora_oracle_deinterleave(arr.ctypes.data, n_words, ppm, out.ctypes.data)
                got = M.deinterleave(words, ppm)
                assert got == [int(v) for v in out[:ppm]], (n_words, ppm, words)
                assert M.interleave(got, ppm, n_words) == words             # (and the builder's inverse)


def test_symbol_count_is_the_transmit_models():
    for sf in range(7, 13):
        for cr in range(1, 5):
            for rr in (False, True):
                for n in range(0, 258):
                    assert M.payload_symbol_count(n, sf, cr, rr) == synth.payload_symbol_count(n, sf, cr, rr)


def test_valid_frames_decode_to_their_payload():
    """the model on the transmit model's own frames (synth.encode_shifts): the published bytes are the payload's"""
    rng = np.random.default_rng(2)
    for sf, cr, rr in ((7, 1, False), (7, 4, True), (8, 3, False), (9, 2, False), (10, 4, False), (11, 1, True), (12, 3, True)):
        cfg = synth.TxConfig(sf=sf, cr=cr, reduced_rate=rr)
        payload = bytes(rng.integers(0, 256, 23, dtype=np.uint8))
        hs, ps = synth.encode_shifts(payload, cfg)
        n = 1 << sf
        fr = M.Frame(sf, rr, False, [(s - 1) % n for s in hs], [(s - 1) % n for s in ps])
        for cr_prev in (1, 2, 3, 4):
            body, (_, cr_got, nsym, n_left) = fr.decode(cr_prev, 1)          # (demodulator 1: a valid frame may hold the full-rate top word)
            assert body == synth.expected_frame_tail(payload, cfg) and cr_got == cr and nsym == len(ps) and n_left == sf - 7


def oracle_frames(oracle_mod, cfg_kw, dec_kw, frames, demod):
    """(frames behind the loratap header, seconds in the oracle) of one stream"""
    import time
    iq = M.render(frames, synth.TxConfig(**cfg_kw))
    o = oracle_mod.Oracle(**M.decoder_kwargs(dec_kw, demod))
    t = time.perf_counter()
    o.run(iq)
    return [f[15:] for f in o.frames()], time.perf_counter() - t


def _demods_of(name):
    """the demodulators on which some family of tests/test_gpu_chain.py decodes the cell"""
    return sorted({d for cells in M.families().values() for n, d in cells if n == name})


@pytest.mark.parametrize("case_set", ["random_words", "many", "header_bit_errors", "header_fields", "carry", "residues", "longest", "top_word", "implicit"])
def test_every_crafted_frame_through_the_oracle(oracle_mod, case_set):
    import concurrent.futures as cf
    cells = M.cases(case_set + "/")
    assert cells
    jobs = []
    for cell in cells:
        assert _demods_of(cell[0]), cell[0]
        for demod in _demods_of(cell[0]):
            jobs += [(cell, demod, s, frames) for s, frames in M.streams_for(cell, demod)]

    def one(job):
        (name, cfg_kw, dec_kw, _), demod, s, frames = job
        return oracle_frames(oracle_mod, cfg_kw, dec_kw, frames, demod)
    with cf.ThreadPoolExecutor(8) as ex:
        results = list(ex.map(one, jobs))
    n, seconds = 0, 0.0
    for ((name, cfg_kw, dec_kw, _), demod, s, frames), (got, t) in zip(jobs, results):
        want = M.expect(frames, dec_kw, demod)
        assert len(got) == len(frames), (name, s, demod, len(got), len(frames))
        assert got == want, (name, s, demod, [f.note for f in frames], [g.hex() for g in got], [w.hex() for w in want])
        n += len(frames)
        seconds += t
    print("%s: %d cells, %d stream decodes, %d frames, %.1f s in the oracle (summed over threads)" % (case_set, len(cells), len(jobs), n, seconds))


def _traces(prefix, **where):
    out = []
    for name, cfg_kw, dec_kw, streams in M.cases(prefix, **where):
        for frames in streams:
            tr = []
            M.expect(frames, dec_kw, dec_kw["demods"][-1], tr)
            out += [(name, fr, t) for fr, t in zip(frames, tr)]
    return out


def test_coverage_random_words_reach_every_byte_value():
    lo = set()
    for name, _, dec_kw, _ in M.cases("random_words/"):
        seen = {c: set() for c in range(5)}
        count = {c: 0 for c in range(5)}
        for _, _, t in _traces(name):
            for cr, w in t["fec_in"].items():
                seen[cr].update(w)
                count[cr] += len(w)
        lo |= seen[1] | seen[2]
        if dec_kw["sf"] <= 9:
            assert count[1] + count[2] >= 300 and count[3] + count[4] >= 300, (name, count)
            if not dec_kw["reduced_rate"]:                               # every entry of the Hamming table, in every SF7-SF9 cell
                assert len(seen[3] | seen[4]) == 256, (name, len(seen[3] | seen[4]))
    assert len(lo) == 256                                                # (CR 1 / 2: eight-bit codewords only among the header's spare ones)


def test_coverage_header_bit_errors():
    for name in ("header_bit_errors/sf7_cr4", "header_bit_errors/sf7_cr1"):
        clean = [M.ENC[n] for n in (M.FIXED_FIELDS[0] >> 4, M.FIXED_FIELDS[0] & 15, (M.FIXED_FIELDS[1] << 1) | M.FIXED_FIELDS[2], M.FIXED_FIELDS[3], M.FIXED_FIELDS[4])]
        seen = {i: set() for i in range(5)}
        differ = agree = 0
        for _, fr, t in _traces(name):
            err = [a ^ b for a, b in zip(t["hdr_fec_in"], clean)]
            assert sum(1 for e in err if e) == 1
            i = [k for k, e in enumerate(err) if e][0]
            seen[i].add(err[i])
            a, b = t["hdr_classes"]
            differ += a != b
            agree += a == b
        for i in range(5):
            assert seen[i] == set(M.PATTERNS), (name, i)
        assert len(M.PATTERNS) == 36 and sum(bin(p).count("1") == 1 for p in M.PATTERNS) == 8
        assert differ >= 1 and agree >= 1, (name, differ, agree)
    # every other cell: all 36 patterns on at least one codeword between its two constructor CRs' cells, every codeword index under CR 4
    for cell in M.cases("header_bit_errors/", cr=4):
        if cell[2]["sf"] > 10 or cell[0].endswith("sf7_cr4"):
            continue
        idx, pats = set(), set()
        for _, fr, t in _traces(cell[0]):
            i, m = fr.note[2:].split("^")
            idx.add(int(i))
            pats.add(int(m, 16))
        assert idx == set(range(5)) and pats == set(M.PATTERNS), cell[0]


def test_coverage_residues_and_the_wrap():
    for sf in (7, 9, 11):
        n = 1 << sf
        hdr, pay, wraps = set(), set(), set()
        for name, fr, t in _traces("residues/", sf=sf):
            hdr.update(b % 4 for b in fr.hdr_bins)
            wraps.update(b for b in fr.hdr_bins if b >= n - 2)
            if fr.reduced_rate:
                pay.update(b % 4 for b in fr.pay_bins)
                wraps.update(b + n for b in fr.pay_bins if b >= n - 2)
        assert hdr == {0, 1, 2, 3} and pay == {0, 1, 2, 3}, (sf, hdr, pay)
        assert wraps == {n - 2, n - 1, 2 * n - 2, 2 * n - 1}, (sf, wraps)      # both wrapping bins, in header and in payload symbols
    for sf in (8, 10):                                                         # (full rate: the header symbols)
        hdr = set()
        for name, fr, t in _traces("residues/", sf=sf):
            hdr.update(b % 4 for b in fr.hdr_bins)
        assert hdr == {0, 1, 2, 3}


def test_coverage_longest_walks_past_the_whitening_tables():
    n56 = max(t["n_cw"] for _, _, t in _traces("longest/") if t["cr"] <= 2)
    n78 = max(t["n_cw"] for _, _, t in _traces("longest/") if t["cr"] >= 3)
    assert n56 > 516 and n78 > 518, (n56, n78)
    for _, fr, t in _traces("longest/"):
        body, _ = fr.decode(4)
        assert len(body) == 3 + 257 and body[0] == 255


def test_coverage_header_fields_and_carry():
    seen = set()
    for name, fr, t in _traces("header_fields/sf7_cr4"):
        body, (phdr, cr, nsym, _) = fr.decode(t["cr_prev"])
        raw = M.header_bytes(M.deinterleave(fr.words(2)[0], 5)[:5], t["cr_prev"])
        seen.add((raw[1] >> 5, (raw[1] >> 4) & 1, raw[0]))
        assert cr == min(raw[1] >> 5, 4)
    for cr_field in range(8):
        for crc_bit in (0, 1):
            for length in (0, 1, 2, 255):
                assert (cr_field, crc_bit, length) in seen, (cr_field, crc_bit, length)
            for length in M.block_edges(7, min(cr_field, 4), False):
                assert cr_field == 0 or (cr_field, crc_bit, length) in seen, (cr_field, crc_bit, length)
    for cell in M.cases("header_fields/"):
        tr = _traces(cell[0])
        assert any(t["cr_prev"] == 0 and t is not tr[0][2] for _, _, t in tr), cell[0]           # a packet behind a CR-0 header
        nsyms = [fr.decode(t["cr_prev"])[1][2] for _, fr, t in tr]
        assert 0 in nsyms, cell[0]                                                                   # d_payload_symbols <= 0: one symbol, no block
    for cell in M.cases("carry/"):
        for frames in cell[3]:
            tr = []
            M.expect(frames, cell[2], 2, tr)
            assert [t["cr"] for t in tr] == [1, 4, 2, 3], cell[0]
            for t in tr:
                a, b = t["hdr_classes"]
                assert a != b, cell[0]


def test_frame_counts_per_case_set():
    """the figures the summary quotes"""
    tot = {}
    for name, _, _, streams in M.case_sets():
        tot[name.split("/")[0]] = tot.get(name.split("/")[0], 0) + sum(len(s) for s in streams)
    print(tot, sum(tot.values()))
    assert all(v > 0 for v in tot.values())
