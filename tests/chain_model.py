"""The integer decode chain as a bit-level model, and crafted frames that carry arbitrary words into it.

Once a symbol's bin is known, everything up to the published frame is integer work: the reduced-rate rounding, the gray word, the block
de-interleaver, the de-shuffle, de-whitening, Hamming(8,4) or the data-bit extraction, the header parse and the frame bytes.  The device has five
separately written copies of that chain ("The integer decode chain"); `chain_decode` is its definition in plain Python, written from
the reference's lib/decoder_impl.cc:506-565, 567-706 and 826-886 and from nothing in gr_lora_amd/csrc or oracle/lora_oracle.c.  The whitening
sequences are data, read from oracle/whitening_data.inc.

`craft_frame` builds the shifts of a frame whose symbols are *anything*: random words, header codewords with bit errors, every value of the
header fields, symbols off the reduced-rate grid.  `synth.modulate_frame` puts them on a clean signal, where every demodulator returns them
exactly, so the ordinary entry points of the oracle and of the device carry them into the chain.  `case_sets()` is the one list of such frames that
tests/test_chain_model.py (CPU: oracle against this model) and tests/test_gpu_chain.py (device against both) share.

Input rules (symbols that are never sent, each with its reason):

* the full-rate word 1 << (sf - 1) - gray of bin N - 1, on air as shift 0, an unshifted upchirp - is never drawn at random.  The compat FFT
  demodulator (2) pins shift 0 to bin 0, the plain FFT demodulator (1) returns N - 1, and the gradient demodulator (0) has no frequency step to find in
  such a symbol: its answer is an accident of rounding.  The word is sent in the named `top_word` cases only, which run on demodulators 1 and 2.
* shift 0 is kept out of header and reduced-rate symbols as well where the gradient demodulator decodes them (bin N - 1 there rounds to N / 4 and
  wraps to 0 whatever the FFT demodulators make of it, but the gradient demodulator's bin is again an accident): the residue cases that send bin
  N - 1 run on demodulators 1 and 2; bin N - 2 wraps the same way and runs everywhere.
* at decimation 2 and 4 the top word goes to demodulator 1 only: demodulator 2 pins its bin to 0, fine_sync is then fed a bin the symbol does not
  have and moves the symbol clock by a sample - an eighth of a bin at decimation 8, half a bin at decimation 2, where every symbol behind it sits on
  a tie between two bins.
* a frame goes to the gradient demodulator only if its first header symbol is decidable with the window one sample off (Frame.gradient_safe): the
  decoder's clock reaches that symbol up to a sample early or late, and the phase step between two symbols inside the window can outweigh the
  symbol's own frequency drop.  The builders draw the header's two free nibbles until the rule holds; where a case fixes them (bit errors, residues,
  top word) the streams that break it go to demodulators 1 and 2 only (streams_for).
* a frame sends exactly the symbols the decoder will take (its header as decoded under the carried CR decides), followed by silence: symbols behind
  the end of a frame would be scanned as a new preamble.
"""
from __future__ import annotations

import functools
import os
import re
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- tables ------------------------------------------------------------------------------------------------------------------------------------
SHUFFLE = (5, 0, 1, 2, 4, 3, 6, 7)      # decode(): out bit j = in bit SHUFFLE[j] (:568, :611-621)
DATA_IDX = (1, 2, 3, 5)                 # extract_data_only (:694)


@functools.lru_cache(None)
def whitening() -> Dict[str, Tuple[int, ...]]:
    src = open(os.path.join(ROOT, "oracle", "whitening_data.inc")).read()
    out = {}
    for name in ("HEADER", "CR56", "CR78"):
        m = re.search(r"LORA_WHITEN_%s\[(\d+)\]\s*=\s*\{([^}]*)\}" % name, src)
        v = tuple(int(x, 16) for x in re.findall(r"0x[0-9a-fA-F]+", m.group(2)))
        assert len(v) == int(m.group(1))
        out[name] = v
    return out


def hamming_encode(n: int) -> int:
    """include/lora/utilities.h:257-264"""
    b0, b1, b2, b3 = n & 1, (n >> 1) & 1, (n >> 2) & 1, (n >> 3) & 1
    return (b1 ^ b2 ^ b3) | (b0 << 1) | (b1 << 2) | (b2 << 3) | ((b0 ^ b1 ^ b2) << 4) | (b3 << 5) | ((b0 ^ b1 ^ b3) << 6) | ((b0 ^ b2 ^ b3) << 7)


ENC = tuple(hamming_encode(n) for n in range(16))


def hamming84_decode(cw: int) -> int:
    """fec_decode(HAMMING84): the nearest codeword; among equally near ones the lowest symbol"""
    return min(range(16), key=lambda s: (bin(cw ^ ENC[s]).count("1"), s))


H84 = tuple(hamming84_decode(c) for c in range(256))


def data_bits(cw: int) -> int:
    return sum(((cw >> p) & 1) << j for j, p in enumerate(DATA_IDX))


def deshuffle(v: int) -> int:
    return sum(((v >> p) & 1) << j for j, p in enumerate(SHUFFLE))


def shuffle_tx(v: int) -> int:
    """the transmitter's side of deshuffle"""
    return sum(((v >> j) & 1) << p for j, p in enumerate(SHUFFLE))


def rotl(bits: int, count: int, size: int) -> int:
    """include/lora/utilities.h:96-103"""
    mask = (1 << size) - 1
    count %= size
    bits &= mask
    return ((bits << count) & mask) | (bits >> (size - count))


def gray(b: int) -> int:
    return b ^ (b >> 1)


def gray_inverse(w: int) -> int:
    b = 0
    while w:
        b ^= w
        w >>= 1
    return b


def deinterleave(words: Sequence[int], ppm: int) -> List[int]:
    """:535-565: len(words) words of ppm bits -> ppm codewords, bit i of codeword x = bit x of word i rotated left by i"""
    out = [0] * ppm
    for i, w in enumerate(words):
        r = rotl(w, i, ppm)
        for x in range(ppm):
            out[x] |= ((r >> x) & 1) << i
    return out


def interleave(codewords: Sequence[int], ppm: int, n_words: int) -> List[int]:
    """the transmitter's side of deinterleave: ppm codewords -> n_words words (codeword bits above n_words are lost)"""
    words = []
    for i in range(n_words):
        r = sum(((codewords[x] >> i) & 1) << x for x in range(ppm))
        words.append(rotl(r, ppm - (i % ppm), ppm))
    return words


def reduce_bin(b: int, sf: int) -> int:
    """:507-509: std::lround(bin / 4.0f) % (N / 4) - halves round away from zero"""
    return ((b + 2) // 4) % (1 << (sf - 2))


def bins_to_words(bins: Sequence[int], sf: int, reduced: bool, demod: int = 2) -> List[int]:
    """demodulate() behind the bin (:506-512).  `bins` are the gradient demodulator's: shift - 1 mod N.  Shift 0 is bin N - 1 for the plain FFT
    demodulator and pinned to bin 0 by demodulators 0 and 2."""
    n = 1 << sf
    out = []
    for b in bins:
        if b == n - 1 and demod != 1:
            b = 0
        out.append(gray(reduce_bin(b, sf) if reduced else b))
    return out


def payload_symbol_count(payload_length: int, sf: int, cr: int, reduced_rate: bool) -> int:
    """:842-847, in float32 as there"""
    f = np.float32
    spb = cr + 4
    bits_needed = f(payload_length) * f(8.0)
    symbols_needed = bits_needed * (f(spb) / f(4.0)) / f(sf - (2 if reduced_rate else 0))
    return int(np.ceil(symbols_needed / f(spb))) * spb


def header_bytes(cw5: Sequence[int], cr: int) -> List[int]:
    """decode(true) (:567-586): the five header codewords and one zero byte (:633), under the FEC class of the CR the decoder carries"""
    w = [deshuffle(c) ^ p for c, p in zip(cw5, whitening()["HEADER"])] + [whitening()["HEADER"][5]]
    if cr >= 3:
        return [(H84[w[2 * k]] << 4) | H84[w[2 * k + 1]] for k in range(3)]
    if cr >= 1:
        return [(data_bits(w[2 * k]) << 4) | data_bits(w[2 * k + 1]) for k in range(3)]
    return [0, 0, 0]                    # no switch case for CR 0 (:655): d_decoded stays empty, read as zeros


def payload_bytes(cws: Sequence[int], cr: int, trace: Optional[dict] = None) -> List[int]:
    """decode(false): de-shuffle, de-whiten (0 past the table's end), Hamming or data bits, low nibble first"""
    prng = whitening()["CR56" if cr <= 2 else "CR78"]
    w = [deshuffle(c) ^ (prng[i] if i < len(prng) else 0) for i, c in enumerate(cws)]
    if trace is not None:
        trace.setdefault("fec_in", {}).setdefault(cr, []).extend(w)
        trace["n_cw"] = len(w)
    if cr >= 3:
        n = int(np.ceil(np.float32(len(w)) * np.float32(4.0) / (np.float32(4.0) + np.float32(cr))))   # :658
        at = lambda i: H84[w[i]] if i < len(w) else H84[0]
    elif cr >= 1:
        n = (len(w) + 1) // 2
        at = lambda i: data_bits(w[i]) if i < len(w) else 0
    else:
        return []
    return [(at(2 * k + 1) << 4) | at(2 * k) for k in range(n)]


def chain_decode(hdr_words: Sequence[int], pay_words: Sequence[int], sf: int, cr_prev: int, reduced_rate: bool, implicit: bool = False,
                 demod: int = 2, crc: bool = True, trace: Optional[dict] = None):
    """One packet through the chain: (bytes behind the 15-byte loratap header, (phdr, cr, payload_symbols, n_left)).

    hdr_words: the 8 words of the header block (sf - 2 bits).  pay_words: the payload symbols' words as demodulate() forms them, sf bits or, at
    the reduced rate, sf - 2; the decoder takes as many as the header asks for (one, and no block, where d_payload_symbols <= 0), the implicit-header
    decoder all of them.  cr_prev: d_phdr.cr on entry - the constructor's, or what the packet before left.  At the full rate demodulators 0 and 2
    never return bin N - 1: its word, 1 << (sf - 1), reads as 0."""
    assert len(hdr_words) == 8
    first = deinterleave(hdr_words, sf - 2)
    ppm = sf - 2 if reduced_rate else sf
    if not reduced_rate and demod != 1:
        pay_words = [0 if w == 1 << (sf - 1) else w for w in pay_words]
    if implicit:
        phdr = [0, ((cr_prev & 7) << 5) | (int(bool(crc)) << 4), 0]
        cr, payload_symbols, cws = cr_prev, 1, list(first)
        n_left = len(cws)
        spb = 4 + cr
        for b in range(len(pay_words) // spb):                           # (a block cut short by the end of the signal is dropped)
            cws += deinterleave(pay_words[b * spb:(b + 1) * spb], ppm)
        payload_length = len(cws) // 2                                   # :864
    else:
        phdr = header_bytes(first[:5], cr_prev)
        if trace is not None:
            trace["hdr_fec_in"] = [deshuffle(c) for c in first[:5]]
            trace["hdr_classes"] = (header_bytes(first[:5], 4), header_bytes(first[:5], 1))
        if (phdr[1] >> 5) > 4:                                           # :834-835
            phdr[1] = (phdr[1] & 0x1f) | (4 << 5)
        cr = phdr[1] >> 5
        payload_length = phdr[0] + 2 * ((phdr[1] >> 4) & 1)             # :838
        payload_symbols = payload_symbol_count(payload_length, sf, cr, reduced_rate)
        cws = list(first[5:])                                            # the spare codewords stay in d_demodulated (:632)
        n_left = len(cws)
        spb = 4 + cr
        if payload_symbols > 0:
            assert len(pay_words) >= payload_symbols, (len(pay_words), payload_symbols)
            for b in range(payload_symbols // spb):
                cws += deinterleave(pay_words[b * spb:(b + 1) * spb], ppm)
    dec = payload_bytes(cws, cr, trace)
    assert payload_length <= 257 or implicit                             # length + CRC of an explicit header: the cap of a published payload
    body = [dec[i] if i < len(dec) else 0 for i in range(payload_length)]
    return bytes(phdr + body), (bytes(phdr), cr, payload_symbols, n_left)


def symbols_taken(payload_symbols: int) -> int:
    return payload_symbols if payload_symbols > 0 else 1


# ---- the frame builder --------------------------------------------------------------------------------------------------------------------------
@dataclass
class Frame:
    sf: int
    reduced_rate: bool
    implicit: bool
    hdr_bins: List[int]                 # the bins the decoder demodulates (gradient convention: shift - 1 mod N)
    pay_bins: List[int]
    note: str = ""
    decim: int = 8

    def shifts(self) -> Tuple[List[int], List[int]]:
        n = 1 << self.sf
        return [(b + 1) % n for b in self.hdr_bins], [(b + 1) % n for b in self.pay_bins]

    def words(self, demod: int) -> Tuple[List[int], List[int]]:
        return bins_to_words(self.hdr_bins, self.sf, True, demod), bins_to_words(self.pay_bins, self.sf, self.reduced_rate, demod)

    def decode(self, cr_prev: int, demod: int = 2, crc: bool = True, trace: Optional[dict] = None):
        h, p = self.words(demod)
        return chain_decode(h, p, self.sf, cr_prev, self.reduced_rate, self.implicit, demod, crc, trace)


    def gradient_safe(self) -> bool:
        """The input rule for the gradient demodulator (0).  The decoder's clock may reach the first header symbol one sample early or late
        (fine_sync puts it right from there on), and a window one sample off holds the phase step between two symbols: one or two samples of
        instantaneous frequency of any value, which can outweigh the symbol's own frequency drop (max_frequency_gradient_idx keeps the largest
        drop between D-sample averages, :466-491).  A frame goes to demodulator 0 only where, in float64 and for the window one sample early, exact
        and one sample late, the first header symbol's own drop is the largest of the window by 0.15 rad and lands on the bin sent."""
        n, d = 1 << self.sf, self.decim
        sps = n * d
        k = np.arange(sps, dtype=np.float64)
        cyc = (k * k / (2.0 * d * d * n) - k / (2.0 * d)) % 1.0             # the base upchirp's phase in cycles (synth.base_upchirp)
        up = np.exp(2j * np.pi * cyc)
        sym = lambda b: up[(np.arange(sps) + ((b + 1) % n) * d) % sps]
        seq = np.concatenate([np.conj(up[:sps // 4]), sym(self.hdr_bins[0]), sym(self.hdr_bins[1])])
        for off in (-1, 0, 1):
            w = seq[sps // 4 + off:sps // 4 + off + sps]
            f = np.angle(w[1:] * np.conj(w[:-1]))
            avg = np.append(f, f[-1]).reshape(n, d).mean(axis=1)
            g = avg[:-1] - avg[1:]
            top = int(np.argmax(g))
            rest = np.delete(g, [i for i in (top - 1, top, top + 1) if 0 <= i < g.size])
            if reduce_bin((n - (top + 2)) % n, self.sf) != reduce_bin(self.hdr_bins[0], self.sf) or g[top] - rest.max() < 0.15:
                return False
        return True


def _reduced_bin(word: int, r: int, sf: int) -> int:
    """a bin 4 g + r (r in 0..3) that the reduced-rate rounding brings to `word`: residues 2 and 3 round up, so they sit under the next g -
    for word 0 that is the wrap at bins N - 2 and N - 1"""
    g = gray_inverse(word)
    if r >= 2:
        g = (g - 1) % (1 << (sf - 2))
    return 4 * g + r


def header_codewords(fields, spare: Sequence[int], sf: int, xor: Sequence[Tuple[int, int]] = ()) -> List[int]:
    """the sf - 2 codewords of an explicit header block as they sit in d_demodulated: fields = (length, cr_field 0..7, crc_bit, nibble3, nibble4);
    spare: the sf - 7 codewords behind the header's five, of any value; xor: (codeword index, mask) in the Hamming domain (bit errors on air)"""
    length, cr_field, crc_bit, n3, n4 = fields
    hn = [length >> 4, length & 15, ((cr_field & 7) << 1) | (crc_bit & 1), n3 & 15, n4 & 15]
    pre = [ENC[n] ^ whitening()["HEADER"][i] for i, n in enumerate(hn)]
    for i, m in xor:
        pre[i] ^= m
    assert len(spare) == sf - 7
    return [shuffle_tx(c) for c in pre] + [int(s) & 0xff for s in spare]


def craft_frame(sf: int, cr_prev: int, reduced_rate: bool = False, *, implicit: bool = False, demod: int = 2, hdr_words: Optional[Sequence[int]] = None,
                fields=None, spare: Optional[Sequence[int]] = None, hdr_xor: Sequence[Tuple[int, int]] = (), pay_words: Optional[Sequence[int]] = None,
                rng: Optional[np.random.Generator] = None, n_pay: Optional[int] = None, hdr_res: Optional[Sequence[int]] = None,
                pay_res: Optional[Sequence[int]] = None, top_at: Sequence[int] = (), note: str = "", decim: int = 8) -> Frame:
    """A frame from explicit header words, or from header fields (+ spare codewords, + bit errors), and from explicit payload words or a draw from
    `rng`.  The header is decoded by the model under `cr_prev` to learn how many payload symbols the decoder will take; exactly those are sent
    (`n_pay`: for an implicit header, whose end is the end of the signal).  hdr_res / pay_res: residues r in 0..3 of header and reduced-rate symbols
    (sent at bin 4 g + r).  top_at: payload positions set to the full-rate top word (named cases only)."""
    n = 1 << sf
    ppm_h, ppm = sf - 2, (sf - 2 if reduced_rate else sf)
    if hdr_words is None:
        if fields is not None:
            if spare is None:
                spare = [int(v) for v in rng.integers(0, 256, sf - 7)]
            cws = header_codewords(fields, spare, sf, hdr_xor)
        else:                                                             # an implicit header's first block: any codewords
            cws = [int(v) for v in rng.integers(0, 256, ppm_h)]
        hdr_words = interleave(cws, ppm_h, 8)
    hdr_words = [int(w) for w in hdr_words]
    assert len(hdr_words) == 8 and all(0 <= w < 1 << ppm_h for w in hdr_words)
    hdr_res = list(hdr_res) if hdr_res is not None else [0] * 8
    hdr_bins = [_reduced_bin(w, r, sf) for w, r in zip(hdr_words, hdr_res)]
    if implicit:
        want = int(n_pay)
    else:
        _, (_, _, payload_symbols, _) = chain_decode(hdr_words, [0] * 4096, sf, cr_prev, reduced_rate, False, demod)
        want = symbols_taken(payload_symbols)
    if pay_words is None:
        top = 1 << (sf - 1)
        pay_words = []
        while len(pay_words) < want:
            w = int(rng.integers(0, 1 << ppm))
            if reduced_rate or w != top:                                  # the input rule on the full-rate top word
                pay_words.append(w)
    pay_words = [int(w) for w in pay_words]
    assert len(pay_words) == want, (len(pay_words), want)
    for p in top_at:
        assert not reduced_rate
        pay_words[p] = 1 << (sf - 1)
    if reduced_rate:
        pay_res = list(pay_res) if pay_res is not None else [0] * want
        pay_bins = [_reduced_bin(w, r, sf) for w, r in zip(pay_words, pay_res)]
    else:
        pay_bins = [gray_inverse(w) for w in pay_words]
    fr = Frame(sf, reduced_rate, implicit, hdr_bins, pay_bins, note, decim)
    assert fr.words(1) == (hdr_words, pay_words) and all(0 <= b < n for b in hdr_bins + pay_bins)
    return fr


def render(frames: Sequence[Frame], cfg, lead: float = 1.37, gap: float = 3.29, tail: float = 3.0) -> np.ndarray:
    """the stream's samples: silence, frame, silence, ... (leads and gaps off the symbol grid, as real captures are)"""
    from gr_lora_amd import synth
    sps = cfg.sps
    pieces = []
    for i, fr in enumerate(frames):
        pieces.append(np.zeros(int((lead if i == 0 else gap + 0.61 * (i % 3)) * sps), dtype=np.complex64))
        pieces.append(synth.modulate_frame(*fr.shifts(), cfg))
    pieces.append(np.zeros(int(tail * sps), dtype=np.complex64))
    return np.concatenate(pieces)


def expect(frames: Sequence[Frame], dec_kw: dict, demod: int, traces: Optional[list] = None) -> List[bytes]:
    """the model's frames of one stream: d_phdr.cr starts as the constructor's and is carried from packet to packet"""
    cr, out = dec_kw.get("cr", 4), []
    for fr in frames:
        t = {} if traces is not None else None
        body, (_, cr_next, _, _) = fr.decode(cr, demod, dec_kw.get("crc", True), t)
        if traces is not None:
            t["cr_prev"], t["cr"] = cr, cr_next
            traces.append(t)
        if not fr.implicit:
            cr = cr_next
        out.append(body)
    return out


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------
RATES = {8: 1e6, 4: 5e5, 2: 2.5e5}
PATTERNS = [1 << a for a in range(8)] + [(1 << a) | (1 << b) for a in range(8) for b in range(a + 1, 8)]   # 8 one-bit + 28 two-bit masks
FIXED_FIELDS = (5, 4, 1, 0x2, 0x8)     # the fixed header of the bit-error cases: length 5, CR 4, CRC


def _seed(*parts) -> np.random.Generator:
    h = 0
    for p in parts:
        for ch in str(p):
            h = (h * 131 + ord(ch)) % (1 << 61)
    return np.random.default_rng(h)


def _chain(sf, ctor_cr, reduced, specs, demod=2, decim=8) -> List[Frame]:
    """a stream: craft_frame for every spec in turn with the CR the model says the decoder carries.  Fields whose two free nibbles are None get
    them drawn from the spec's rng until the frame may go to the gradient demodulator (Frame.gradient_safe)."""
    cr, out = ctor_cr, []
    for kw in specs:
        kw = dict(kw)
        fields = kw.get("fields")
        if fields is not None and fields[3] is None:
            nrng = _seed("nibbles", sf, decim, reduced, fields, len(out))
            for _ in range(64):
                kw["fields"] = tuple(fields[:3]) + (int(nrng.integers(16)), int(nrng.integers(16)))
                state = kw["rng"].bit_generator.state
                fr = craft_frame(sf, cr, reduced, demod=demod, decim=decim, **kw)
                if fr.gradient_safe():
                    break
                kw["rng"].bit_generator.state = state                     # (the same payload draw behind the next pair of nibbles)
            else:
                raise AssertionError("no gradient-safe header for %r" % (fields,))
        else:
            fr = craft_frame(sf, cr, reduced, demod=demod, decim=decim, **kw)
        _, (_, cr, _, _) = fr.decode(cr, demod)
        out.append(fr)
    return out


def streams_for(cell, demod: int) -> List[Tuple[int, List[Frame]]]:
    """(index, stream) of the cell's streams that may go to `demod`: all of them, but for demodulator 0 those whose frames are all gradient_safe"""
    return [(i, fr) for i, fr in enumerate(cell[3]) if demod != 0 or all(f.gradient_safe() for f in fr)]


def _len_for(sf, cr, reduced, n_cw) -> int:
    """the shortest length (with CRC) whose payload holds at least n_cw codewords"""
    for length in range(0, 256):
        if payload_symbol_count(length + 2, sf, cr, reduced) // (4 + cr) * (sf - 2 if reduced else sf) >= n_cw:
            return length
    return 255


def block_edges(sf, cr, reduced, upto=40) -> List[int]:
    """payload lengths (no CRC) on either side of every change of blocks_needed, up to `upto` bytes"""
    out = set()
    for length in range(1, upto + 1):
        if payload_symbol_count(length, sf, cr, reduced) != payload_symbol_count(length - 1, sf, cr, reduced):
            out.update((length - 1, length))
    return sorted(out)


def _cell(name, sf, ctor_cr, streams, reduced=False, decim=8, implicit=False, crc=True, demods=(0, 1, 2)):
    cfg_kw = dict(sf=sf, cr=ctor_cr if 1 <= ctor_cr <= 4 else 4, samp_rate=RATES[decim], reduced_rate=reduced, implicit=implicit, crc=crc)
    dec_kw = dict(sf=sf, cr=ctor_cr, samp_rate=RATES[decim], reduced_rate=reduced, implicit=implicit, crc=crc, demods=tuple(demods))
    return (name, cfg_kw, dec_kw, streams)


def _all_values_spec(sf, reduced, rng) -> dict:
    """a CR 4 packet whose codewords, as they reach the Hamming step (de-shuffled and de-whitened), run through all 256 byte values"""
    ppm, n_left, prng = (sf - 2 if reduced else sf), sf - 7, whitening()["CR78"]
    length = _len_for(sf, 4, reduced, 256)
    n_cw = payload_symbol_count(length + 2, sf, 4, reduced) // 8 * ppm
    while True:
        vals = [int(v) for v in rng.permutation(256)] + [int(v) for v in rng.integers(0, 256, n_cw - 256)]
        cws = [shuffle_tx(v ^ (prng[n_left + i] if n_left + i < len(prng) else 0)) for i, v in enumerate(vals)]
        words = [w for b in range(n_cw // ppm) for w in interleave(cws[b * ppm:(b + 1) * ppm], ppm, 8)]
        if reduced or (1 << (sf - 1)) not in words:                      # (the input rule on the full-rate top word)
            return dict(fields=(length, 4, 1, None, None), pay_words=words, rng=rng, note="all values")


def _spare_values_specs(sf, rng) -> List[dict]:
    """short CR 1 packets whose spare header codewords - the only codewords of a CR 1 / 2 payload that carry eight bits - run through all 256 values
    as they reach the data-bit extraction"""
    n_left, prng = sf - 7, whitening()["CR56"]
    specs = []
    for f in range(-(-256 // n_left)):
        vals = [(f * n_left + j) % 256 for j in range(n_left)]
        specs.append(dict(fields=(2, 1, 0, None, None), spare=[shuffle_tx(v ^ prng[j]) for j, v in enumerate(vals)], rng=rng, note="spare values"))
    return specs


def _random_words(sf, reduced, decim, n_cw, crs=(1, 4, 2, 3), all_values=False, spare_values=False, tag="") -> tuple:
    """a stream of packets with valid headers, CR fields `crs` (an order that alternates the classes), each long enough for n_cw codewords of
    payload drawn uniformly; all_values: a second stream, one CR 4 packet with every byte value at the Hamming step; spare_values: streams of short
    CR 1 packets with every byte value in the spare header codewords"""
    rng = _seed("random_words", sf, reduced, decim, tag)
    specs = [dict(fields=(_len_for(sf, cr, reduced, n_cw), cr, 1, None, None), rng=rng) for cr in crs]
    streams = [_chain(sf, 4, reduced, specs, decim=decim)]
    if all_values:
        streams.append(_chain(sf, 4, reduced, [_all_values_spec(sf, reduced, rng)], decim=decim))
    if spare_values:
        sv = _spare_values_specs(sf, rng)
        streams += [_chain(sf, 4, reduced, sv[k:k + 16], decim=decim) for k in range(0, len(sv), 16)]
    return _cell("random_words/sf%d%s%s%s" % (sf, "r" if reduced else "", "_d%d" % decim if decim != 8 else "", tag), sf, 4, streams, reduced, decim)


def _bit_errors(sf, ctor_cr, which, decim=8, tag="") -> tuple:
    """single-packet streams: the fixed header with mask PATTERNS[p] on codeword i for every (i, p) of `which`; short payload"""
    rng = _seed("header_bit_errors", sf, ctor_cr, decim, tag)
    for _ in range(64):                                                   # spare codewords with which the header WITHOUT errors is gradient_safe
        spare = [int(v) for v in rng.integers(0, 256, sf - 7)]
        if craft_frame(sf, ctor_cr, False, fields=FIXED_FIELDS, spare=spare, rng=_seed(0), decim=decim).gradient_safe():
            break
    else:
        raise AssertionError("fixed header")
    streams = [_chain(sf, ctor_cr, False, [dict(fields=FIXED_FIELDS, spare=spare, hdr_xor=[(i, PATTERNS[p])], rng=rng, note="cw%d^%02x" % (i, PATTERNS[p]))], decim=decim)
               for i, p in which]
    return _cell("header_bit_errors/sf%d%s_cr%d%s" % (sf, "_d%d" % decim if decim != 8 else "", ctor_cr, tag), sf, ctor_cr, streams, False, decim)


def _spread(k: int) -> List[Tuple[int, int]]:
    """all 36 patterns, pattern p on codeword (p + k) mod 5: every pattern once and every codeword index"""
    return [((p + k) % 5, p) for p in range(36)]


def _header_fields(sf, ctor_cr, reduced=False, decim=8, full=True, long_all=False, cr_fields=range(8), full_crc=(0, 1)) -> tuple:
    """CR field 0..7 x CRC bit x lengths 0, 1, 2 and (full) the lengths on either side of every change of blocks_needed up to 40 bytes; length 255
    for every CR field and CRC bit (long_all) or once per FEC class"""
    rng = _seed("header_fields", sf, ctor_cr, reduced, decim)
    nib = lambda: (None, None)
    streams = []
    for cr_field in cr_fields:
        lengths = sorted(set([0, 1, 2] + (block_edges(sf, min(cr_field, 4), reduced) if full else [])))
        if long_all:
            lengths.append(255)
        for crc_bit in (0, 1):
            specs = [dict(fields=(length, cr_field, crc_bit) + nib(), rng=rng) for length in lengths if crc_bit in full_crc or length in (0, 1, 2, 255)]
            if cr_field == 0:                                             # a CR-0 header ends the stream's headers for good: one per stream
                streams += [_chain(sf, ctor_cr, reduced, [s], decim=decim) for s in specs if s["fields"][0] in (0, 1, 2, 255)]
            else:                                                         # (the packets behind the first meet this CR field's class as the carried one)
                streams.append(_chain(sf, ctor_cr, reduced, specs, decim=decim))
    if not long_all:
        streams.append(_chain(sf, ctor_cr, reduced, [dict(fields=(255, 2, 0, None, None), rng=rng)], decim=decim))
        streams.append(_chain(sf, ctor_cr, reduced, [dict(fields=(255, 3, 1, None, None), rng=rng)], decim=decim))
    # length 0 without CRC immediately followed by a second packet (one symbol taken, no block); a CR-0 header followed by two more packets:
    # d_phdr.cr stays 0 and their headers read as zeros
    streams.append(_chain(sf, ctor_cr, reduced, [dict(fields=(0, 2, 0, None, None), rng=rng), dict(fields=(7, 3, 1, None, None), rng=rng)], decim=decim))
    streams.append(_chain(sf, ctor_cr, reduced, [dict(fields=(3, 0, 1, None, None), rng=rng), dict(fields=(9, 4, 1, None, None), rng=rng), dict(fields=(4, 1, 0, None, None), rng=rng)],
                          decim=decim))
    return _cell("header_fields/sf%d%s%s_cr%d" % (sf, "r" if reduced else "", "_d%d" % decim if decim != 8 else "", ctor_cr), sf, ctor_cr, streams, reduced, decim)


def _other_class(cr: int) -> int:
    return 1 if cr >= 3 else 4


def _carry(sf, ctor_cr, reduced=False, decim=8) -> tuple:
    """four packets whose CR field alternates between the classes (1, 4, 2, 3), each header with a two-bit error on its CR / CRC codeword that the
    class the decoder carries reads as the field sent and the other class reads as something else: a packet decoded under the wrong carried CR shows
    in its header bytes, its symbol count and its payload"""
    rng = _seed("carry", sf, ctor_cr, reduced, decim)
    streams = []
    for k in range(2):
        cr_run, frames = ctor_cr, []
        for j, cr in enumerate((1, 4, 2, 3)):
            fields = (6 + 3 * j + k, cr, 1, None, None)
            masks = []
            for m in PATTERNS[8:]:
                cws = header_codewords(fields[:3] + (0, 0), [0] * (sf - 7), sf, [(2, m)])
                mine, other = header_bytes(cws[:5], cr_run), header_bytes(cws[:5], _other_class(cr_run))
                if mine[1] >> 5 == cr and mine != other:
                    masks.append(m)
            assert masks, (fields, cr_run)
            frames += _chain(sf, cr_run, reduced, [dict(fields=fields, hdr_xor=[(2, masks[(j + 3 * k) % len(masks)])], rng=rng)], decim=decim)
            _, (_, cr_run, _, _) = frames[-1].decode(cr_run)
            assert cr_run == cr
        streams.append(frames)
    return _cell("carry/sf%d%s%s_cr%d" % (sf, "r" if reduced else "", "_d%d" % decim if decim != 8 else "", ctor_cr), sf, ctor_cr, streams, reduced, decim)


def _fields_with_zero_word(sf, cr, rng) -> tuple:
    """header fields (zero spare codewords) whose block holds a word 0 - a bit that is 0 in all five codewords"""
    for t in rng.permutation(15 * 16 * 16):
        fields = (1 + int(t) % 15, cr, 1, (int(t) // 15) % 16, int(t) // 240)
        if 0 in interleave(header_codewords(fields, [0] * (sf - 7), sf), sf - 2, 8):
            return fields
    raise AssertionError("no header with a zero word")


def _residues(sf, reduced, decim=8, wrap_top=False) -> tuple:
    """header symbols (and reduced-rate payload symbols) one, two and three bins off the grid; words 0 at residues 2 and 3 are the wrap at bins
    N - 2 and N - 1 (the latter is shift 0: demodulators 1 and 2 only, `wrap_top`)"""
    rng = _seed("residues", sf, reduced, decim, wrap_top)
    streams = []
    for k in range(3):
        fields = _fields_with_zero_word(sf, (1, 4, 2)[k], rng)
        probe = craft_frame(sf, 4, reduced, fields=fields, rng=_seed("residues-probe", sf, k), spare=[0] * (sf - 7))
        hw, _ = probe.words(1)
        res_of = lambda w, r: (2 if r == 3 and w == 0 and not wrap_top else r)
        hdr_res = [(3 if wrap_top else 2) if w == 0 else int(rng.integers(4)) for w in hw]
        spec = dict(fields=fields, spare=[0] * (sf - 7), hdr_res=hdr_res)
        if reduced:
            n_pay = len(probe.pay_bins)
            pw = [int(v) for v in rng.integers(0, 1 << (sf - 2), n_pay)]
            pw[1], pw[2], pw[n_pay - 1] = 0, 0, 0                         # the wrap, at the residues below
            pr = [int(v) for v in rng.integers(4, size=n_pay)]
            pr[1], pr[2], pr[n_pay - 1] = 2, (3 if wrap_top else 2), 1
            pr = [res_of(w, r) for w, r in zip(pw, pr)]
            spec.update(pay_words=pw, pay_res=pr)
        else:
            spec.update(rng=rng)
        streams.append(_chain(sf, 4, reduced, [spec], decim=decim))
    return _cell("residues/sf%d%s%s%s" % (sf, "r" if reduced else "", "_d%d" % decim if decim != 8 else "", "_top" if wrap_top else ""), sf, 4, streams, reduced, decim,
                 demods=(1, 2) if wrap_top else (0, 1, 2))


def _longest(sf, reduced, cr) -> tuple:
    rng = _seed("longest", sf, reduced, cr)
    return _cell("longest/sf%d%s_cr%d" % (sf, "r" if reduced else "", cr), sf, 4, [_chain(sf, 4, reduced, [dict(fields=(255, cr, 1, None, None), rng=rng)])], reduced)


def _top_word(sf, decim=8) -> tuple:
    """the full-rate word 1 << (sf - 1) first, in the middle and last in a block, at CR 4 (Hamming) and CR 1 (data bits)"""
    rng = _seed("top_word", sf, decim)
    streams = []
    for cr in (4, 1):
        spb = 4 + cr
        streams.append(_chain(sf, 4, False, [dict(fields=(12, cr, 1, 2, 7), rng=rng, top_at=(0, spb + spb // 2, 3 * spb - 1))], demod=1, decim=decim))
    # (demodulator 2 pins the word's bin to 0 and its fine_sync, fed that bin, moves the symbol clock by a sample: an eighth of a bin at decimation 8,
    # but half a bin at decimation 2, where every symbol behind it then sits on a tie between two bins - there the word goes to demodulator 1 only)
    return _cell("top_word/sf%d%s" % (sf, "_d%d" % decim if decim != 8 else ""), sf, 4, streams, False, decim, demods=(1, 2) if decim == 8 else (1,))


def _implicit(sf, decim, cr=3) -> tuple:
    rng = _seed("implicit", sf, decim)
    streams = [[craft_frame(sf, cr, False, implicit=True, rng=rng, n_pay=(4 + cr) * nb, decim=decim) for nb in (3, 5)]]
    return _cell("implicit/sf%d_d%d" % (sf, decim), sf, cr, streams, False, decim, implicit=True, crc=False)


@functools.lru_cache(None)
def case_sets() -> list:
    """[(name, TxConfig kwargs, decoder kwargs (+ "demods": the demodulators the case may run on), [streams of Frames])]"""
    out = []
    # random_words: >= 300 codewords per CR class and cell at SF7-SF9, one block-rich packet per CR at SF10-SF12
    for sf, reduced, decim, n_cw in ((7, False, 8, 160), (7, True, 8, 160), (8, False, 8, 160), (9, False, 8, 160), (9, True, 8, 160),
                                    (7, False, 2, 160), (8, False, 4, 160), (9, False, 2, 160), (9, True, 4, 160), (9, False, 4, 160),
                                    (10, False, 8, 60), (10, False, 4, 60)):
        out.append(_random_words(sf, reduced, decim, n_cw, all_values=sf <= 9 and not reduced, spare_values=(sf, decim) == (9, 8) and not reduced))
    for sf, reduced, crs in ((11, True, (1, 4)), (12, True, (2, 3)), (11, False, (2, 3)), (12, False, (1, 4))):   # two packets per cell
        out.append(_random_words(sf, reduced, 8, 40, crs))
    for sf in (7, 8):                                                     # sixteen distinct single-packet streams for the two-per-CU builds
        streams = []
        for k in range(16):
            rng = _seed("many", sf, k)
            streams.append(_chain(sf, 4, False, [dict(fields=(10 + k, 1 + k % 4, k & 1, None, None), rng=rng)]))
        out.append(_cell("many/sf%d" % sf, sf, 4, streams))
    # header_bit_errors
    every = [(i, p) for i in range(5) for p in range(36)]
    out.append(_bit_errors(7, 4, every))
    out.append(_bit_errors(7, 1, every))
    for k, (sf, decim) in enumerate(((8, 8), (9, 8), (10, 8), (7, 2), (8, 4), (9, 2), (9, 4))):
        out.append(_bit_errors(sf, 4, _spread(k), decim))
        out.append(_bit_errors(sf, 1, _spread(k + 2)[:12], decim))
    out.append(_bit_errors(11, 4, _spread(1)[8::7]))                      # (SF11 / SF12: a few two-bit patterns)
    out.append(_bit_errors(12, 1, _spread(3)[9::9]))
    # header_fields
    out.append(_header_fields(7, 4, long_all=True))
    out.append(_header_fields(9, 4, full_crc=(1,)))                        # (the block edges with the CRC bit set only: SF9 symbols are four SF7 symbols long)
    for sf, ctor_cr in ((7, 1), (7, 0), (8, 4), (8, 1), (9, 1), (9, 0)):
        out.append(_header_fields(sf, ctor_cr, full=False))
    out.append(_header_fields(10, 4, full=False, cr_fields=(0, 2, 3, 6)))
    out.append(_header_fields(9, 4, decim=2, full=False))
    out.append(_header_fields(11, 1, reduced=True, full=False, cr_fields=(0, 1, 4, 7)))
    # carry
    for sf, ctor_cr, reduced, decim in ((7, 4, False, 8), (7, 1, False, 8), (8, 4, False, 8), (9, 4, False, 8), (9, 1, True, 8), (10, 4, False, 8), (11, 4, True, 8),
                                        (7, 4, False, 2), (8, 4, False, 4), (9, 4, False, 2), (9, 4, False, 4), (10, 4, False, 4)):
        out.append(_carry(sf, ctor_cr, reduced, decim))
    # residues
    for sf, reduced, decim in ((7, False, 8), (7, True, 8), (8, False, 8), (9, True, 8), (9, False, 8), (10, False, 8), (11, True, 8), (9, True, 4), (7, False, 2), (10, False, 4)):
        out.append(_residues(sf, reduced, decim))
    for sf, reduced in ((7, True), (9, True), (11, True)):
        out.append(_residues(sf, reduced, 8, wrap_top=True))
    # longest
    for sf, reduced in ((7, False), (12, True)):
        for cr in (1, 4):
            out.append(_longest(sf, reduced, cr))
    # top_word
    for sf, decim in ((7, 8), (8, 8), (9, 8), (10, 8), (9, 2), (10, 4)):
        out.append(_top_word(sf, decim))
    # implicit header (the generic walker's SF7 cell and walker2's SF6)
    out.append(_implicit(7, 8))
    out.append(_implicit(6, 4))
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    return out


def cases(prefix: str = "", **where) -> list:
    """the cells of case_sets() whose name starts with `prefix` and whose decoder kwargs match `where`"""
    return [c for c in case_sets() if c[0].startswith(prefix) and all(c[2].get(k) == v for k, v in where.items())]


def decoder_kwargs(dec_kw: dict, demod: int) -> dict:
    kw = {k: v for k, v in dec_kw.items() if k != "demods"}
    assert demod in dec_kw["demods"], (dec_kw, demod)
    kw["demod"] = demod
    return kw


# ---- which cells each device copy of the chain decodes (tests/test_gpu_chain.py), and on which demodulators ----------------------------------
def _pick(pred, demods) -> List[Tuple[str, int]]:
    return [(c[0], d) for c in case_sets() if pred(c[0], c[2]) for d in demods if d in c[2]["demods"]]


@functools.lru_cache(None)
def families() -> Dict[str, List[Tuple[str, int]]]:
    """{family: [(cell name, demodulator)]} - the SF / demodulator cells of every family of the device's decode chain"""
    d8 = lambda kw: kw["samp_rate"] == RATES[8]
    few = lambda n: not n.startswith("many/")
    small = lambda n: n.split("/")[0] in ("random_words", "header_bit_errors", "carry", "residues", "top_word")
    f = {}
    f["walker2_wide"] = (_pick(lambda n, kw: d8(kw) and kw["sf"] in (7, 8) and few(n) and not kw["implicit"], (0, 2))
                         + _pick(lambda n, kw: n in ("random_words/sf7", "residues/sf7r_top", "top_word/sf7", "carry/sf7_cr1"), (1,)))
    f["walker2_two_per_cu"] = _pick(lambda n, kw: n.startswith("many/"), (0, 2))
    f["walker2_decim"] = (_pick(lambda n, kw: not d8(kw) and kw["sf"] <= 9, (0, 2)) + _pick(lambda n, kw: n == "top_word/sf9_d2", (1,)))
    f["walker3"] = _pick(lambda n, kw: d8(kw) and kw["sf"] >= 9, (0, 2)) + _pick(lambda n, kw: n in ("top_word/sf9", "top_word/sf10"), (1,))
    f["walker3_trace"] = _pick(lambda n, kw: d8(kw) and kw["sf"] in (9, 10) and small(n), (0, 2))
    f["walker3_half"] = (_pick(lambda n, kw: d8(kw) and kw["sf"] == 9 and small(n), (0,)) + _pick(lambda n, kw: d8(kw) and kw["sf"] == 10 and small(n), (0, 2)))
    f["payload_pass"] = _pick(lambda n, kw: d8(kw) and few(n) and not kw["implicit"] and (kw["sf"] in (7, 8, 9) or (kw["sf"] == 11 and kw["reduced_rate"]))
                              and not n.startswith("header_fields/sf7_cr4") and not n.startswith("header_fields/sf9_cr4"), (0, 2))
    f["generic"] = (_pick(lambda n, kw: d8(kw) and kw["sf"] in (7, 9) and (small(n) or n in ("header_fields/sf7_cr0", "header_fields/sf9_cr1", "implicit/sf7_d8")), (0, 2))
                    + _pick(lambda n, kw: kw["sf"] == 10 and not d8(kw), (0, 2)) + _pick(lambda n, kw: n in ("top_word/sf10_d4", "top_word/sf7"), (1,)))
    return f


def cell(name: str) -> tuple:
    (c,) = [c for c in case_sets() if c[0] == name]
    return c
