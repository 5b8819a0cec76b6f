"""Soft-decision decoding of a LoRa frame at a known header position: the float64 definition (include/lora_hip_soft.h).

The hard chain turns every symbol into its arg-max bin and throws away what tells a wrong bin from a barely-right one; the block
de-interleaver then spreads every codeword over 4 + CR symbols and Hamming(8,4) corrects one bit at 4/8 and nothing at 4/5 and 4/6.  Here
every bit of a symbol's word keeps a log-likelihood ratio taken from the whole dechirped spectrum, the LLRs go through the de-interleaver,
the de-shuffle and the de-whitening as positions and signs, and each codeword is decided by correlation against the 16 codewords of the
Hamming(8,4) code - at every CR: a position that was not sent is an erasure (LLR 0).  Numpy only, no torch and no device: this is what
soft_symbols_kernel / soft_chain_kernel (gr_lora_amd/csrc/lora_soft.inc.hip) and lora_hip_soft_decode_at_headers_device are held to.

  symbol metric   m[k] = |X[k]|, X the N bins k in [-N/2, N/2) (index k mod N) of the sps-point DFT of x * d_downchirp - the magnitude, not
                  the power: at working SNR the non-coherent log-likelihood is linear in |X|
  bin, word       b(k) = (k - 1) mod N (the plain FFT demodulator's bin); full rate w = gray(b), ppm = sf bits; reduced rate
                  w = gray(((b + 2) // 4) mod (N / 4)), ppm = sf - 2 bits.  The eight header symbols are always at the reduced rate
  bit LLR         L[i] = max{m[k]: bit i of w(k) = 0} - max{m[k]: bit i of w(k) = 1} (max-log); positive: the bit is 0
  codeword LLRs   a block of n_w words yields ppm codewords x: C_x[i] = L_i[(x - i) mod ppm], i < n_w
  de-shuffle      D_x[j] = C_x[SHUFFLE[j]] where SHUFFLE[j] < n_w, else 0 (an erasure), j = 0 .. 7
  de-whitening    D_x[j] negated where bit j of the codeword's whitening byte is 1
  decision        score[s] = sum over j ascending of (bit j of ENC[s] ? -D[j] : D[j]); the nibble is the smallest s with the largest score,
                  margin = best - second best; second = the smallest s != nibble with the largest score among the rest
  CRC repair      (off unless asked for; crc_repair below) where a published frame's payload CRC fails, the L least reliable codewords of the
                  frame body may take their second-best nibble: of the 2^L - 1 patterns the one that makes the CRC hold at the smallest
                  summed margin is applied.  The CRC is affine over GF(2) in the body bits, so every pattern is one XOR of L fixed 16-bit words
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import linkmetrics, synth

SHUFFLE = (5, 0, 1, 2, 4, 3, 6, 7)
DATA_IDX = (1, 2, 3, 5)
ENC = tuple(synth.hamming_encode(n) for n in range(16))
STATUS_FRAME, STATUS_HEADER_REJECTED, STATUS_CR_ZERO, STATUS_TRUNCATED = 0, 1, 2, 3
REPAIR_NOT_ATTEMPTED, REPAIR_CRC_HELD, REPAIR_REPAIRED, REPAIR_FAILED = 0, 1, 2, 3
REPAIR_MAX_CANDIDATES = 8
_SIGN = np.array([[-1.0 if (ENC[s] >> j) & 1 else 1.0 for j in range(8)] for s in range(16)])
_H84 = tuple(min(range(16), key=lambda s: (bin(c ^ ENC[s]).count("1"), s)) for c in range(256))


def whitening(name: str) -> np.ndarray:
    """HEADER, CR56 or CR78 of gr_lora_amd/csrc/whitening_data.inc"""
    return synth._WHITEN["LORA_WHITEN_" + name]


def _down(cfg) -> np.ndarray:
    return linkmetrics.downchirp(cfg.sf, cfg.bw, cfg.samp_rate)


def magnitudes(iq: np.ndarray, pos: int, cfg, down: Optional[np.ndarray] = None) -> np.ndarray:
    """m[k], index k mod N, of the window of sps items at pos"""
    down = _down(cfg) if down is None else down
    sps, N = down.size, cfg.nbins
    F = np.fft.fft(np.asarray(iq[pos:pos + sps], dtype=np.complex128) * down.astype(np.complex128))
    return np.abs(np.concatenate([F[:N // 2], F[sps - N // 2:]]))


def words_of_index(sf: int, reduced: bool) -> np.ndarray:
    """w(k) for k = 0 .. N - 1"""
    N = 1 << sf
    b = (np.arange(N) - 1) % N
    if reduced:
        b = ((b + 2) // 4) % (N // 4)
    return b ^ (b >> 1)


def llr_of_magnitudes(m: np.ndarray, sf: int, reduced: bool) -> np.ndarray:
    w = words_of_index(sf, reduced)
    ppm = sf - 2 if reduced else sf
    L = np.empty(ppm)
    for i in range(ppm):
        one = ((w >> i) & 1).astype(bool)
        L[i] = m[~one].max() - m[one].max()
    return L


def llr_window(iq: np.ndarray, pos: int, cfg, reduced: bool, down: Optional[np.ndarray] = None):
    """-> (L[ppm], arg-max index k, peak magnitude, sum of m^2, second largest magnitude)"""
    m = magnitudes(iq, pos, cfg, down)
    k = int(np.argmax(m))
    second = float(np.partition(m, -2)[-2])
    return llr_of_magnitudes(m, cfg.sf, reduced), k, float(m[k]), float((m * m).sum()), second


def soft_block(llrs, ppm: int, n_w: int, whitening_bytes: Sequence[int], dtype=np.float64, first: int = 0, with_second: bool = False):
    """llrs[n_w][ppm] -> (nibbles, margins, hard words, sums of |LLR|) of the codewords x = first .. first + len(whitening_bytes) - 1 (all ppm
    of them: give ppm whitening bytes).  A hard word is the de-whitened 8-bit word of the signs (D < 0; an erased position reads as its
    whitening bit, which is what the integer chain's zero becomes there).  With a dtype of float32 every sum is formed as the device forms it.
    with_second: a fifth list, the second-best nibble of every codeword (the one its margin is measured against)."""
    L = np.asarray(llrs, dtype=dtype)
    assert L.shape == (n_w, ppm), (L.shape, n_w, ppm)
    sign = _SIGN.astype(dtype)
    nibbles, margins, hards, sums, seconds = [], [], [], [], []
    for n, wb in enumerate(whitening_bytes):
        x = first + n
        C = [L[i][(x - i) % ppm] for i in range(n_w)]
        D = np.zeros(8, dtype=dtype)
        hard = 0
        for j in range(8):
            if SHUFFLE[j] < n_w:
                D[j] = C[SHUFFLE[j]]
            hard |= (int(D[j] < 0) ^ ((int(wb) >> j) & 1)) << j
            if (int(wb) >> j) & 1:
                D[j] = -D[j]
        sc = np.zeros(16, dtype=dtype)
        for j in range(8):
            sc = sc + sign[:, j] * D[j]
        s = int(np.argmax(sc))                                            # (the first of equal maxima)
        rest = np.delete(sc, s)
        r = int(np.argmax(rest))                                          # (the first of equal maxima among the rest)
        seconds.append(r if r < s else r + 1)
        sa = dtype(0.0)
        for c in C:
            sa = sa + abs(c)
        nibbles.append(s)
        margins.append(dtype(sc[s] - rest.max()))
        hards.append(hard)
        sums.append(sa)
    if with_second:
        return nibbles, margins, hards, sums, seconds
    return nibbles, margins, hards, sums


def hard_nibble(word: int, cr: int) -> int:
    """what the integer chain makes of a de-whitened word under the FEC class of `cr`"""
    return _H84[word] if cr >= 3 else sum(((word >> p) & 1) << j for j, p in enumerate(DATA_IDX))


def _table(cr: int) -> np.ndarray:
    return whitening("CR56" if cr <= 2 else "CR78")


def _wh(tab: np.ndarray, first: int, n: int) -> List[int]:
    return [int(tab[i]) if i < len(tab) else 0 for i in range(first, first + n)]


def header_checksum_ok(phdr: Sequence[int]) -> bool:
    c4, low = synth.valid_hdr_nibbles(phdr[0], phdr[1] >> 5, bool((phdr[1] >> 4) & 1))
    return ((phdr[1] & 1), phdr[2] >> 4) == (c4, low)


def soft_header(llr_header, sf: int, dtype=np.float64):
    """the five header codewords -> (the three header bytes, cr field rewritten, nibbles, margins, hard words, sums)"""
    nib, mar, hard, sums = soft_block(llr_header, sf - 2, 8, _wh(whitening("HEADER"), 0, 5), dtype)
    phdr = [(nib[0] << 4) | nib[1], (nib[2] << 4) | nib[3], (nib[4] << 4) | _H84[int(whitening("HEADER")[5])]]
    if (phdr[1] >> 5) > 4:
        phdr[1] = (phdr[1] & 0x1f) | (4 << 5)
    return phdr, nib, mar, hard, sums


def body_bytes(nibbles: Sequence[int], payload_length: int) -> List[int]:
    """the payload_length bytes of the frame body, low nibble first; 0 where a nibble is missing"""
    return [(nibbles[2 * k] if 2 * k < len(nibbles) else 0) | ((nibbles[2 * k + 1] if 2 * k + 1 < len(nibbles) else 0) << 4) for k in range(payload_length)]


def syndrome(body: Sequence[int], length: int) -> int:
    """lora_hip_check_frame's payload CRC as one word: calculated XOR received, 0 where the CRC holds.  body: length + 2 bytes.  The CRC starts at 0
    and has no final XOR, so this is affine over GF(2) in the bits of body (the constant: the two whitening bytes)."""
    w = synth.whitening_bytes(length + 2)
    return synth.lora_crc16(bytes(body[:length])) ^ ((body[length] ^ w[length]) | ((body[length + 1] ^ w[length + 1]) << 8))


def syndrome_effect(c: int, delta: int, length: int) -> int:
    """what XORing delta into body codeword c (nibble c & 1 of byte c >> 1) changes the syndrome by: the syndrome of the body that is zero but
    for delta << 4 (c & 1) at byte c >> 1, XOR the syndrome of the zero body"""
    zero = [0] * (length + 2)
    one = list(zero)
    one[c >> 1] = (delta & 15) << (4 * (c & 1))
    return syndrome(one, length) ^ syndrome(zero, length)


def no_repair(status: int = REPAIR_NOT_ATTEMPTED, dtype=np.float64) -> dict:
    return dict(status=status, candidates=0, pattern=0, changed=0, syndrome=0, penalty=dtype(0.0), codewords=[])


def crc_repair(nibbles: Sequence[int], seconds: Sequence[int], margins: Sequence, payload_length: int, candidates: int, dtype=np.float64):
    """CRC-aided repair of a frame body that carries a payload CRC.  nibbles / seconds / margins: the codewords that feed the body (spare header
    codewords first, then payload codewords: soft_chain's list behind the five header codewords); payload_length counts the two CRC bytes.
    -> (new nibbles, record).
      eligible    the codewords c < 2 * payload_length (those that are there)
      candidates  the n_cand = min(candidates, eligible) of them with the smallest (margin, c), margins compared as values; candidate 0 is the least reliable
      e[i]        what the syndrome changes by when candidate i takes its second nibble: syndrome of the body that is zero but for
                  (nibble ^ second) << 4 (c & 1) at byte c >> 1, XOR the syndrome of the zero body
      pattern p   1 .. 2^n_cand - 1 matches iff the XOR of e[i] over its set bits is the body's syndrome; penalty: the sum of margin[i] over the
                  set bits, i ascending, in dtype.  The matching pattern with the smallest (penalty, p) is applied
    record: status (CRC_HELD: nothing else is filled in), candidates (n_cand), pattern, changed (its set bits), syndrome (before repair), penalty,
    codewords (the n_cand indices c)."""
    assert 1 <= candidates <= REPAIR_MAX_CANDIDATES and payload_length >= 2
    length = payload_length - 2
    out = list(nibbles)
    syn = syndrome(body_bytes(out, payload_length), length)
    if syn == 0:
        return out, no_repair(REPAIR_CRC_HELD, dtype)
    eligible = range(min(2 * payload_length, len(out)))
    cand = sorted(eligible, key=lambda c: (float(margins[c]), c))[:candidates]
    n_cand = len(cand)
    e = [syndrome_effect(c, out[c] ^ int(seconds[c]), length) for c in cand]
    best = None
    for p in range(1, 1 << n_cand):
        x, pen = 0, dtype(0.0)
        for i in range(n_cand):
            if (p >> i) & 1:
                x ^= e[i]
                pen = dtype(pen + dtype(margins[cand[i]]))
        if x == syn and (best is None or (pen, p) < best):
            best = (pen, p)
    rec = dict(status=REPAIR_FAILED, candidates=n_cand, pattern=0, changed=0, syndrome=syn, penalty=dtype(0.0), codewords=list(cand))
    if best is not None:
        rec.update(status=REPAIR_REPAIRED, pattern=best[1], changed=bin(best[1]).count("1"), penalty=best[0])
        for i, c in enumerate(cand):
            if (best[1] >> i) & 1:
                out[c] = int(seconds[c])
    return out, rec


_repair = crc_repair                                                      # (soft_chain and decode_frame take an argument of that name)


def soft_chain(llr_header, llr_payload, cfg, dtype=np.float64, require_header_checksum: bool = False, crc_repair: int = 0):
    """llr_header[8][sf - 2], llr_payload[n][ppm] (n >= the symbols the header asks for; None or fewer rows: TRUNCATED)
    -> (bytes behind the loratap header or None, report).  report["nibbles"] / ["margins"]: every codeword decided, the five header ones first.
    crc_repair = L in 1 .. 8: where a frame is published with a CRC that fails, the function crc_repair above with L candidates; the bytes
    returned and crc_ok are those after repair, report["repair"] is its record, every other key keeps its meaning (the decision before repair)."""
    L = int(crc_repair)
    assert 0 <= L <= REPAIR_MAX_CANDIDATES
    sf = cfg.sf
    ppm = sf - 2 if cfg.reduced_rate else sf
    phdr, nib, mar, hard, sums = soft_header(llr_header, sf, dtype)
    cr, has_crc = phdr[1] >> 5, (phdr[1] >> 4) & 1
    payload_length = phdr[0] + 2 * has_crc
    rep = dict(status=STATUS_FRAME, cr=cr, payload_length=payload_length, payload_symbols=0, header_checksum_ok=int(header_checksum_ok(phdr)),
               has_crc=has_crc, crc_ok=0, codewords=5, changed=sum(int(n != _H84[h]) for n, h in zip(nib, hard)),
               min_margin=dtype(min(mar)), mean_abs_llr=0.0, nibbles=list(nib), margins=list(mar))
    if L:
        rep["repair"] = no_repair(dtype=dtype)
    if cr == 0:
        rep["status"] = STATUS_CR_ZERO
        return None, rep
    if require_header_checksum and not rep["header_checksum_ok"]:
        rep["status"] = STATUS_HEADER_REJECTED
        return None, rep
    n_sym = synth.payload_symbol_count(payload_length, sf, cr, cfg.reduced_rate)
    rep["payload_symbols"] = n_sym
    if llr_payload is None or len(llr_payload) < n_sym:
        rep["status"] = STATUS_TRUNCATED
        return None, rep
    tab = _table(cr)
    n_spare = sf - 7
    nibs, margins, hards, sums_all, seconds = [], list(mar), [], list(sums), []
    if n_spare:
        n, m, h, s, s2 = soft_block(llr_header, sf - 2, 8, _wh(tab, 0, n_spare), dtype, first=5, with_second=True)
        nibs += n; margins += m; hards += h; sums_all += s; seconds += s2
    spb = 4 + cr
    for b in range(n_sym // spb):
        n, m, h, s, s2 = soft_block(np.asarray(llr_payload[b * spb:(b + 1) * spb])[:, :ppm], ppm, spb, _wh(tab, n_spare + b * ppm, ppm), dtype, with_second=True)
        nibs += n; margins += m; hards += h; sums_all += s; seconds += s2
    rep["codewords"] = 5 + len(nibs)
    rep["nibbles"], rep["margins"] = list(nib) + nibs, margins
    rep["changed"] += sum(int(n != hard_nibble(h, cr)) for n, h in zip(nibs, hards))
    rep["min_margin"] = dtype(min(margins))
    rep["mean_abs_llr"] = float(np.sum(np.asarray(sums_all, dtype=np.float64)) / (8 * (sf - 2) + n_sym * ppm))
    body = body_bytes(nibs, payload_length)
    if has_crc and payload_length >= 2:
        if L:
            fixed, rep["repair"] = _repair(nibs, seconds, margins[5:], payload_length, L, dtype)
            body = body_bytes(fixed, payload_length)
        rep["crc_ok"] = int(syndrome(body, phdr[0]) == 0)
    return bytes(phdr + body), rep


def symbols_taken(payload_symbols: int) -> int:
    """payload symbols the decoder consumes: a header that asks for none still takes one (and no block)"""
    return payload_symbols if payload_symbols > 0 else 1


def decode_frame(iq: np.ndarray, header_pos: int, cfg, dtype=np.float64, require_header_checksum: bool = False, down: Optional[np.ndarray] = None,
                 crc_repair: int = 0):
    """The frame whose first header symbol is the window at header_pos: symbol k is the window at header_pos + k * sps, no fine_sync.
    -> (bytes or None, report); report["end_pos"] where a frame was published.  TRUNCATED as in the hard path: every symbol taken needs
    2 * sps items from its position.  crc_repair: as in soft_chain."""
    down = _down(cfg) if down is None else down
    sps = down.size
    assert header_pos >= 0 and header_pos + 2 * sps <= len(iq)
    if header_pos + 9 * sps > len(iq):
        rep = dict(status=STATUS_TRUNCATED, payload_symbols=0)
        if crc_repair:
            rep["repair"] = no_repair(dtype=dtype)
        return None, rep
    W = [llr_window(iq, header_pos + k * sps, cfg, True, down) for k in range(8)]
    Lh = np.array([w[0] for w in W])
    blob, rep = soft_chain(Lh, None, cfg, dtype, require_header_checksum, crc_repair)
    rep["peak"] = max(w[2] for w in W)
    if rep["status"] != STATUS_TRUNCATED:
        return blob, rep
    n_sym = rep["payload_symbols"]
    taken = symbols_taken(n_sym)
    if header_pos + (8 + taken + 1) * sps > len(iq):
        return None, rep
    W += [llr_window(iq, header_pos + (8 + k) * sps, cfg, cfg.reduced_rate, down) for k in range(n_sym)]
    blob, rep = soft_chain(Lh, [w[0] for w in W[8:]], cfg, dtype, require_header_checksum, crc_repair)
    rep["end_pos"] = header_pos + (8 + taken) * sps
    rep["peak"] = max(w[2] for w in W)                                    # the largest magnitude of the frame's windows
    rep["words"] = [sum(int(v < 0) << i for i, v in enumerate(w[0])) for w in W]   # the hard word of every symbol, header first
    return blob, rep
