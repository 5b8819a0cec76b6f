"""Frame bodies as codewords for the CRC-aided repair (softdecode.crc_repair; lora_hip_soft_crc_repair_codewords), shared by
tests/test_soft_repair_model.py (CPU) and tests/test_gpu_soft_repair.py (device): hand-made edge cases and random frames with quantised margins.
A case is (name, length, nibbles, seconds, margins, candidates): length counts the payload bytes in front of the two CRC bytes, the three lists
hold the 2 * (length + 2) body codewords; margins are float32 values."""
import functools

import numpy as np

from gr_lora_amd import synth


def valid_nibbles(rng, length):
    """the codewords (low nibble first) of a body of `length` random bytes and the CRC bytes that hold"""
    payload = bytes(rng.integers(0, 256, length, dtype=np.uint8))
    body = payload + synth.valid_crc_bytes(payload)
    return [(b >> (4 * t)) & 15 for b in body for t in (0, 1)]


def other_nibbles(rng, nibbles):
    """a runner-up for every codeword: any nibble but the codeword's own"""
    return [(n + int(rng.integers(1, 16))) & 15 for n in nibbles]


def wrong_at(rng, nibbles, seconds, where):
    """codewords `where` decided wrongly with the right nibble as runner-up"""
    for c in where:
        seconds[c] = nibbles[c]
        nibbles[c] = (nibbles[c] + int(rng.integers(1, 16))) & 15


def _case(name, rng, length, where, margins, candidates, runner_up_right=True):
    nib = valid_nibbles(rng, length)
    sec = other_nibbles(rng, nib)
    if runner_up_right:
        wrong_at(rng, nib, sec, where)
    else:
        for c in where:
            nib[c] = (nib[c] + 1) & 15
            sec[c] = (nib[c] + 1) & 15                                    # (neither is the nibble sent)
    m = np.asarray(margins, dtype=np.float32)
    assert m.size == len(nib) == 2 * (length + 2), (name, m.size, len(nib))
    return name, length, nib, sec, [np.float32(v) for v in m], candidates


@functools.lru_cache(None)
def edge_cases():
    rng = np.random.default_rng(4242)
    ramp = lambda n: 1.0 + np.arange(n) / 8.0
    out = []
    out.append(_case("crc holds", rng, 5, [], ramp(14), 8))
    # every margin equal: the candidates are the lowest indices
    out.append(_case("equal margins, error inside", rng, 3, [2], np.ones(10), 4))
    out.append(_case("equal margins, error outside", rng, 3, [4], np.ones(10), 4))
    # -0.0 and 0.0 are one value: codeword 1 (0.0) comes before codeword 6 (-0.0)
    m = ramp(10); m[6] = -0.0; m[1] = 0.0
    out.append(_case("signed zeros", rng, 3, [1, 6], m, 2))
    # length 0: four eligible codewords, fewer than L
    out.append(_case("length 0", rng, 0, [3], [0.5, 0.25, 0.75, 0.125], 8))
    out.append(_case("length 0, all wrong", rng, 0, [0, 1, 2, 3], [0.5, 0.25, 0.75, 0.125], 8))
    # two candidates in one byte; candidates inside the CRC bytes
    m = ramp(38); m[[10, 11]] = [0.125, 0.25]
    out.append(_case("two in one byte", rng, 17, [10, 11], m, 8))
    m = ramp(38); m[[34, 35, 36, 37]] = [0.5, 0.125, 0.25, 0.0625]
    out.append(_case("inside the CRC bytes", rng, 17, [35, 36], m, 6))
    # the last payload byte and the low CRC byte enter the syndrome alike (length 1: codewords 0 and 2): with equal deltas and equal margins the
    # patterns {0} and {2} both match at one penalty, and the smaller pattern - candidate 0, codeword 0 - wins although codeword 2 is the wrong one
    name, length, nib, sec, mar, L = _case("equal penalties", rng, 1, [2], [0.5, 2.0, 0.5, 2.0, 2.0, 2.0], 8)
    sec[0] = nib[0] ^ (nib[2] ^ sec[2])
    out.append((name, length, nib, sec, mar, L))
    # length 2: codewords 2 and 4 enter alike (low byte, low nibble), and so do 1 and 7 (high byte, high nibble).  Codewords 1 and 2 are wrong,
    # their twins offer the same deltas, so four patterns match, all at 0.25 + 0.5: the smallest, candidates {0, 2} = codewords {2, 1}, wins
    name, length, nib, sec, mar, L = _case("equal sums", rng, 2, [1, 2], [3.0, 0.5, 0.25, 3.0, 0.25, 3.0, 3.0, 0.5], 4)
    sec[4] = nib[4] ^ (nib[2] ^ sec[2])
    sec[7] = nib[7] ^ (nib[1] ^ sec[1])
    out.append((name, length, nib, sec, mar, L))
    # no pattern matches: the wrong codewords are not among the candidates, or their runner-up is wrong too
    out.append(_case("failed, not a candidate", rng, 9, [20], ramp(22), 8))
    m = ramp(22); m[3] = 0.125
    out.append(_case("failed, runner-up wrong", rng, 9, [3], m, 1, runner_up_right=False))
    # the longest bodies: 514 and 512 codewords, three per lane of the workgroup
    m = 1.0 + rng.integers(0, 8, 514) / 8.0; m[[0, 255, 256, 511, 513]] = [0.5, 0.25, 0.25, 0.125, 0.375]
    out.append(_case("length 255", rng, 255, [255, 513], m, 8))
    m = 1.0 + rng.integers(0, 8, 512) / 8.0; m[[7, 300, 510]] = [0.5, 0.25, 0.125]
    out.append(_case("length 254", rng, 254, [7, 300, 510], m, 5))
    out.append(_case("length 2", rng, 2, [0, 7], [0.5, 3, 3, 3, 3, 3, 3, 0.25], 2))
    return out


@functools.lru_cache(None)
def random_cases(n=200, seed=777):
    """n frames of lengths 0 .. 40 with zero to four wrong codewords and margins quantised to 8 levels (ties everywhere); the wrong codewords
    draw from the lower levels, as unreliable decisions do"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        length = int(rng.integers(0, 41))
        n_cw = 2 * (length + 2)
        nib = valid_nibbles(rng, length)
        sec = other_nibbles(rng, nib)
        where = [int(c) for c in rng.choice(n_cw, size=min(int(rng.integers(0, 5)), n_cw), replace=False)]
        wrong_at(rng, nib, sec, where)
        m = rng.integers(2, 8, n_cw) / 8.0
        m[where] = rng.integers(0, 4, len(where)) / 8.0
        out.append(("random %d" % k, length, nib, sec, [np.float32(v) for v in m], int(rng.integers(1, 9))))
    return out
