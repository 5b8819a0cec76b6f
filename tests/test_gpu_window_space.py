"""GPU: the three copies of the pruned dechirp spectrum - detect_windows_kernel, link_windows_kernel, soft_symbols_kernel - against their float64
definitions at every spreading factor 6 .. 12 and every decimation 1, 2, 4, 8, 16 (35 shapes each), on the window streams of
tests/window_cases.py, and the grid-stride loop of the detect and soft kernels past 4096 windows.  DESIGN.md 4.20.

Every amplitude-like quantity q is held as |q_dev - q_model| <= R U, U = 2^-24 log2(sps) sqrt(sps) ||m||_2 the unit of window_cases.unit:
  detect  sqrt(peak), sqrt(total), both halves          link  sqrt(peak_power), sqrt(lobe_power), sqrt(total_power)
  soft    peak and L[i] / 2 (an LLR is a difference of two maxima of magnitudes: at most twice a bin's error)
R = window_cases.LIMIT_R[kernel] = 4 x the largest err / U of the first whole sweep on an MI355X, never above the cap 16; arg-max indices, the
link frac, what may be set aside and what holds in its place: window_cases' docstring.  The zeros window (U = 0) must read exactly +0 with index 0,
a window listed first and last in one call must give bit-equal records, and the stream sits between sps NaN items either side - a read outside
it reaches a record as NaN and fails its comparison - which must be bit-equal afterwards.

Largest err / U of the first whole sweep on an MI355X, per shape, as detect link soft (every case prints its own):
        D = 1                  D = 2                  D = 4                  D = 8                  D = 16
  SF6   0.346 0.280 0.346      0.277 0.235 0.277      0.255 0.113 0.255      0.125 0.170 0.174      0.124 0.062 0.173
  SF7   0.288 0.219 0.288      0.255 0.208 0.255      0.229 0.190 0.229      0.105 0.088 0.105      0.100 0.142 0.157
  SF8   0.234 0.187 0.234      0.216 0.172 0.216      0.097 0.132 0.121      0.137 0.124 0.156      0.102 0.237 0.095
  SF9   0.215 0.180 0.215      0.124 0.163 0.157      0.181 0.119 0.181      0.108 0.114 0.083      0.110 0.102 0.117
  SF10  0.202 0.165 0.202      0.183 0.152 0.183      0.168 0.139 0.168      0.116 0.104 0.098      0.156 0.168 0.083
  SF11  0.177 0.182 0.177      0.164 0.137 0.164      0.153 0.148 0.153      0.077 0.090 0.082      0.131 0.085 0.077
  SF12  0.166 0.136 0.166      0.154 0.126 0.154      0.084 0.094 0.082      0.080 0.127 0.066      0.142 0.099 0.170
Per kernel: detect 0.3464 (sqrt(total)), link 0.2796 (sqrt(peak_power)), soft 0.3464 (peak), each one unit in the last place of the peak of the
on-bin tone k = -1 at SF6, D = 1; the grid-stride and 700-frame cases: 0.239 / 0.136 (detect), 0.152 / 0.092 (soft), 0.171 (link).
LIMIT_R = 4 x that: detect 1.386, link 1.118, soft 1.386.
"""
import math

import numpy as np
import pytest

import window_cases as WC
from gr_lora_amd import capi, linkmetrics as LM

pytestmark = pytest.mark.gpu

BW = WC.BW
CASES = [(kern, sf, decim) for kern in WC.KERNELS for sf, decim in WC.SHAPES]          # 3 x 35, every one of them run
REFUSED = {}                                                                           # (kernel, sf, decim): the refusing line - none
WORST = {}                                                                             # (kernel, sf, decim) -> (err / U, what)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU: the HIP path has no CPU fallback")
    yield torch
    if WORST:
        print("\n[window space] worst err / U per shape (kernel: SF.D value ...)")
        for kern in WC.KERNELS:
            rows = [(k[1], k[2], v[0], v[1]) for k, v in sorted(WORST.items()) if k[0] == kern]
            if rows:
                top = max(rows, key=lambda r: r[2])
                print("[window space] %s: max %.4f at SF%d D%d (%s) | %s" % (kern, top[2], top[0], top[1], top[3], " ".join("%d.%d %.3f" % r[:3] for r in rows)))


def _handle(sf, decim):
    return capi.Handle(sf=sf, samp_rate=WC.rate(decim), bandwidth=BW, reduced_rate=(sf > 10), demod=capi.DEMOD_FFT, disable_drift_correction=True)


def _table(h, sf, decim):
    down = h.table(0).view(np.complex64)
    assert down.size == h.sps == decim << sf and h.nbins == 1 << sf and h.decim == decim
    assert np.abs(down.astype(np.complex128) - LM.downchirp(sf, BW, WC.rate(decim))).max() < 1e-5
    return down


def _guarded(torch, iq, sps):
    """iq between sps NaN items either side -> (buffer, its bits before the call, pointer to the first real item)"""
    buf = torch.full((2 * (iq.size + 2 * sps),), float("nan"), dtype=torch.float32, device="cuda")
    buf[2 * sps:2 * (sps + iq.size)] = torch.from_numpy(np.ascontiguousarray(iq).view(np.float32)).cuda()
    return buf, buf.view(torch.int32).clone(), buf.data_ptr() + 8 * sps


class _Seen:
    def __init__(self, kernel, sf, decim):
        self.key, self.R, self.worst, self.what = (kernel, sf, decim), WC.LIMIT_R[kernel], 0.0, ""
        assert self.R <= WC.CAP_R

    def see(self, err, U, what):
        e = err / U
        assert e <= self.R, (self.key, what, "err / U", e, "limit", self.R)                # (NaN fails)
        if e > self.worst:
            self.worst, self.what = float(e), "%s, window %s" % (what[-1], what[0])

    def report(self, note=""):
        old = WORST.get(self.key, (0.0, ""))
        WORST[self.key] = max(old, (self.worst, self.what))
        print("\n[window space] %s SF%d D%d%s: worst err / U %.4f (%s), limit %.3g" % (self.key + (note, self.worst, self.what, self.R)))


def _plus_zero(*vals):
    return all(float(v) == 0.0 and math.copysign(1.0, float(v)) > 0.0 for v in vals)


def _bits(vals):
    return np.asarray(vals, dtype=np.float64).tobytes()


def _hold_index(idx, want, gap, mag, U, R, what):
    if WC.index_compared(gap, U, R):
        assert idx == want, (what, idx, want)
    else:
        assert WC.near_max(mag, idx, U, R), (what, idx, want)


def _hold_detect(g, m, s, i):
    for half, name in ((0, "down"), (1, "up")):
        gi, wi, U = g[3 * half:3 * half + 3], m.rec[3 * half:3 * half + 3], m.U[half]
        if U == 0.0:
            assert gi[0] == 0 and _plus_zero(gi[1], gi[2]), (i, name, gi)
            continue
        s.see(abs(math.sqrt(gi[1]) - math.sqrt(wi[1])), U, (i, name, "sqrt(peak)"))
        s.see(abs(math.sqrt(gi[2]) - math.sqrt(wi[2])), U, (i, name, "sqrt(total)"))
        _hold_index(gi[0], wi[0], m.gap[half], m.mag[half], U, s.R, (s.key, i, name))


def _hold_link(g, m, s, i):
    assert g.valid == 1
    if m.U == 0.0:
        assert g.peak_bin == 0 and _plus_zero(g.frac, g.lobe_power, g.total_power, g.peak_power), (i, g.peak_bin, g.frac, g.total_power)
        return
    w = m.rec
    s.see(abs(math.sqrt(g.total_power) - math.sqrt(w.total_power)), m.U, (i, "sqrt(total_power)"))
    s.see(abs(math.sqrt(g.peak_power) - math.sqrt(w.peak_power)), m.U, (i, "sqrt(peak_power)"))
    _hold_index(g.peak_bin, w.peak_bin, m.gap, m.mag, m.U, s.R, (s.key, i))
    if g.peak_bin == w.peak_bin:
        s.see(abs(math.sqrt(g.lobe_power) - math.sqrt(w.lobe_power)), m.U, (i, "sqrt(lobe_power)"))
    if WC.index_compared(m.gap, m.U, s.R):
        bound, _aside = WC.frac_bound(m, s.R)
        assert abs(g.frac - w.frac) <= bound, (s.key, i, g.frac, w.frac, bound)


def _hold_soft(L, k, peak, m, s, i):
    assert L.size == m.L.size
    if m.U == 0.0:
        assert int(k) == 0 and _plus_zero(peak, *L), (i, k, peak, L)
        return
    s.see(abs(float(peak) - m.peak), m.U, (i, "peak"))
    s.see(float(np.abs(L.astype(np.float64) - m.L).max()) / 2.0, m.U, (i, "L / 2"))
    _hold_index(int(k), m.k, m.gap, m.mag, m.U, s.R, (s.key, i))


@pytest.mark.parametrize("kernel,sf,decim", CASES, ids=["%s-sf%d-d%d" % c for c in CASES])
def test_window_spectrum_equals_its_definition(torch_cuda, kernel, sf, decim):
    if (kernel, sf, decim) in REFUSED:
        with pytest.raises(capi.LoraHipError):
            _handle(sf, decim)
        return
    h = _handle(sf, decim)
    down = _table(h, sf, decim)
    st = WC.build(sf, decim, down, link=(kernel == "link"))
    sps, N, n_items = st.sps, st.nbins, st.iq.size
    buf, before, ptr = _guarded(torch_cuda, st.iq, sps)
    s = _Seen(kernel, sf, decim)
    dup = 9                                                                            # the first noise window: listed first and last
    order = [dup] + [i for i in range(WC.N_WINDOWS) if i != dup] + [dup]
    if kernel == "detect":
        got = h.window_stats_device(ptr, n_items, [st.starts[i] for i in order])
        assert _bits(got[0]) == _bits(got[-1]), (got[0], got[-1])
        for g, i in zip(got[:-1], order):
            _hold_detect(g, WC.detect_model(st.iq, st.starts[i], down, N), s, i)
    elif kernel == "soft":
        L, k, peak = h.soft_symbols_device(ptr, n_items, [st.starts[i] for i in order], [WC.soft_reduced(i) for i in order])
        assert L[0].tobytes() == L[-1].tobytes() and int(k[0]) == int(k[-1]) and peak[:1].tobytes() == peak[-1:].tobytes()
        for j, i in enumerate(order[:-1]):
            _hold_soft(L[j], k[j], peak[j], WC.soft_model(st.iq, st.starts[i], down, N, WC.soft_reduced(i)), s, i)
    else:
        frames = [1, 0, 2, 1]                                                          # frame 1 (noise, the tone in noise) first and last
        mets, wins = h.measure_link_device(ptr, n_items, [0], [n_items], [(0, st.header_pos(f)) for f in frames], windows=True)
        assert [m.flags for m in mets] == [7] * 4
        for a, b in zip(wins[0:6], wins[18:24]):
            assert bytes(a) == bytes(b)
        for j, f in enumerate(frames[:-1]):
            for w in range(6):
                i = 6 * f + w
                _hold_link(wins[6 * j + w], WC.link_model(st.window(i), down, N, st.conj(i)), s, i)
    h.close()
    assert torch_cuda.equal(buf.view(torch_cuda.int32), before)
    s.report()


@pytest.mark.parametrize("kernel,sf,decim", [(k, sf, d) for k in ("detect", "soft") for sf, d in ((7, 1), (8, 2))])
def test_grid_stride_loop_past_4096_windows(torch_cuda, kernel, sf, decim):
    """Both kernels launch min(n, 4096) workgroups and loop s += gridDim.x over the same LDS: 4096 + 37 windows, one every 61 items; every window
    past index 4095 and every 16th before it against the definition, and a second call with the last 37 alone - then computed on the first
    trip of the loop - bit-equal."""
    n, tail = 4096 + 37, 37
    h = _handle(sf, decim)
    down = _table(h, sf, decim)
    iq, offs = WC.grid_stream(sf, decim, down, n)
    assert 240_000 < iq.size < 280_000 and offs[-1] + h.sps <= iq.size
    buf, before, ptr = _guarded(torch_cuda, iq, h.sps)
    s = _Seen(kernel, sf, decim)
    check = [i for i in range(n) if i >= 4096 or i % 16 == 0]
    red = [WC.soft_reduced(i) for i in range(n)]
    if kernel == "detect":
        got = h.window_stats_device(ptr, iq.size, offs)
        again = h.window_stats_device(ptr, iq.size, offs[-tail:])
        assert [_bits(g) for g in got[-tail:]] == [_bits(g) for g in again]
        for i in check:
            _hold_detect(got[i], WC.detect_model(iq, offs[i], down, h.nbins), s, i)
    else:
        L, k, peak = h.soft_symbols_device(ptr, iq.size, offs, red)
        L2, k2, peak2 = h.soft_symbols_device(ptr, iq.size, offs[-tail:], red[-tail:])
        assert [a.tobytes() for a in L[-tail:]] == [a.tobytes() for a in L2] and k[-tail:].tobytes() == k2.tobytes() and peak[-tail:].tobytes() == peak2.tobytes()
        for i in check:
            _hold_soft(L[i], k[i], peak[i], WC.soft_model(iq, offs[i], down, h.nbins, red[i]), s, i)
    h.close()
    assert torch_cuda.equal(buf.view(torch_cuda.int32), before)
    s.report(", %d windows" % n)


def test_link_kernel_700_frames(torch_cuda):
    """One workgroup per window, no loop: 700 frames (4200 windows) in one launch at SF7, D = 1; frames 0, 350 and 699 against the definition."""
    sf, decim, n_frames = 7, 1, 700
    h = _handle(sf, decim)
    down = _table(h, sf, decim)
    sps = h.sps
    iq, offs = WC.grid_stream(sf, decim, down, 6 * n_frames, step=sps)
    buf, before, ptr = _guarded(torch_cuda, iq, sps)
    s = _Seen("link", sf, decim)
    hdr = [offs[6 * f] + (25 * sps) // 4 for f in range(n_frames)]
    assert LM.window_starts(hdr[-1], sps) == offs[-6:]
    mets, wins = h.measure_link_device(ptr, iq.size, [0], [iq.size], [(0, p) for p in hdr], windows=True)
    assert h.link_stats()["launches"] == 1 and all(m.flags == 7 for m in mets)
    h.close()
    for f in (0, 350, 699):
        for w in range(6):
            i = 6 * f + w
            _hold_link(wins[i], WC.link_model(iq[offs[i]:offs[i] + sps], down, h.nbins, w >= 4), s, i)
    assert torch_cuda.equal(buf.view(torch_cuda.int32), before)
    s.report(", %d frames" % n_frames)
