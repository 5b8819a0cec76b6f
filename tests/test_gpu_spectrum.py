"""GPU: the spectral scan (include/lora_hip_spectrum.h, csrc/lora_spectrum.hip, capi.Spectrum, lora.spectrum_scanner) against
its float64 definition (gr_lora_amd.spectrum.welch_rows), bit-identical whatever the chunking and the input format, and beside
the gateway on a capture made on the device.

Observed err = max |device - model| / (model row total) over psd, peak and band, worst case per size on an MI355X (bound
4 log2(nfft) 2^-24; every case: profiles/spectrum_model_errors.txt):
    nfft   64: 1.5e-7 (bound 1.43e-6)     nfft  256: 1.6e-7 (bound 1.91e-6)
    nfft 1024: 1.8e-7 (bound 2.38e-6)     nfft 4096: 2.2e-7 (bound 2.86e-6)
"""
import functools
import math
from collections import Counter

import numpy as np
import pytest

import spectrum_cases as sc
from gr_lora_amd import capi, iqformat, lora, spectrum

pytestmark = pytest.mark.gpu

CASES = [(64, 64, 1), (64, 32, 3), (256, 128, 4), (256, 129, 16), (1024, 512, 3), (4096, 4096, 1), (4096, 2048, 2), (4096, 2049, 5)]
INPUTS = ["noise", "tone", "dc"]
ROWS = 11            # rows per stream where 200 k items allow: more than one workgroup, an odd count
MAX_ITEMS = 200000


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU: the HIP path has no CPU fallback")
    return torch


def _bound(nfft):
    return 4.0 * math.log2(nfft) * 2.0 ** -24


def _n_items(nfft, hop, n_avg, rows=ROWS):
    """rows complete rows and part of another one, within MAX_ITEMS."""
    extra = min(n_avg * hop - 1, n_avg * hop // 2 + 17)
    while (rows * n_avg - 1) * hop + nfft + extra > MAX_ITEMS:
        rows -= 1
    assert rows >= 3
    return (rows * n_avg - 1) * hop + nfft + extra


def _bands(nfft):
    """The whole spectrum, one bin, a band around DC, one that is no multiple of a wave and ends on the last bin."""
    return [(0, nfft), (1, 1), (nfft // 2 - 3, 7), (nfft - 37, 37), (nfft // 2 + nfft // 8 - 2, 5)]


@functools.lru_cache(maxsize=None)
def _stream(nfft, hop, n_avg, kind, rows=ROWS):
    """complex64 stream: made once per case, never changed."""
    n = _n_items(nfft, hop, n_avg, rows)
    rng = np.random.default_rng([nfft, hop, n_avg, INPUTS.index(kind)])
    noise = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    if kind == "noise":
        x = noise
    elif kind == "tone":
        x = np.exp(2j * np.pi * (nfft // 8 + 0.37) * np.arange(n) / nfft) + 1e-3 * noise
    else:
        x = (0.5 + 0.25j) + 1e-3 * noise
    x = x.astype(np.complex64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _model(nfft, hop, n_avg, kind, window="hann", rows=ROWS):
    return spectrum.welch_rows(_stream(nfft, hop, n_avg, kind, rows), nfft, hop, n_avg, window, _bands(nfft))


def _handle(nfft, hop, n_avg, window="hann", peak=True, bands=None):
    return capi.Spectrum(1e6, nfft, hop, n_avg, spectrum.window_id(window), peak, _bands(nfft) if bands is None else bands)


@functools.lru_cache(maxsize=None)
def _one_shot(nfft, hop, n_avg, kind, window="hann", rows=ROWS):
    h = _handle(nfft, hop, n_avg, window)
    out = h.work(_stream(nfft, hop, n_avg, kind, rows))
    assert np.array_equal(h.window(), spectrum.window_table(nfft, window))
    h.close()
    for a in out[:3]:
        a.setflags(write=False)
    return out


def _err(dev, model):
    psd, peak, band, _ = dev
    mpsd, mpeak, mband, _ = model
    total = mpsd.sum(axis=1, keepdims=True)
    return max(float((np.abs(a - b) / total).max()) for a, b in ((psd, mpsd), (peak, mpeak), (band, mband)))


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("nfft,hop,n_avg", CASES)
def test_against_the_float64_model(torch_cuda, nfft, hop, n_avg, kind):
    """err <= 4 log2(nfft) 2^-24 of the row total on psd, peak and band: fp32 FFT error growth, doubled for a power.  On noise
    every bin holds about 1 / nfft of the total, so a misplaced bin cannot hide under it; the tone's arg-max is asserted outright."""
    dev, model = _one_shot(nfft, hop, n_avg, kind), _model(nfft, hop, n_avg, kind)
    psd, peak, band, first = dev
    rows = spectrum.output_rows(_stream(nfft, hop, n_avg, kind).size, nfft, hop, n_avg)
    assert psd.shape == (rows, nfft) == model[0].shape and peak.shape == psd.shape and band.shape == (rows, len(_bands(nfft))) and first == 0
    assert psd.dtype == np.float32 and np.isfinite(psd).all()
    err = _err(dev, model)
    print("spectrum err nfft %d hop %d n_avg %d %s: %.3g (bound %.3g)" % (nfft, hop, n_avg, kind, err, _bound(nfft)))
    assert err <= _bound(nfft)
    if kind == "tone":
        assert np.all(psd.argmax(axis=1) == nfft // 2 + nfft // 8) and np.all(peak.argmax(axis=1) == nfft // 2 + nfft // 8)
    if kind == "dc":
        assert np.all(psd.argmax(axis=1) == nfft // 2)


def test_rect_window(torch_cuda):
    dev, model = _one_shot(256, 128, 4, "noise", "rect"), _model(256, 128, 4, "noise", "rect")
    err = _err(dev, model)
    print("spectrum err nfft 256 rect: %.3g (bound %.3g)" % (err, _bound(256)))
    assert err <= _bound(256)
    # Parseval on the device's own row: the mean power of unit noise
    assert abs(float(dev[0].sum(axis=1).mean()) - 1.0) < 0.05


@pytest.mark.parametrize("nfft", [128, 512, 2048])
def test_sizes_with_a_radix_2_stage(torch_cuda, nfft):
    """log2 nfft odd: the transform ends in a radix-2 stage; the tone lands where it must."""
    dev, model = _one_shot(nfft, nfft // 2, 2, "tone", rows=5), _model(nfft, nfft // 2, 2, "tone", rows=5)
    err = _err(dev, model)
    print("spectrum err nfft %d: %.3g (bound %.3g)" % (nfft, err, _bound(nfft)))
    assert err <= _bound(nfft) and np.all(dev[0].argmax(axis=1) == nfft // 2 + nfft // 8)


def _feed(h, x, sizes):
    """x in chunks of the given sizes (the last size repeats) -> rows as one-shot returns them, and the first_row of every call
    checked against the rows emitted so far."""
    parts, pos, i, emitted = [], 0, 0, 0
    while pos < x.size:
        c = sizes[min(i, len(sizes) - 1)]
        want = h.output_rows(min(c, x.size - pos))
        psd, peak, band, first = h.work(x[pos:pos + c])
        assert first == emitted and psd.shape[0] == want
        emitted += psd.shape[0]
        if psd.shape[0]:
            parts.append((psd, peak, band))
        pos += c
        i += 1
    return tuple(np.concatenate([p[j] for p in parts]) for j in range(3)), emitted


def _same(got, want):
    return all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, want[:3]))


@pytest.mark.parametrize("nfft,hop,n_avg", [(256, 129, 16), (4096, 2049, 5)])
def test_chunking_is_bit_identical(torch_cuda, nfft, hop, n_avg):
    """Chunks of hop - 1, nfft - 1, nfft, 7919 and random sizes give the one-shot rows bit for bit (psd, peak, band, first_row), and
    again after reset(); chunks of 1 (one call per item) on the whole (256, 129, 16) stream, about 24 k calls, and on the first
    three rows of the (4096, 2049, 5) stream, 33 k calls of its 120 k: the flip of the carried state, the carried samples and a row
    boundary, within the seconds a test may take."""
    x = _stream(nfft, hop, n_avg, "noise")
    want = _one_shot(nfft, hop, n_avg, "noise")
    rng = np.random.default_rng(nfft)
    random_sizes = [int(v) for v in rng.integers(1, 3 * nfft, 4000)]
    h = _handle(nfft, hop, n_avg)
    for sizes in ([hop - 1], [nfft - 1], [nfft], [7919], random_sizes, [1, hop, 1, 2 * nfft + 1, 3, 50000]):
        got, emitted = _feed(h, x, sizes)
        assert emitted == want[0].shape[0] and _same(got, want), "chunks of %s" % (sizes[:6],)
        h.reset()
    rows_1 = want[0].shape[0] if nfft == 256 else 3
    short = x if nfft == 256 else x[:(rows_1 * n_avg - 1) * hop + nfft + 5]
    got, emitted = _feed(h, short, [1])
    assert emitted == rows_1 and _same(got, [a[:rows_1] for a in want[:3]])
    h.close()


def test_a_call_too_short_for_a_segment_loses_nothing(torch_cuda):
    nfft, hop, n_avg = 256, 129, 16
    x = _stream(nfft, hop, n_avg, "noise")
    want = _one_shot(nfft, hop, n_avg, "noise")
    h = _handle(nfft, hop, n_avg)
    assert h.work(x[:0])[0].shape[0] == 0 and h.work(x[:100])[0].shape[0] == 0 and h.work(x[100:255])[0].shape[0] == 0
    got = h.work(x[255:])
    assert got[3] == 0 and _same(got, want)
    h.close()


def test_output_rows_follows_the_definition(torch_cuda):
    for nfft, hop, n_avg, chunks in [(64, 32, 3, [127, 1, 95, 1, 1000, 5]), (4096, 2049, 5, [4095, 8196, 1, 12000, 7919, 100000])]:
        h = _handle(nfft, hop, n_avg, peak=False, bands=[])
        total, seen = 0, 0
        for c in chunks:
            rows = spectrum.output_rows(total + c, nfft, hop, n_avg) - seen
            assert h.output_rows(c) == rows
            psd, peak, band, first = h.work(np.zeros(c, dtype=np.complex64))
            assert psd.shape[0] == rows and peak is None and band is None and (first == seen)
            total, seen = total + c, seen + rows
        h.reset()
        assert h.output_rows(nfft + (n_avg - 1) * hop) == 1 and h.output_rows(nfft + (n_avg - 1) * hop - 1) == 0
        h.close()


def _raw(fmt, n, seed):
    info = np.iinfo(iqformat.DTYPES[fmt])
    return np.random.default_rng(seed).integers(info.min, info.max + 1, 2 * n, dtype=np.int64).astype(iqformat.DTYPES[fmt])


@pytest.mark.parametrize("device_input", [False, True])
@pytest.mark.parametrize("fmt_a,scale_a,fmt_b,scale_b", [
    (iqformat.SC16, 0, iqformat.CU8, 0),
    (iqformat.SC8, 1.0 / 100.0, iqformat.SC16, 3.0e-5),
    (iqformat.CU8, 0.013, iqformat.SC8, 0),
])
def test_integer_formats_give_the_bits_of_the_cf32_call(torch_cuda, fmt_a, scale_a, fmt_b, scale_b, device_input):
    """Random full-range integers, default and explicit scale, the format changing between the two calls of one stream; host
    arrays through capi.Spectrum, torch device tensors through lora.spectrum_scanner."""
    nfft, hop, n_avg = 256, 129, 3
    n1, n2 = 5003, 6001
    qa, qb = _raw(fmt_a, n1, 1), _raw(fmt_b, n2, 2)
    xa, xb = iqformat.to_cf32(qa, fmt_a, scale_a), iqformat.to_cf32(qb, fmt_b, scale_b)
    bins = _bands(nfft)
    if not device_input:
        ref, dut = _handle(nfft, hop, n_avg), _handle(nfft, hop, n_avg)
        want = [ref.work(xa), ref.work(xb)]
        got = [dut.work_raw(qa, fmt_a, scale_a), dut.work_raw(qb, fmt_b, scale_b)]
        for g, w in zip(got, want):
            assert g[3] == w[3] and g[0].shape[0] > 0 and _same(g, w)
        ref.close()
        dut.close()
        return
    torch = torch_cuda
    hz = [((a - nfft // 2) * 1e6 / nfft, (a + n - nfft // 2) * 1e6 / nfft) for a, n in bins]
    ref, dut = (lora.spectrum_scanner(1e6, nfft, hop, n_avg, peak=True, bands=hz) for _ in range(2))
    assert ref.band_bins == bins
    want = [ref.work(torch.from_numpy(xa).cuda()), ref.work(torch.from_numpy(xb.view(np.float32).copy()).cuda())]    # complex64, then float32 interleaved
    got = [dut.work(torch.from_numpy(qa).cuda(), scale=scale_a), dut.work(torch.from_numpy(qb.reshape(-1, 2)).cuda(), scale=scale_b)]
    host = _handle(nfft, hop, n_avg)
    href = [host.work(xa), host.work(xb)]
    for g, w, hr in zip(got, want, href):
        assert len(g) > 0 and np.array_equal(g.first_sample, w.first_sample) and g.first_sample[0] == hr[3] * n_avg * hop
        assert _same((g.psd, g.peak, g.band), (w.psd, w.peak, w.band)) and _same((g.psd, g.peak, g.band), hr)
    with pytest.raises(TypeError):
        ref.work(torch.from_numpy(xa).cuda(), scale=0.5)
    for s in (ref, dut, host):
        s.close()


def test_raw_argument_checks(torch_cuda):
    """An unknown format, an unusable scale and a pointer not aligned to its component are refused, and consume nothing."""
    C = capi.C
    h = _handle(256, 128, 4)
    q = _raw(iqformat.SC16, 4097, 3)
    psd, peak, band = h._host_out(64)
    n, first = C.c_size_t(0), C.c_uint64(0)
    for ptr, fmt, scale in ((q.ctypes.data, 7, 0.0), (q.ctypes.data, iqformat.SC16, float("inf")), (q.ctypes.data, iqformat.SC16, -1.0),
                            (q.ctypes.data + 1, iqformat.SC16, 0.0)):
        st = h.L.lora_hip_spectrum_work_raw(h.h, ptr, 4096, fmt, scale, psd.ctypes.data, peak.ctypes.data, band.ctypes.data, 256, 64, C.byref(n), C.byref(first))
        assert st == -6
    got = h.work_raw(q[:8192])
    assert got[0].shape[0] == spectrum.output_rows(4096, 256, 128, 4) and got[3] == 0       # (nothing was consumed by the refused calls)
    h.close()


def test_same_stream_twice_gives_equal_bits(torch_cuda):
    nfft, hop, n_avg = 1024, 512, 3
    x = _stream(nfft, hop, n_avg, "noise")
    outs = []
    for _ in range(2):
        h = _handle(nfft, hop, n_avg)
        outs.append(_feed(h, x, [7919])[0])
        h.close()
    assert _same(outs[0], outs[1]) and _same(outs[0], _one_shot(nfft, hop, n_avg, "noise"))


def test_overflow_leaves_the_stream_untouched(torch_cuda):
    nfft, hop, n_avg = 256, 129, 16
    x = _stream(nfft, hop, n_avg, "noise")
    want = _one_shot(nfft, hop, n_avg, "noise")
    rows = want[0].shape[0]
    h = _handle(nfft, hop, n_avg)
    cut = 3000                                       # (inside row 1)
    head = h.work(x[:cut])
    assert head[0].shape[0] == 1
    for max_rows in (0, rows - 2):
        with pytest.raises(capi.LoraHipError) as e:
            h.work(x[cut:], max_rows=max_rows)
        assert e.value.status == -7
        assert h.output_rows(x.size - cut) == rows - 1
    tail = h.work(x[cut:], max_rows=rows + 5)        # room to spare
    assert tail[3] == 1 and _same([np.concatenate([a, b]) for a, b in zip(head[:3], tail[:3])], want)
    # pointer rules: a peak buffer without the flag, a band buffer without bands
    plain = _handle(nfft, hop, n_avg, peak=False, bands=[])
    n, first = capi.C.c_size_t(0), capi.C.c_uint64(0)
    buf = np.zeros((4, nfft), dtype=np.float32)
    xs = np.ascontiguousarray(x[:2000])
    for peak_p, band_p in ((buf.ctypes.data, None), (None, buf.ctypes.data)):
        st = plain.L.lora_hip_spectrum_work(plain.h, xs.ctypes.data, xs.size, buf.ctypes.data, peak_p, band_p, nfft, 4, capi.C.byref(n), capi.C.byref(first))
        assert st == -6
    st = plain.L.lora_hip_spectrum_work(plain.h, xs.ctypes.data, 2500, buf.ctypes.data, None, None, nfft - 1, 4, capi.C.byref(n), capi.C.byref(first))
    assert st == -6 and n.value == 1                 # row_stride < nfft with a row to write
    assert plain.work(x[:2500])[0].shape[0] == 1     # (still at sample 0)
    plain.close()
    h.close()


def test_beside_the_gateway_on_a_device_capture(torch_cuda):
    """tests/spectrum_cases.py's two emitters made by lora.traffic_synthesizer as sc16 (full scale 2^14); the same items go to
    spectrum_scanner.for_grid, as the device tensor, and to gateway_receiver, as its host copy (gateway_receiver.work takes numpy).  The band powers are the model's within the bound and mean what the CPU test
    says; the frames decoded are the same with and without the scanner."""
    torch = torch_cuda
    n = MAX_ITEMS
    tx = lora.traffic_synthesizer(sc.FS)
    tails = [tx.add_frame(pl, 7, 4, sc.BANDWIDTH, start, f, amplitude=a)[0] for pl, start, f, a in sc.EMITTERS]
    y = tx.generate(n, fmt="sc16", full_scale=2.0 ** 14)
    tx.close()
    host = y.cpu().numpy()

    def decode(with_scanner):
        rx = lora.gateway_receiver(sc.FS, 0.0, sc.GRID_OFFSET, sc.N_GRID, sc.CHANNELS, sc.BANDWIDTH, 7, False, 4, True, decimation=2)
        seen, recs = [], []
        rx.subscribe("channel_frames", seen.append)
        scan = lora.spectrum_scanner.for_grid(sc.FS, sc.GRID_OFFSET, sc.N_GRID, sc.CHANNELS, sc.BANDWIDTH, nfft=sc.NFFT, hop=sc.HOP, n_avg=sc.N_AVG) \
            if with_scanner else None
        for lo in range(0, n, 65536):
            if scan is not None:
                recs.append(scan.work(y[2 * lo:2 * (lo + 65536)], scale=2.0 ** -14))
            rx.work(host[2 * lo:2 * (lo + 65536)], scale=2.0 ** -14)
        rx.stop()
        rx.close()
        if scan is not None:
            scan.close()
        return Counter((int(k), blob[15:]) for k, blob in seen), recs

    alone, _ = decode(False)
    beside, recs = decode(True)
    assert alone == beside == Counter([(-2, tails[0]), (1, tails[1])])
    band = np.concatenate([r.band for r in recs])
    first = np.concatenate([r.first_sample for r in recs])
    mpsd, _, mband, mfirst = spectrum.welch_rows(iqformat.to_cf32(host, scale=2.0 ** -14), sc.NFFT, sc.HOP, sc.N_AVG, bands=sc.bands())
    assert np.array_equal(first, mfirst) and recs[0].band.shape[1] == len(sc.CHANNELS)
    inside = sc.rows_inside_all(first)
    total = mpsd.sum(axis=1, keepdims=True)
    err = float((np.abs(band[inside] - mband[inside]) / total[inside]).max())
    print("spectrum err beside the gateway: %.3g (bound %.3g)" % (err, _bound(sc.NFFT)))
    assert err <= _bound(sc.NFFT)
    quiet = total[:, 0] == 0.0                                            # (rows of silence: the device must read exactly 0 there)
    assert np.all(band[quiet] == 0.0) and quiet[sc.rows_before_any(first)].all()
    busy = ~quiet
    assert float((np.abs(band[busy] - mband[busy]) / total[busy]).max()) <= _bound(sc.NFFT)
    db = spectrum.to_dbfs(band[inside])
    assert np.abs(db[:, sc.STRONG]).max() <= 0.5 and np.abs(db[:, sc.WEAK] - 20 * np.log10(0.25)).max() <= 0.5
    idle = [c for c in range(len(sc.CHANNELS)) if c not in (sc.STRONG, sc.WEAK)]
    assert (db[:, idle] - db[:, [sc.STRONG]]).max() <= -25.0


def test_scan_tool_on_the_device_prints_what_the_model_prints(torch_cuda, tmp_path):
    """tools/spectrum_scan.py without --model (lora.spectrum_scanner fed the file's int16 items in chunks) against --model on
    the same SigMF capture: the same rows, and every band's mean and maximum within the bound above of a row's total.  The tool
    prints no totals: a row's total is at most 1.1 times the sum of the bands' maxima (what lies between the bands of this capture
    is leakage, 30 dB down)."""
    import os
    import sys
    from gr_lora_amd import sigmf
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    try:
        import spectrum_scan
    finally:
        sys.path.pop(0)
    base = str(tmp_path / "two_emitters")
    sigmf.write_trace(base, sc.capture()[:40000], sc.FS, 868.1e6, 868.1e6, 7, "4/8", sc.BANDWIDTH, 8, True, False, "", 1, datatype="ci16_le",
                      full_scale=16000.0)
    argv = [base, "--nfft", str(sc.NFFT), "--hop", str(sc.HOP), "--n-avg", str(sc.N_AVG), "--grid=%g:%d:%d" % (sc.GRID_OFFSET, sc.N_GRID, sc.BANDWIDTH),
            "--channels=%d:%d" % (sc.CHANNELS[0], sc.CHANNELS[-1]), "--chunk", "7919"]
    ap = spectrum_scan.parser()
    dev, model = spectrum_scan.scan(ap.parse_args(argv)), spectrum_scan.scan(ap.parse_args(argv + ["--model"]))
    assert dev["source"] == "device" and model["source"] == "model" and dev["rows"] == model["rows"] > 0
    tol = _bound(sc.NFFT) * 1.1 * sum(10.0 ** (m["max_dbfs"] / 10.0) for m in model["bands"])
    for d, m in zip(dev["bands"], model["bands"]):
        assert (d["first_bin"], d["n_bins"]) == (m["first_bin"], m["n_bins"])
        for key in ("mean_dbfs", "max_dbfs"):
            assert abs(10.0 ** (d[key] / 10.0) - 10.0 ** (m[key] / 10.0)) <= tol, (key, d, m)
    assert abs(dev["bands"][sc.STRONG]["max_dbfs"] - 20 * np.log10(16000.0 / 32768.0)) <= 0.5
