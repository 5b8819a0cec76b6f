"""GPU: the rational resampler (include/lora_hip_resampler.h, csrc/lora_resampler.hip, capi.Resampler, lora.rational_resampler)
against its float64 definition (gr_lora_amd.resampler.resample), bit-identical whatever the chunking and the input format, and in
front of the gateways on a capture at 2.4 Msps.

The model tolerance is |device - model| <= (Q + 2) 2^-24 bound[m] + 1e-30 per component, bound[m] = sum_j |h[p + j L]| |x[n0 - j]|:
the rounding bound of a Q-term fp32 sum in any order, with or without fused multiply-add.  Observed maxima of err / tolerance
on an MI355X (every case: DESIGN.md 4.16, profiles/resampler_bench.txt): 0.07 .. 0.18 where Q is 33 .. 77, 0.002 .. 0.024 where Q is 513 .. 1021.
"""
import functools
import os
import socket
import sys
from collections import Counter

import numpy as np
import pytest

import spectrum_cases as sc
from gr_lora_amd import capi, iqformat, lora, resampler, sigmf, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (L, M, Z): the issue's ten ratios with the default design, and two deep decimations that take the smaller tiles of the plan
CASES = [(1, 1, 16), (1, 2, 16), (3, 1, 16), (5, 6, 16), (6, 5, 16), (5, 12, 16), (125, 128, 16), (125, 256, 16), (512, 511, 16), (1, 31, 16),
         (1, 64, 4), (1, 255, 2)]
INPUTS = ["noise", "tone"]
N_ITEMS = 100003                  # odd, several workgroups in every case; the deepest decimation takes MAX_ITEMS
MAX_ITEMS = 200000
SMOKE_PAYLOADS = [bytes.fromhex("deadbeef"), b"MI355X LoRa smoke", bytes(range(32))]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU: the HIP path has no CPU fallback")
    return torch


def _n_items(L, M):
    return MAX_ITEMS if M >= 100 * L else N_ITEMS


@functools.lru_cache(maxsize=None)
def _stream(L, M, kind):
    """complex64 stream: made once per case, never changed."""
    n = _n_items(L, M)
    rng = np.random.default_rng([L, M, INPUTS.index(kind)])
    noise = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    if kind == "noise":
        x = noise
    else:
        x = np.exp(2j * np.pi * 0.3 * 0.5 * min(1.0, L / M) * np.arange(n)) + 1e-3 * noise
    x = x.astype(np.complex64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _model(L, M, Z, kind):
    y, bound = resampler.resample(_stream(L, M, kind), L, M, resampler.design(L, M, Z))
    y.setflags(write=False)
    bound.setflags(write=False)
    return y, bound


@functools.lru_cache(maxsize=None)
def _one_shot(L, M, Z, kind):
    h = capi.Resampler(L, M, Z)
    y, first = h.work(_stream(L, M, kind))
    assert first == 0
    h.close()
    y.setflags(write=False)
    return y


def _bits(y):
    return np.ascontiguousarray(y).view(np.uint32)


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("L,M,Z", CASES)
def test_against_the_float64_model(torch_cuda, L, M, Z, kind):
    x = _stream(L, M, kind)
    h = capi.Resampler(L, M, Z)
    taps = h.taps()
    l, m, Q = h.ratio()
    assert (l, m, Q) == (L, M, resampler.taps_per_output(L, M, Z)) and h.delay() == resampler.delay(L, M, Z)
    assert taps.dtype == np.float32 and np.array_equal(_bits(taps), _bits(resampler.design(L, M, Z)))
    assert h.output_items(x.size) == resampler.output_items(x.size, L, M)
    y, first = h.work(x)
    h.close()
    want, bound = _model(L, M, Z, kind)
    assert y.shape == want.shape == (resampler.output_items(x.size, L, M),) and y.dtype == np.complex64 and first == 0
    tol = (Q + 2) * 2.0 ** -24 * bound + 1e-30
    er, ei = np.abs(y.real.astype(np.float64) - want.real), np.abs(y.imag.astype(np.float64) - want.imag)
    worst = max(float((er / tol).max()), float((ei / tol).max()))
    print("resampler %d/%d Z %d %s: Q %d, max err / tolerance %.3g" % (L, M, Z, kind, Q, worst))
    assert np.all(er <= tol) and np.all(ei <= tol)
    assert np.array_equal(_bits(y), _bits(_one_shot(L, M, Z, kind)))


def test_the_cases_cover_every_tile_of_the_plan(torch_cuda):
    """lora_hip_resampler_get_plan: tiles of 256, 128 and 64 outputs, one and several tiles per workgroup, an odd row stride and
    LDS inside what a workgroup can have."""
    plans = {}
    for L, M, Z in CASES:
        h = capi.Resampler(L, M, Z)
        tile, per_group, stride, lds = h.plan()
        Q = h.ratio()[2]
        h.close()
        plans[(L, M, Z)] = (tile, per_group)
        assert stride % 2 == 1 and stride >= Q and lds <= 160 * 1024 and 1 <= per_group <= 32
        span = ((tile - 1) * M + L - 1) // L + Q
        assert lds == 4 * ((L * stride + 1) // 2 * 2) + 8 * span
    print("resampler plans (tile, tiles per workgroup): %s" % (plans,))
    assert len(set(plans.values())) >= 2
    assert {t for t, _ in plans.values()} == {256, 128, 64}
    assert min(g for _, g in plans.values()) == 1 and max(g for _, g in plans.values()) > 1


@pytest.mark.parametrize("L,M", [(5, 6), (1, 31)])
def test_zeros_in_give_exact_zeros_out(torch_cuda, L, M):
    h = capi.Resampler(L, M)
    y, _ = h.work(np.zeros(20001, dtype=np.complex64))
    h.close()
    assert y.size == resampler.output_items(20001, L, M) and not _bits(y).any()       # (+0, not -0)


def _feed_device(torch, h, x, sizes, limit=None):
    """x (a device tensor) in chunks of the given sizes (the last size repeats) through run_device, the outputs appended on the
    device; first_out and output_items of every call are checked against the outputs emitted so far."""
    n_total = x.numel() if limit is None else limit
    L, M, _ = h.ratio()
    out = torch.zeros(resampler.output_items(n_total, L, M) + 1, dtype=torch.complex64, device=x.device)
    base_in, base_out = x.data_ptr(), out.data_ptr()
    pos, i, emitted = 0, 0, 0
    while pos < n_total:
        c = min(sizes[min(i, len(sizes) - 1)], n_total - pos)
        want = resampler.output_items(pos + c, L, M) - emitted
        assert h.output_items(c) == want
        got, first = h.run_device(base_in + 8 * pos, c, base_out + 8 * emitted, want)
        assert got == want and first == emitted
        emitted += got
        pos += c
        i += 1
    return out[:emitted].cpu().numpy()


def _feed_host(h, x, sizes):
    parts, pos, i, emitted = [], 0, 0, 0
    while pos < x.size:
        c = sizes[min(i, len(sizes) - 1)]
        want = h.output_items(min(c, x.size - pos))
        y, first = h.work(x[pos:pos + c])
        assert first == emitted and y.size == want
        emitted += y.size
        parts.append(y)
        pos += c
        i += 1
    return np.concatenate(parts)


@pytest.mark.parametrize("L,M", [(5, 12), (125, 128)])
def test_chunking_is_bit_identical(torch_cuda, L, M):
    """Chunks of Q - 2, Q - 1, Q, 7919, 4000 random sizes in 1 .. 3 Q and [1, M, 1, 2 Q + 1, 3, 50000] give the one-shot stream bit
    for bit, with first_out and output_items of every call, and again after reset(); chunks of 1 over the first 20 000 items."""
    torch = torch_cuda
    x = _stream(L, M, "noise")
    want = _one_shot(L, M, 16, "noise")
    xd = torch.from_numpy(np.array(x)).cuda()
    h = capi.Resampler(L, M)
    Q = h.ratio()[2]
    rng = np.random.default_rng(L * 1000 + M)
    random_sizes = [int(v) for v in rng.integers(1, 3 * Q + 1, 4000)]
    lists = ([Q - 2], [Q - 1], [Q], [7919], random_sizes, [1, M, 1, 2 * Q + 1, 3, 50000])
    for _ in range(2):
        for sizes in lists:
            got = _feed_device(torch, h, xd, sizes)
            assert np.array_equal(_bits(got), _bits(want)), "chunks of %s" % (sizes[:6],)
            h.reset()
    got = _feed_host(h, x, [7919])
    assert np.array_equal(_bits(got), _bits(want))
    h.reset()
    got = _feed_device(torch, h, xd, [1], limit=20000)
    assert np.array_equal(_bits(got), _bits(want[:resampler.output_items(20000, L, M)]))
    h.close()


@pytest.mark.parametrize("L,M", [(5, 12), (125, 256), (6, 5)])
def test_short_calls_lose_nothing(torch_cuda, L, M):
    """Calls of 0 items and calls shorter than Q - 1 (the carried items shift) emit what the definition says, and the stream that
    follows is the one-shot stream."""
    x = _stream(L, M, "noise")
    want = _one_shot(L, M, 16, "noise")
    h = capi.Resampler(L, M)
    Q = h.ratio()[2]
    sizes = [0, 5, 0, 1, Q - 2, 3, 0, 2, Q - 1, 1, 0]
    parts, pos = [], 0
    for c in sizes + [x.size - sum(sizes)]:
        n_before = resampler.output_items(pos, L, M)
        assert h.output_items(c) == resampler.output_items(pos + c, L, M) - n_before
        y, first = h.work(x[pos:pos + c])
        assert first == n_before and y.size == resampler.output_items(pos + c, L, M) - n_before
        parts.append(y)
        pos += c
    assert h.work(x[:0])[0].size == 0
    h.close()
    assert np.array_equal(_bits(np.concatenate(parts)), _bits(want))


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
    """Random full-range integers, default and explicit scale, the format changing between the two calls of one stream (the second
    call shorter than Q - 1 in one more pair of calls); host arrays through capi.Resampler, torch device tensors through
    lora.rational_resampler."""
    n1, n2, n3 = 5003, 6001, 17
    qa, qb, qc = _raw(fmt_a, n1, 1), _raw(fmt_b, n2, 2), _raw(fmt_a, n3, 3)
    xa, xb, xc = iqformat.to_cf32(qa, fmt_a, scale_a), iqformat.to_cf32(qb, fmt_b, scale_b), iqformat.to_cf32(qc, fmt_a, scale_a)
    if not device_input:
        ref, dut = capi.Resampler(5, 6), capi.Resampler(5, 6)
        want = [ref.work(xa), ref.work(xb), ref.work(xc), ref.work(xb)]
        got = [dut.work_raw(qa, fmt_a, scale_a), dut.work_raw(qb, fmt_b, scale_b), dut.work_raw(qc, fmt_a, scale_a), dut.work_raw(qb.reshape(-1, 2), fmt_b, scale_b)]
        for g, w in zip(got, want):
            assert g[1] == w[1] and g[0].size == w[0].size > 0 and np.array_equal(_bits(g[0]), _bits(w[0]))
        ref.close()
        dut.close()
        return
    torch = torch_cuda
    ref, dut = lora.rational_resampler(2.4e6, 2e6), lora.rational_resampler(2.4e6, 2e6)
    assert (ref.interpolation, ref.decimation, ref.out_rate, ref.delay) == (5, 6, 2e6, 16.0)
    want = [ref.work(torch.from_numpy(xa).cuda()), ref.work(torch.from_numpy(xb.view(np.float32).copy()).cuda()),     # complex64, then float32 interleaved
            ref.work(torch.from_numpy(xc).cuda()), ref.work(xb)]                                                        # ... and a host array
    got = [dut.work(torch.from_numpy(qa).cuda(), scale=scale_a), dut.work(torch.from_numpy(qb.reshape(-1, 2)).cuda(), scale=scale_b),
           dut.work(torch.from_numpy(qc).cuda(), scale=scale_a), dut.work(qb, scale=scale_b)]
    host = capi.Resampler(5, 6)
    href = [host.work(xa)[0], host.work(xb)[0], host.work(xc)[0], host.work(xb)[0]]
    for i, (g, w, hr) in enumerate(zip(got, want, href)):
        assert (i == 3) == isinstance(g, np.ndarray) == isinstance(w, np.ndarray)
        if i < 3:
            assert g.is_cuda and g.dtype == torch.complex64 and w.is_cuda
            g, w = g.cpu().numpy(), w.cpu().numpy()
        assert g.size == hr.size > 0 and np.array_equal(_bits(g), _bits(w)) and np.array_equal(_bits(g), _bits(hr))
    with pytest.raises(TypeError):
        ref.work(torch.from_numpy(xa).cuda(), scale=0.5)
    for s in (ref, dut, host):
        s.close()


def test_raw_argument_checks(torch_cuda):
    """An unknown format, an unusable scale and a pointer not aligned to its component are refused, and consume nothing."""
    C = capi.C
    h = capi.Resampler(5, 6)
    q = _raw(iqformat.SC16, 4097, 3)
    out = np.zeros(8192, dtype=np.complex64)
    n, first = C.c_size_t(0), C.c_uint64(0)
    for ptr, fmt, scale in ((q.ctypes.data, 7, 0.0), (q.ctypes.data, iqformat.SC16, float("inf")), (q.ctypes.data, iqformat.SC16, -1.0),
                            (q.ctypes.data + 1, iqformat.SC16, 0.0)):
        st = h.L.lora_hip_resampler_work_raw(h.h, ptr, 4096, fmt, scale, out.ctypes.data, out.size, C.byref(n), C.byref(first))
        assert st == -6
    y, first_out = h.work_raw(q[:8192])
    assert y.size == resampler.output_items(4096, 5, 6) and first_out == 0            # (nothing was consumed by the refused calls)
    ref = capi.Resampler(5, 6)
    assert np.array_equal(_bits(y), _bits(ref.work(iqformat.to_cf32(q[:8192]))[0]))
    ref.close()
    h.close()


def test_overflow_leaves_the_stream_untouched(torch_cuda):
    L, M = 125, 128
    x = _stream(L, M, "noise")
    want = _one_shot(L, M, 16, "noise")
    h = capi.Resampler(L, M)
    cut = 3001
    head, first = h.work(x[:cut])
    n_head, n_tail = resampler.output_items(cut, L, M), want.size - resampler.output_items(cut, L, M)
    assert first == 0 and head.size == n_head
    for max_out in (0, n_tail - 1):
        with pytest.raises(capi.LoraHipError) as e:
            h.work(x[cut:], max_out=max_out)
        assert e.value.status == -7
        assert h.output_items(x.size - cut) == n_tail
    n, first_c = capi.C.c_size_t(0), capi.C.c_uint64(0)
    xs = np.ascontiguousarray(x[cut:])
    st = h.L.lora_hip_resampler_work(h.h, xs.ctypes.data, xs.size, None, 5, capi.C.byref(n), capi.C.byref(first_c))
    assert st == -7 and n.value == n_tail and first_c.value == n_head              # (*n_out is set)
    tail, first = h.work(x[cut:], max_out=n_tail + 5)                                # room to spare
    assert first == n_head and np.array_equal(_bits(np.concatenate([head, tail])), _bits(want))
    h.close()


def test_same_stream_twice_gives_equal_bits(torch_cuda):
    L, M = 125, 256
    x = _stream(L, M, "noise")
    outs = []
    for _ in range(2):
        h = capi.Resampler(L, M)
        outs.append(_feed_host(h, x, [7919]))
        h.close()
    assert np.array_equal(_bits(outs[0]), _bits(outs[1])) and np.array_equal(_bits(outs[0]), _bits(_one_shot(L, M, 16, "noise")))


@functools.lru_cache(maxsize=None)
def _capture_at_2400k():
    """tests/spectrum_cases.py's two emitters at 2 Msps plus 20 000 zeros, taken up 6/5 to 2.4 Msps by the float64 model."""
    x = np.concatenate([sc.capture(), np.zeros(20000, dtype=np.complex128)])
    hi, _ = resampler.resample(x, 6, 5, resampler.design(6, 5))
    hi.setflags(write=False)
    return x, hi


def _tails():
    return [synth.expected_frame_tail(f.payload, f.cfg, f.crc_bytes) for f in sc.frames()]


def test_in_front_of_the_multi_sf_gateway_on_the_device(torch_cuda):
    """The capture at 2.4 Msps as sc16 (full scale 2^14), in 65 536-item chunks as device tensors through rational_resampler(2.4e6,
    2e6) into multi_sf_gateway_receiver without leaving the device: the frames of the gateway fed the 2 Msps capture directly."""
    torch = torch_cuda
    x, hi = _capture_at_2400k()
    q = iqformat.quantize(hi, "sc16", 2.0 ** 14)

    def gateway():
        rx = lora.multi_sf_gateway_receiver(2e6, 0, 0.0, sc.N_GRID, sc.CHANNELS, sc.BANDWIDTH, sfs=(7,), decimation=2)
        seen = []
        rx.subscribe("channel_frames", seen.append)
        return rx, seen

    rx, direct = gateway()
    x32 = x.astype(np.complex64)
    for lo in range(0, x32.size, 65536):
        rx.work(x32[lo:lo + 65536])
    rx.stop()
    rx.close()
    rx, seen = gateway()
    rr = lora.rational_resampler(2.4e6, 2e6)
    n_out = 0
    for lo in range(0, hi.size, 65536):
        y = rr.work(torch.from_numpy(q[2 * lo:2 * (lo + 65536)]).cuda(), scale=2.0 ** -14)
        assert y.is_cuda and y.dtype == torch.complex64
        n_out += y.numel()
        rx.work(y)
    rx.stop()
    rx.close()
    rr.close()
    assert n_out == resampler.output_items(hi.size, 5, 6)
    tails = _tails()
    want = Counter([(-2, tails[0]), (1, tails[1])])
    assert Counter((int(k), blob[15:]) for k, blob in seen) == want == Counter((int(k), blob[15:]) for k, blob in direct)


def test_in_front_of_the_gateway_as_cu8_host_arrays(torch_cuda):
    """The same capture as cu8 (1.3 mapped to full scale, scale given accordingly) through gateway_receiver with host arrays."""
    _, hi = _capture_at_2400k()
    q = iqformat.quantize(hi, "cu8", 127.5 / 1.3)
    rx = lora.gateway_receiver(2e6, 0.0, 0.0, sc.N_GRID, sc.CHANNELS, sc.BANDWIDTH, 7, False, 4, True, decimation=2)
    seen = []
    rx.subscribe("channel_frames", seen.append)
    rr = lora.rational_resampler(2.4e6, 2e6)
    for lo in range(0, hi.size, 65536):
        y = rr.work(q[2 * lo:2 * (lo + 65536)], scale=1.3 / 127.5)
        assert isinstance(y, np.ndarray) and y.dtype == np.complex64
        rx.work(y)
    rx.stop()
    rx.close()
    rr.close()
    tails = _tails()
    assert Counter((int(k), blob[15:]) for k, blob in seen) == Counter([(-2, tails[0]), (1, tails[1])])


def test_receive_file_app_resamples_a_capture_at_2400k(torch_cuda, tmp_path):
    """apps/lora_receive_file_nogui.py --resample-to 1000000 on a SigMF file written at 2.4 Msps (ci16_le) from the smoke trace taken
    up 12/5 by the model: the three smoke frames come back over UDP."""
    sys.path.insert(0, os.path.join(ROOT, "apps"))
    try:
        import lora_receive_file_nogui as app
    finally:
        sys.path.pop(0)
    cfg = synth.TxConfig(sf=7, cr=4)
    st = synth.build_stream(SMOKE_PAYLOADS, cfg, rng=np.random.default_rng(7))
    x = np.concatenate([st.iq, np.zeros(4096, dtype=np.complex64)])
    hi, _ = resampler.resample(x, 12, 5, resampler.design(12, 5))
    base = str(tmp_path / "smoke_2400k")
    sigmf.write_trace(base, hi, 2.4e6, 868.1e6, 868.1e6, 7, "4/8", 125000, 8, True, False, "", 3, datatype="ci16_le")
    srv = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    srv.bind(("127.0.0.1", 0))
    srv.settimeout(5.0)                               # (the datagrams are queued by the time main returns: only a failure waits)
    app.main([base, "--port", str(srv.getsockname()[1]), "--chunk", "50001", "--resample-to", "1000000"])
    got = [srv.recvfrom(4096)[0] for _ in SMOKE_PAYLOADS]
    srv.close()
    assert [g[15:] for g in got] == [synth.expected_frame_tail(p, cfg) for p in SMOKE_PAYLOADS]
