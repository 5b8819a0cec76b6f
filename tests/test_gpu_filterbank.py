"""GPU: the polyphase DFT filter bank (include/lora_hip_filterbank.h, csrc/lora_filterbank.hip) against the channeliser's float64
oracle (oracle/channelizer_oracle.Channelizer, one instance per grid channel at center_freq 0 and f = f0 + kappa fs / M in whole
Hz), and the gateway built on it (lora.gateway_receiver) end to end.  Tolerance: |y - y_oracle| <= 2e-5 max|y| up to 481 taps,
1e-4 max|y| at 3 855 taps (float32 sums of that many products).  The planner's design space (PLAN_CASES: tile shapes pfb_plan chooses
that the cases above never reach, each asserted through lora_hip_filterbank_get_plan) against tools/filterbank_model.direct, same tolerance (observed 1.6e-7 to
1.3e-6)."""
import os
import sys

import numpy as np
import pytest

from gr_lora_amd import lora, synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

CASES = [(2e6, 10, 2), (2e6, 10, 3), (2e6, 8, 8), (1.75e6, 7, 16), (16e6, 80, 16)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU: the HIP path has no CPU fallback")
    return torch


def _noise(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def _grid(M):
    return list(range(-(M // 2), (M + 1) // 2))


def _tol(ntaps):
    return 2e-5 if ntaps <= 481 else 1e-4


def _err(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got.astype(np.complex128) - want).max() / np.abs(want).max())


# every case with and without the grid offset; the 3 855-tap case once, with it
ONE_SHOT = [(fs, M, D, f0) for fs, M, D in CASES for f0 in (0.0, 100e3) if M <= 16 or f0 != 0.0]


@pytest.mark.parametrize("fs,M,D,f0", ONE_SHOT)
def test_one_shot_vs_oracle(torch_cuda, fs, M, D, f0):
    from gr_lora_amd import capi
    from oracle import channelizer_oracle as co
    rng = np.random.default_rng(M * 1000 + D)
    big = M > 16
    x = _noise(rng, 200_000 if big else 60_001)
    ks = _grid(M)
    fb = capi.FilterBank(fs, f0, M, ks, 125000, D)
    taps = fb.taps()
    y = fb.work(x)
    assert y.shape == (M, (x.size + D - 1) // D)
    check = [-32, -17, -1, 0, 9, 31] if big else ks
    worst = 0.0
    for k in check:
        o = co.Channelizer(fs, 0.0, f0 + k * fs / M, 125000, D)
        assert np.array_equal(taps, o.taps)
        e = _err(y[ks.index(k)], o.work(x))
        worst = max(worst, e)
        assert e <= _tol(taps.size), (k, e)
    print("filterbank one-shot fs=%g M=%d D=%d f0=%g taps=%d: max rel err %.2e" % (fs, M, D, f0, taps.size, worst))
    fb.close()


@pytest.mark.parametrize("fs,M,D,ks", [(2e6, 10, 3, [-5, -2, 0, 1, 4]), (1.75e6, 7, 16, [-3, 0, 3]), (16e6, 80, 16, [-40, 0, 39])])
def test_streaming_chunks_vs_oracle(torch_cuda, fs, M, D, ks):
    """Random chunk sizes, among them chunks shorter than D and shorter than the filter: the same stream as the oracle fed
    the same chunks."""
    from gr_lora_amd import capi
    from oracle import channelizer_oracle as co
    rng = np.random.default_rng(D)
    n = 120_000 if M > 16 else 90_000
    x = _noise(rng, n)
    f0 = 100e3 + 37.0
    fb = capi.FilterBank(fs, f0, M, ks, 125000, D)
    L = fb.taps().size
    os_ = [co.Channelizer(fs, 0.0, f0 + k * fs / M, 125000, D) for k in ks]
    got, want = [], [[] for _ in ks]
    pos, i = 0, 0
    fixed = [1, max(D - 1, 1), L - 1, L // 3, 2 * D + 1]
    while pos < n:
        c = fixed[i] if i < len(fixed) else int(rng.integers(1, 3 * L))
        c = min(c, n - pos)
        i += 1
        got.append(fb.work(x[pos:pos + c]))
        for j, o in enumerate(os_):
            want[j].append(o.work(x[pos:pos + c]))
        pos += c
    y = np.concatenate(got, axis=1)
    worst = 0.0
    for j, k in enumerate(ks):
        e = _err(y[j], np.concatenate(want[j]))
        worst = max(worst, e)
        assert e <= _tol(L), (k, e)
    print("filterbank streaming fs=%g M=%d D=%d taps=%d chunks=%d: max rel err %.2e" % (fs, M, D, L, i, worst))
    fb.close()


# ---- the planner's design space ------------------------------------------------------------------------------------------
# pfb_plan picks the tile shape (g, cw, nc) from (M, D, taps); each case states the plan it was chosen for (asserted through
# lora_hip_filterbank_get_plan: if the planner changes, these cases have to be chosen again) and what that plan reaches.
# Reference: tools/filterbank_model.direct, the one-shot float64 definition, at f = f0 + kappa fs / M.
#        fs    M    D    tw  taps Q  g  cw  nc  lds
PLAN_CASES = [
    (1e6,   1,    1, 1e5,  25, 25, 8, 64, 64, None),     # M = 1, g = 8
    (2e6,   5,    3, 1e5,  49, 10, 7, 64, 28, None),     # even Q, g = 7
    (2e6,  12,    7, 1e5,  49,  5, 2, 64, 10, None),     # g = 2, D coprime to M
    (2e6,  16,    5, 1e5,  49,  4, 1, 64, 13, None),     # even Q, n_sel = 16
    (2e6,  25,    1, 1e5,  49,  2, 2, 64, 64, None),     # Q = 2, odd M
    (2e6,  64,    1, 4e5,  13,  1, 1, 64, 64, None),     # Q = 1 with taps < M, nc stops at 64 g
    (2e6, 256,    1, 1e5,  49,  1, 1, 64, 56, 163696),   # M = 256, all 256 rows, 144 bytes below the LDS limit
    (2e6, 256,  256, 1e4, 481,  2, 1, 32,  1, None),     # cw = 32, D == M
    (2e6, 200, 1024, 1e4, 481,  3, 1, 16,  1, 161256),   # cw = 16, D > M with D mod M != 0
    (2e6, 256, 1024, 1e4, 481,  2, 1,  8,  1, None),     # cw = 8
]
PLAN_F0 = 100037.0
PLAN_IDS = ["M%d-D%d" % (c[1], c[2]) for c in PLAN_CASES]


def _plan_rows(M, D):
    """All rows up to M = 25 and in the M = 256, D = 1 case; otherwise both grid ends, 0 and two more."""
    if M <= 25 or (M == 256 and D == 1):
        return _grid(M)
    lo, hi = -(M // 2), (M + 1) // 2 - 1
    return [lo, -(M * 3 // 10), 0, M // 6 - 1, hi]


def _plan_fb(case):
    from gr_lora_amd import capi
    fs, M, D, tw, ntaps, Q, g, cw, nc, lds = case
    ks = _plan_rows(M, D)
    fb = capi.FilterBank(fs, PLAN_F0, M, ks, 125000, D, cutoff_hz=200e3, transition_hz=tw)
    p = fb.plan()
    assert fb.taps().size == ntaps
    assert (p["q"], p["g"], p["cw"], p["nc"]) == (Q, g, cw, nc), p
    assert p["lds_bytes"] <= 160 * 1024 and (lds is None or p["lds_bytes"] == lds), p
    return fb, ks, p


def _direct_rows(fs, M, D, ks, taps, x):
    from filterbank_model import direct
    return np.stack([direct(fs, PLAN_F0 + k * fs / M, taps, D, x) for k in ks])


def _stream_chunks(rng, n, D, L):
    """The chunk recipe of test_streaming_chunks_vs_oracle: [(pos, size)]."""
    fixed = [1, max(D - 1, 1), L - 1, L // 3, 2 * D + 1]
    out, pos, i = [], 0, 0
    while pos < n:
        c = fixed[i] if i < len(fixed) else int(rng.integers(1, 3 * L))
        c = min(c, n - pos)
        out.append((pos, c))
        pos += c
        i += 1
    return out


@pytest.mark.parametrize("case", PLAN_CASES, ids=PLAN_IDS)
def test_plan_space_one_shot_vs_model(torch_cuda, case):
    """Two full tiles, half a tile and one more output, in one call."""
    fs, M, D, tw, ntaps = case[:5]
    fb, ks, p = _plan_fb(case)
    T = p["cw"] * p["nc"]
    n_in = (2 * T + T // 2 + 1) * D + 1
    assert n_in <= 45_000
    x = _noise(np.random.default_rng(M * 1000 + D), n_in)
    y = fb.work(x)
    assert y.shape == (len(ks), (n_in + D - 1) // D) and np.isfinite(y.view(np.float32)).all()
    want = _direct_rows(fs, M, D, ks, fb.taps(), x)
    errs = [_err(y[i], want[i]) for i in range(len(ks))]
    print("filterbank plan one-shot fs=%g M=%d D=%d taps=%d plan=%s rows=%d n_in=%d: max rel err %.2e" % (fs, M, D, ntaps, p, len(ks), n_in, max(errs)))
    assert max(errs) <= _tol(ntaps), (ks[int(np.argmax(errs))], max(errs))
    fb.close()


STREAM_PLAN_CASES = [c for c in PLAN_CASES if (c[1], c[2]) in ((5, 3), (256, 256), (200, 1024))]
ROWS_PLAN_CASES = [c for c in PLAN_CASES if (c[1], c[2]) in ((256, 256), (200, 1024), (256, 1024))]


def _stream_len(p, D):
    """Two tiles and a half of input, 12 000 items at least, so that the random chunks follow the fixed ones for a while."""
    return max(5 * p["cw"] * p["nc"] * D // 2 + 1, 12_000)


@pytest.mark.parametrize("case", STREAM_PLAN_CASES, ids=["M%d-D%d" % (c[1], c[2]) for c in STREAM_PLAN_CASES])
def test_plan_space_streaming_vs_model(torch_cuda, case):
    """The same plans fed in chunks (shorter than D, shorter than the filter, random): the concatenated stream is the one-shot
    definition's."""
    fs, M, D, tw, ntaps = case[:5]
    fb, ks, p = _plan_fb(case)
    rng = np.random.default_rng(7 * M + D)
    n = _stream_len(p, D)
    assert n <= 45_000
    x = _noise(rng, n)
    chunks = _stream_chunks(rng, n, D, ntaps)
    y = np.concatenate([fb.work(x[pos:pos + c]) for pos, c in chunks], axis=1)
    want = _direct_rows(fs, M, D, ks, fb.taps(), x)
    errs = [_err(y[i], want[i]) for i in range(len(ks))]
    print("filterbank plan streaming fs=%g M=%d D=%d taps=%d chunks=%d n_in=%d: max rel err %.2e" % (fs, M, D, ntaps, len(chunks), n, max(errs)))
    assert max(errs) <= _tol(ntaps), (ks[int(np.argmax(errs))], max(errs))
    fb.close()


@pytest.mark.parametrize("case", ROWS_PLAN_CASES, ids=["M%d-D%d" % (c[1], c[2]) for c in ROWS_PLAN_CASES])
def test_plan_space_rows_mode_equals_run_device(torch_cuda, case):
    """run_device_rows at cw < 64 (the kernel reads the row pointers from lanes that hold no output; at cw = 8 the second
    destination's lie outside the active lanes), 2 destinations, fed the same chunks as run_device: the same bits in both, and
    nothing written around them."""
    torch = torch_cuda
    fs, M, D, tw, ntaps = case[:5]
    fb, ks, p = _plan_fb(case)
    ref, _, _ = _plan_fb(case)
    rng = np.random.default_rng(11 * M + D)
    n = _stream_len(p, D)
    x = _noise(rng, n)
    chunks = _stream_chunks(rng, n, D, ntaps)
    nch, total, pad = len(ks), (n + D - 1) // D, 5
    d_x = torch.from_numpy(x.view(np.float32)).to("cuda")
    out_ref = torch.full((nch, 2 * total), float("nan"), dtype=torch.float32, device="cuda")
    stride = total + 2 * pad
    bufs = [torch.full((nch * 2 * stride,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
    stream = torch.cuda.current_stream().cuda_stream
    got = 0
    for pos, c in chunks:
        no = fb.output_items(c)
        ptrs = [bufs[d].data_ptr() + 8 * (r * stride + pad + got) for d in range(2) for r in range(nch)]
        assert fb.run_device_rows(d_x.data_ptr() + 8 * pos, c, ptrs, 2, no, stream) == no
        assert ref.run_device(d_x.data_ptr() + 8 * pos, c, out_ref.data_ptr() + 8 * got, total, stream) == no
        got += no
    assert got == total and not torch.isnan(out_ref).any()
    want = out_ref.view(torch.int32).cpu()
    for d in range(2):
        b = bufs[d].view(nch, 2 * stride).cpu()
        assert torch.equal(b[:, 2 * pad:2 * (pad + total)].contiguous().view(torch.int32), want), d
        assert torch.isnan(b[:, :2 * pad]).all() and torch.isnan(b[:, 2 * (pad + total):]).all(), d
    e = _err(out_ref.cpu().numpy().view(np.complex64), _direct_rows(fs, M, D, ks, fb.taps(), x))
    print("filterbank plan rows fs=%g M=%d D=%d taps=%d chunks=%d: max rel err %.2e" % (fs, M, D, ntaps, len(chunks), e))
    assert e <= _tol(ntaps)
    ref.close()
    fb.close()


def test_long_stream_phase_does_not_drift(torch_cuda):
    """More than 2^32 zero items through run_device (one row, D = 1024), then noise: the premix phase is evaluated in double
    per tile and the grid shift in int64, so the output still matches the oracle placed at the same absolute index."""
    from gr_lora_amd import capi
    from oracle import channelizer_oracle as co
    torch = torch_cuda
    fs, M, D, k, f0 = 2e6, 10, 1024, 3, 100037.0
    fb = capi.FilterBank(fs, f0, M, [k], 125000, D)
    o = co.Channelizer(fs, 0.0, f0 + k * fs / M, 125000, D)
    chunk = 1 << 27
    calls = 33                                   # 33 * 2^27 = 4.43e9 > 2^32
    zeros = torch.zeros(2 * chunk, dtype=torch.float32, device="cuda")
    out = torch.empty(2 * (chunk // D + 1), dtype=torch.float32, device="cuda")
    for _ in range(calls):
        assert fb.run_device(zeros.data_ptr(), chunk, out.data_ptr(), chunk // D + 1) == chunk // D
    skip = calls * chunk
    assert skip > 1 << 32
    o._n = skip
    p = o.freq / o.fs * skip
    o._phase = p - np.floor(p)
    x = _noise(np.random.default_rng(4), 300_000)
    e = _err(fb.work(x)[0], o.work(x))
    print("filterbank after %d items: rel err %.2e" % (skip, e))
    assert e <= 2e-5
    fb.close()


def _wideband(fs, f0, M, ks, payloads_per_channel, seed):
    """One transmitter per grid channel (SF7, CR 4/8, 125 kHz, synthesised at fs), each moved to f0 + kappa fs / M, summed."""
    cfg = synth.TxConfig(sf=7, cr=4, samp_rate=fs)
    rng = np.random.default_rng(seed)
    streams = []
    for k in ks:
        pl = [bytes(rng.integers(0, 256, int(rng.integers(4, 40)), dtype=np.uint8)) for _ in range(payloads_per_channel)]
        streams.append(synth.build_stream(pl, cfg, rng=rng, lead=int(rng.integers(cfg.sps, 6 * cfg.sps))))
    n = max(st.iq.size for st in streams)
    t = np.arange(n, dtype=np.float64)
    wide = np.zeros(n, dtype=np.complex128)
    for k, st in zip(ks, streams):
        f = f0 + k * fs / M
        ph = f / fs * t[: st.iq.size]
        wide[: st.iq.size] += st.iq * np.exp(2j * np.pi * (ph - np.floor(ph)))
        st.iq = None                             # (64 channels at 16 Msps: keep only the sum)
    return wide.astype(np.complex64), streams, synth.TxConfig(sf=7, cr=4)


def test_eu868_gateway_end_to_end(torch_cuda, oracle_mod):
    """Workload (a): 8 transmitters on the EU868-like grid -> gateway_receiver in chunks of 65 536.  Per channel: the
    transmitted payloads; the blobs of channeliser-oracle -> decoder-oracle; the device chain run_device -> decode_device."""
    from gr_lora_amd import capi
    from oracle import channelizer_oracle as co
    torch = torch_cuda
    fs, M, f0, D = 2e6, 10, 100e3, 2
    ks = list(range(-4, 4))
    wide, streams, cfg1 = _wideband(fs, f0, M, ks, 4, seed=868)
    gw = lora.gateway_receiver(fs, 868.0e6, f0, M, ks, 125000, 7, False, 4, True, decimation=D)
    frames, chan_frames = [], []
    gw.subscribe("frames", frames.append)
    gw.subscribe("channel_frames", chan_frames.append)
    for i in range(0, wide.size, 65536):
        gw.work(wide[i:i + 65536])
    gw.stop()
    assert [b for _, b in chan_frames] == frames
    got = {k: [b for kk, b in chan_frames if kk == k] for k in ks}
    # the device chain over the same capture, all rows decoded as independent streams in one pass
    fb = capi.FilterBank(fs, f0, M, ks, 125000, D)
    no = fb.output_items(wide.size)
    d_in = torch.from_numpy(wide.view(np.float32)).to("cuda:0")
    d_out = torch.empty((len(ks), 2 * no), dtype=torch.float32, device="cuda:0")
    assert fb.run_device(d_in.data_ptr(), wide.size, d_out.data_ptr(), no) == no
    h = capi.Handle(sf=7, cr=4, demod=capi.DEMOD_FFT_COMPAT)
    h.decode_device(d_out.data_ptr(), len(ks) * no, [c * no for c in range(len(ks))], [no] * len(ks), 0)
    dev = {}
    for blob, info in h.drain():
        dev.setdefault(ks[info.stream], []).append(blob)
    for k, st in zip(ks, streams):
        assert [b[15:] for b in got[k]] == [synth.expected_frame_tail(p, cfg1) for p in st.payloads], k
        bb = co.Channelizer(fs, 0.0, f0 + k * fs / M, 125000, D).work(wide).astype(np.complex64)
        assert got[k] == oracle_mod.decode_stream(bb, demod=2, sf=7, cr=4), k
        assert dev.get(k, []) == got[k], k
    h.close()
    fb.close()
    gw.close()


def test_us915_gateway_end_to_end(torch_cuda):
    """Workload (b): 64 transmitters on the US915-like uplink grid synthesised at 16 Msps -> gateway_receiver: every payload on
    every channel decoded, on its own channel, and nothing else."""
    fs, M, f0, D = 16e6, 80, 100e3, 16
    ks = list(range(-32, 32))
    wide, streams, cfg1 = _wideband(fs, f0, M, ks, 3, seed=915)
    gw = lora.gateway_receiver(fs, 902.2e6, f0, M, ks, 125000, 7, False, 4, True, decimation=D)
    chan_frames = []
    gw.subscribe("channel_frames", chan_frames.append)
    for i in range(0, wide.size, 1 << 20):
        gw.work(wide[i:i + (1 << 20)])
    gw.stop()
    got = {k: [b[15:] for kk, b in chan_frames if kk == k] for k in ks}
    assert len(chan_frames) == sum(len(st.payloads) for st in streams)
    for k, st in zip(ks, streams):
        assert got[k] == [synth.expected_frame_tail(p, cfg1) for p in st.payloads], k
    gw.close()
