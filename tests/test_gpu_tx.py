"""GPU: the transmit side (include/lora_hip_tx.h, csrc/lora_tx.hip, lora.traffic_synthesizer / lora.modulator).  The capture
against its float64 definition (synth.build_wideband), bit-identical whatever the chunking, decoded again by the single decoder
and by the multi-SF gateway without leaving the device, integer output against iqformat.quantize, and the noise's statistics."""
import math
from collections import Counter

import numpy as np
import pytest

from gr_lora_amd import capi, iqformat, lora, synth

pytestmark = pytest.mark.gpu

FS = 375e3
N_ITEMS = 200000


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU: the HIP path has no CPU fallback")
    return torch


def _payload(n, seed):
    return bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


# (payload, sf, cr, bandwidth, start, freq_hz, amplitude, implicit, reduced_rate): decimation 3 (no power of two) and 4; starts that
# are no multiple of the kernel's tile or a wave; three and more overlapping from 7001 on; one at sample 0; silence between 75 k and
# 120 k; the last one runs past the end of what is generated
EMITTERS = [
    (_payload(17, 1), 7, 4, 125000, 0, 31000.0, 1.0, False, False),
    (_payload(17, 2), 6, 3, 93750, 4099, -100123.456789, 0.25, True, False),
    (_payload(8, 3), 9, 2, 125000, 7001, 50000.0, 0.5, False, True),
    (_payload(5, 4), 7, 1, 125000, 9003, -62500.0, 0.75, False, False),
    (_payload(9, 5), 7, 4, 125000, 120011, -125000.0 / 3.0, 0.5, False, False),
    (_payload(30, 6), 7, 2, 125000, 190003, 7.0, 1.0, False, False),
]


def _synth(emitters=EMITTERS, amplitude_scale=1.0, **kw):
    tx = lora.traffic_synthesizer(FS, **kw)
    for pl, sf, cr, bw, start, f, a, imp, rr in emitters:
        tx.add_frame(pl, sf, cr, bw, start, f, amplitude=a * amplitude_scale, implicit=imp, reduced_rate=rr)
    return tx


def _model_frames(emitters=EMITTERS):
    out = []
    for pl, sf, cr, bw, start, f, a, imp, rr in emitters:
        cfg = synth.TxConfig(sf=sf, cr=cr, bw=bw, implicit=imp, reduced_rate=rr, hdr_nibbles=synth.valid_hdr_nibbles(len(pl), cr, True))
        out.append(synth.WidebandFrame(pl, cfg, start, f, a, synth.valid_crc_bytes(pl)))
    return out


def _bits(t):
    """A complex64 / integer device tensor as the integers its bytes are (NaN-proof, sign-of-zero-proof equality)."""
    import torch
    return torch.view_as_real(t).contiguous().view(torch.int32) if t.dtype == torch.complex64 else t


@pytest.fixture(scope="module")
def capture(torch_cuda):
    """The capture in one call (device tensor), its model and the amplitude active at each sample: made once, never changed."""
    tx = _synth()
    y = tx.generate(N_ITEMS)
    pending = tx.pending
    tx.close()
    frames = _model_frames()
    model = synth.build_wideband(frames, FS, 0, N_ITEMS)
    amp = np.zeros(N_ITEMS)
    for f in frames:
        amp[f.start:f.start + synth.wideband_waveform(f, FS).size] += f.amplitude
    return y, model, amp, pending


def test_model_parity(torch_cuda, capture):
    """max |y - model| <= 16 * 2^-24 * (sum of the amplitudes active at that sample): two unit phasors good to an fp32 ulp per
    component, one product, one scale and one accumulation per emitter are 6 to 8 units of 2^-24; 16 leaves a factor of two.
    Where no emitter is active the items are +0.0, +0.0 bit for bit.  Measured on the MI355X: 1.92 units of 2^-24 x amplitude at
    the worst sample."""
    y, model, amp, pending = capture
    got = y.cpu().numpy()
    assert got.dtype == np.complex64 and got.size == N_ITEMS
    assert (amp > 2.0).any() and (amp == 0).sum() > 40000 and amp[0] == 1.0 and pending == 1
    err = np.abs(got.astype(np.complex128) - model)
    active = amp > 0
    worst = float((err[active] / amp[active]).max() / 2.0 ** -24)
    print("model parity: worst error %.3f units of 2^-24 x active amplitude, %.3e absolute" % (worst, float(err.max())))
    assert np.all(err <= 16 * 2.0 ** -24 * amp)
    assert not got[~active].view(np.uint32).any()
    assert np.abs(model[active]).max() > 2.0                 # the emitters do add up


def _pieces(tx, bounds, **kw):
    import torch
    out, pos = [], 0
    for b in bounds:
        out.append(tx.generate(b - pos, **kw))
        pos = b
    return torch.cat(out)


# ends: after 1 item, after 4097 more, inside emitter 0's quarter downchirp (symbols of 384 items: 12 * 384 .. + 96), on the last
# sample of its third header symbol, inside the overlap, on a tile's edge, the rest
BOUNDS = [1, 4098, 12 * 384 + 40, 12 * 384 + 96 + 3 * 384, 9004, 8 * 2048, 120011, 120012, N_ITEMS]


def test_chunking_is_bit_identical(torch_cuda, capture):
    torch = torch_cuda
    y = capture[0]
    for bounds in (BOUNDS, [1, 4098, N_ITEMS], list(range(65537, N_ITEMS, 65537)) + [N_ITEMS]):
        tx = _synth()
        z = _pieces(tx, bounds)
        assert tx.position == N_ITEMS and tx.pending == 1
        tx.close()
        assert torch.equal(_bits(z), _bits(y)), bounds


def test_chunking_is_bit_identical_with_noise(torch_cuda):
    torch = torch_cuda
    tx = _synth(noise_sigma=0.3, seed=77)
    whole = tx.generate(N_ITEMS)
    tx.close()
    tx = _synth(noise_sigma=0.3, seed=77)
    parts = _pieces(tx, BOUNDS)
    tx.close()
    assert torch.equal(_bits(parts), _bits(whole))
    tx = _synth(noise_sigma=0.3, seed=77)
    raw = _pieces(tx, BOUNDS, fmt="sc16", full_scale=8192.0)
    tx.close()
    assert np.array_equal(raw.cpu().numpy(), iqformat.quantize(whole.cpu().numpy(), "sc16", 8192.0))


# ---- round trips -----------------------------------------------------------------------------------------------------

def _decode(sf, cr, rr, iq):
    dec = lora.decoder(1e6, 125000, sf, False, cr, True, rr, verbose=False)
    frames = []
    dec.subscribe("frames", frames.append)
    dec.work(iq)
    dec.stop()
    dec.close()
    return [b[15:] for b in frames]


@pytest.mark.parametrize("sf,cr,lengths", [(7, 1, (11, 32)), (7, 4, (11, 32)), (9, 1, (9, 20)), (9, 4, (9, 20)), (10, 1, (7, 12)), (10, 4, (7, 12)),
                                           (12, 1, (4, 4)), (12, 4, (4, 4))])
def test_round_trip_one_channel(torch_cuda, sf, cr, lengths):
    """lora.modulator -> lora.decoder at 1 Msps: the published tails are the transmitted frames (header positions are not
    compared), and those the same decoder publishes from synth.build_stream's host-made stream of the same payloads."""
    rr = lora.lorawan_reduced_rate(sf, 125000)
    sps = 8 << sf
    payloads = [_payload(n, 100 * sf + cr + i) for i, n in enumerate(lengths)]
    mod = lora.modulator(1e6, 125000, sf, False, cr, True, reduced_rate=rr)
    parts, host, want = [], [], []
    for i, pl in enumerate(payloads):
        gap = (3 + i) * sps + 17 * i
        parts.append(mod.modulate(pl, gap_items=gap))
        cfg = synth.TxConfig(sf=sf, cr=cr, reduced_rate=rr, hdr_nibbles=synth.valid_hdr_nibbles(len(pl), cr, True))
        crc = synth.valid_crc_bytes(pl)
        host.append(synth.build_stream([pl], cfg, gaps=[gap], tail_symbols=0.0, crc_bytes=crc).iq)
        want.append(synth.expected_frame_tail(pl, cfg, crc))
    mod.close()
    tail = np.zeros(3 * sps, dtype=np.complex64)
    dev_iq, host_iq = np.concatenate(parts + [tail]), np.concatenate(host + [tail])
    assert dev_iq.dtype == np.complex64 and dev_iq.size == host_iq.size
    got = _decode(sf, cr, rr, dev_iq)
    assert got == want
    assert _decode(sf, cr, rr, host_iq) == got


GW = dict(fs=2e6, M=10, f0=100e3, D=2, ks=[-4, 0, 3])
# (grid index, sf, start in wide items): SF7, SF8 and SF9 overlap in time on three channels; channel 0 then carries an SF7 frame
# behind its SF8 frame (SF8: 4096 wide items per symbol, 44.25 symbols)
GW_PLAN = [(-4, 7, 30001), (0, 8, 20003), (3, 9, 10007), (0, 7, 20003 + 60 * 4096)]


@pytest.mark.parametrize("fmt", ["cf32", "sc16"])
def test_round_trip_gateway_on_the_device(torch_cuda, fmt):
    """traffic_synthesizer.generate -> multi_sf_gateway_receiver.work (a device tensor) -> stop: the multiset of (grid index, SF,
    tail) is what add_frame returned; the same through sc16 at full scale 2^14 and the gateway's integer ingress."""
    tx = lora.traffic_synthesizer(GW["fs"])
    want, end = [], 0
    for i, (k, sf, start) in enumerate(GW_PLAN):
        tail, items = tx.add_frame(_payload(6 + i, 40 + i), sf, 4, 125000, start, GW["f0"] + k * GW["fs"] / GW["M"], amplitude=0.5)
        want.append((k, sf, tail))
        end = max(end, start + items)
    n = end + 3 * (1 << 12) * 16
    rx = lora.multi_sf_gateway_receiver(GW["fs"], 0.0, GW["f0"], GW["M"], GW["ks"], 125000, sfs=(7, 8, 9), decimation=GW["D"])
    seen = []
    rx.subscribe("sf_frames", seen.append)
    for m in (300001, n - 300001):
        if fmt == "cf32":
            rx.work(tx.generate(m))
        else:
            rx.work(tx.generate(m, fmt="sc16", full_scale=2.0 ** 14), scale=2.0 ** -14)
    assert tx.pending == 0 and tx.position == n
    rx.stop()
    rx.close()
    tx.close()
    assert Counter((int(k), int(sf), blob[15:]) for k, sf, blob in seen) == Counter(want)


# ---- integer output --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,full_scale,scale_amp", [("sc16", 2.0 ** 14, 1.0), ("sc16", 32767.0, 1.5), ("sc8", 127.0, 1.5), ("cu8", 127.0, 1.5),
                                                      ("cu8", 100.3, 0.7), ("sc8", None, 0.2)])
def test_raw_output_is_quantize_of_the_cf32_output(torch_cuda, fmt, full_scale, scale_amp):
    """Bit for bit iqformat.quantize(generate(cf32), fmt, full_scale); amplitudes scaled by 1.5 at the type's largest scale clip
    at both ends; silence in cu8 is 128."""
    n = 90001
    tx = _synth(amplitude_scale=scale_amp)
    ref = tx.generate(n).cpu().numpy()
    tx.close()
    tx = _synth(amplitude_scale=scale_amp)
    raw = _pieces(tx, [4097, n], fmt=fmt, full_scale=full_scale).cpu().numpy()
    tx.close()
    fs = full_scale if full_scale is not None else 127.0
    want = iqformat.quantize(ref, fmt, fs)
    assert raw.dtype == want.dtype and raw.shape == want.shape == (2 * n,)
    assert np.array_equal(raw, want)
    info = np.iinfo(raw.dtype)
    if scale_amp > 1.0:
        assert raw.max() == info.max and raw.min() == info.min and np.abs(ref.view(np.float32)).max() * fs > info.max + 1
    silent = np.repeat(ref.view(np.uint64) == 0, 2)
    assert silent.sum() > 20000 and np.all(raw[silent] == (128 if fmt == "cu8" else 0))


# ---- noise -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def noise(torch_cuda):
    tx = lora.traffic_synthesizer(FS, noise_sigma=1.0, seed=12345)
    g = tx.generate(1 << 20).cpu().numpy()
    tx.close()
    return g


def test_noise_statistics(noise):
    """sigma = 1: each component is N(0, 1/2).  Every limit is five standard errors of its estimator at n = 2^20."""
    n = noise.size
    comp = noise.view(np.float32).reshape(-1, 2).astype(np.float64)
    sc = 1.0 / math.sqrt(2.0)
    for c in range(2):
        x = comp[:, c]
        assert abs(x.mean()) <= 5 * sc / math.sqrt(n), c
        assert abs(x.var() / sc ** 2 - 1.0) <= 5 * math.sqrt(2.0 / n), c
        lag1 = float(np.mean(x[:-1] * x[1:]) / x.var())
        assert abs(lag1) <= 5 / math.sqrt(n), c
    corr = float(np.mean(comp[:, 0] * comp[:, 1]) / (comp[:, 0].std() * comp[:, 1].std()))
    assert abs(corr) <= 5 / math.sqrt(n)
    p = math.erfc(3.0 / math.sqrt(2.0))                       # 0.0027: share of |g| > 3 sigma_c
    share = float(np.mean(np.abs(comp) > 3.0 * sc))
    assert abs(share - p) <= 5 * math.sqrt(p * (1 - p) / (2 * n))
    print("noise: mean %s var %s corr %.2e share %.6f" % (comp.mean(0), comp.var(0), corr, share))


def test_noise_is_a_function_of_seed_and_index(torch_cuda, noise):
    torch = torch_cuda
    tx = lora.traffic_synthesizer(FS, noise_sigma=1.0, seed=12345)
    again = _pieces(tx, [1, 4098, 100000, 1 << 18]).cpu().numpy()
    tx.close()
    assert np.array_equal(again.view(np.uint32), noise[: 1 << 18].view(np.uint32))
    tx = lora.traffic_synthesizer(FS, noise_sigma=1.0, seed=12346)
    other = tx.generate(1 << 18).cpu().numpy()
    tx.close()
    assert np.mean(other == noise[: 1 << 18]) < 1e-3
    corr = np.vdot(other, noise[: 1 << 18]) / (1 << 18)       # both of unit power: independent streams give about 1 / sqrt(n)
    assert abs(corr) <= 5 / math.sqrt(1 << 18)


def test_noise_adds_to_the_emitters(torch_cuda, capture, noise):
    """noisy - noiseless is the emitter-free noise to fp32 rounding.  The kernel rounds once: noisy = fl(clean + r) and
    noise = fl(r), each to 2^-24 relative, so per component |(noisy - clean) - noise| <= 2^-24 (|clean| + |r|) + 2^-24 |r|."""
    n = 150000
    tx = _synth(noise_sigma=1.0, seed=12345)
    noisy = tx.generate(n).cpu().numpy().view(np.float32).astype(np.float64)
    tx.close()
    clean = capture[0][:n].cpu().numpy().view(np.float32).astype(np.float64)
    g = noise[:n].view(np.float32).astype(np.float64)
    bound = 2.0 ** -23 * (np.abs(clean) + np.abs(g)) * (1 + 2.0 ** -20)
    assert np.all(np.abs((noisy - clean) - g) <= bound)
    assert np.abs(clean).max() > 1.0


# ---- the stream's bookkeeping ------------------------------------------------------------------------------------------

def test_refusals_and_retirement(torch_cuda):
    tx = lora.traffic_synthesizer(FS)
    _tail, items = tx.add_frame(b"first", 7, 4, 125000, 100, 0.0)
    assert tx.pending == 1 and tx.position == 0
    a = tx.generate(1000)
    assert tx.position == 1000 and tx.pending == 1
    with pytest.raises(capi.LoraHipError) as e:
        tx.add_frame(b"late", 7, 4, 125000, 999, 0.0)         # behind the position
    assert e.value.status == -6 and tx.pending == 1
    good = capi.tx_frame(b"good", 7, 4, 125000, start=2000)
    for bad in (capi.tx_frame(b"bad", 7, 4, 125000, start=500), capi.tx_frame(b"bad", 7, 4, 100000, start=5000),
                capi.tx_frame(b"bad", 7, 4, 125000, start=5000, amplitude=float("inf"))):
        with pytest.raises(capi.LoraHipError):
            tx._h.add_frames([good, bad])                     # one refused: none added
        assert tx.pending == 1
    tx.add_frame(b"on time", 7, 4, 125000, 1000, 0.0)          # exactly at the position: accepted
    assert tx.pending == 2
    b = tx.generate(100 + items - 1000 - 1)                    # one item short of the first frame's end
    assert tx.pending == 2
    c = tx.generate(1)
    assert tx.pending == 1
    rest = tx.generate(2 * items)
    assert tx.pending == 0 and tx.position == 100 + 3 * items
    assert not rest[-items // 2:].cpu().numpy().view(np.uint32).any()
    # the pieces are the model's capture of the two accepted frames
    import torch
    frames = [synth.WidebandFrame(p, synth.TxConfig(sf=7, cr=4, hdr_nibbles=synth.valid_hdr_nibbles(len(p), 4, True)), s, 0.0, 1.0, synth.valid_crc_bytes(p))
              for p, s in ((b"first", 100), (b"on time", 1000))]
    got = torch.cat([a, b, c, rest]).cpu().numpy()
    assert np.abs(got - synth.build_wideband(frames, FS, 0, got.size)).max() <= 16 * 2.0 ** -24 * 2
    tx.close()


def test_host_buffer_sibling_and_kernel_time(torch_cuda, capture):
    """lora_hip_tx_generate: the same items in host memory; the kernel's time is reported."""
    h = capi.Tx(FS)
    for pl, sf, cr, bw, start, f, a, imp, rr in EMITTERS:
        h.add_frames([capi.tx_frame(pl, sf, cr, bw, start=start, freq_hz=f, amplitude=a, implicit=imp, reduced_rate=rr)])
    out = np.concatenate([h.generate(70001), h.generate(N_ITEMS - 70001)])
    assert h.kernel_ms() > 0.0
    h.close()
    assert np.array_equal(out.view(np.uint32), capture[0].cpu().numpy().view(np.uint32))
