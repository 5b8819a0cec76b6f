"""GPU: the IQ conditioner (include/lora_hip_conditioner.h, csrc/lora_conditioner.hip, capi.Conditioner, lora.iq_conditioner) against
its float64 definition (gr_lora_amd.conditioner.condition): block moments bit for bit, parameters within the rounding bound, the
output bit for bit from the device's own parameters, identical whatever the chunking and the input format, and in front of the
decoder and the resampler on impaired captures.

The parameter tolerance is gr_lora_amd.conditioner.parameter_bound: every one of the ten fp64 operations good to one unit in the
last place (u = 2^-52) on either side, propagated to first order along the definition, plus the two roundings to fp32,
2^-23 (|p| + d).  With IEEE division and square root on the device the two sides agree exactly; observed maxima of
error / bound on an MI355X are printed by test_against_the_float64_model and recorded in DESIGN.md 4.18.
"""
import functools

import numpy as np
import pytest

import conditioner_cases as cc
from gr_lora_amd import capi, conditioner as cd, iqformat, lora

pytestmark = pytest.mark.gpu

N_SMALL = 256 * 37 + 101
SHAPES = [(256, 1, N_SMALL), (256, 3, N_SMALL), (256, 16, N_SMALL), (4096, 16, 100003)]      # (B, W, items)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test needs a GPU: the HIP path has no CPU fallback")
    return torch


def _bits(y):
    return np.ascontiguousarray(y).view(np.uint32)


def _bits64(m):
    return np.ascontiguousarray(m).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _model(kind, B, W, n):
    y, mom, par = cd.condition(cc.synthetic(kind, n), B, W)
    for a in (y, mom, par):
        a.setflags(write=False)
    return y, mom, par


@functools.lru_cache(maxsize=None)
def _one_shot(kind, B, W, n):
    """(outputs with the flushed tail, moments, params) of one work() call and one flush()."""
    h = capi.Conditioner(B, W)
    x = cc.synthetic(kind, n)
    y, first = h.work(x)
    mom, par = h.block_records()
    assert first == 0 and y.size == n // B * B and h.held_items() == n % B
    tail, first_tail = h.flush()
    assert first_tail == y.size and tail.size == n % B and h.held_items() == 0
    h.close()
    out = np.concatenate([y, tail])
    for a in (out, mom, par):
        a.setflags(write=False)
    return out, mom, par


@pytest.mark.parametrize("kind", cc.INPUTS)
@pytest.mark.parametrize("B,W,n", SHAPES)
def test_against_the_float64_model(torch_cuda, B, W, n, kind):
    """Moments: equal to the model's as uint64.  Parameters: within parameter_bound of the model's (module docstring); for the
    zeros and the constant the guard holds on both sides, so a = 0 and b = 1 exactly.  Output: the three fp32 operations of the
    definition in numpy on the device's own fp32 parameters, bit for bit, the flushed tail with the last block's."""
    x = cc.synthetic(kind, n)
    y, mom, par = _one_shot(kind, B, W, n)
    _, mmom, mpar = _model(kind, B, W, n)
    nb = n // B
    assert mom.shape == mmom.shape == (nb, 5) and par.shape == mpar.shape == (nb, 4) and y.size == n
    assert np.array_equal(_bits64(mom), _bits64(mmom))
    S, nw = cd.window_sums(mmom, W)
    bound = cd.parameter_bound(S, nw * float(B))
    err = np.abs(par.astype(np.float64) - mpar.astype(np.float64))
    assert np.isfinite(par).all() and np.isfinite(bound).all()
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("conditioner B %d W %d %s: max parameter error / bound %.3g (max error %.3g)" % (B, W, kind, worst, float(err.max())))
    assert np.all(err <= bound)
    if kind in ("zeros", "constant"):
        assert np.array_equal(par[:, 2:], np.tile(np.float32([0.0, 1.0]), (nb, 1)))
        assert np.isfinite(y.view(np.float32)).all() and not _bits(y).any()
    want = np.concatenate([cd.apply(x[:nb * B].reshape(nb, B), par[:, None, :]).reshape(-1), cd.apply(x[nb * B:], par[-1])])
    assert np.array_equal(_bits(y), _bits(want))


def _feed(torch, h, x, sizes, device):
    """x in chunks of the given sizes (the last size repeats), then flush: (outputs, moments, params), with first_out and
    output_items of every call checked.  device: torch tensors through run_device / flush_device, else host arrays."""
    B = h.plan()[0]
    outs, moms, pars, pos, i = [], [], [], 0, 0
    xd = torch.from_numpy(np.array(x)).cuda() if device else None
    buf = torch.zeros(x.size + 2, dtype=torch.complex64, device="cuda") if device else None
    emitted = 0
    while pos < x.size:
        c = min(sizes[min(i, len(sizes) - 1)], x.size - pos)
        want = (pos + c) // B * B - emitted
        assert h.output_items(c) == want
        if device:
            got, first = h.run_device(xd.data_ptr() + 8 * pos, c, buf.data_ptr() + 8 * emitted, want)
            assert got == want
        else:
            y, first = h.work(x[pos:pos + c])
            assert y.size == want
            outs.append(y)
        assert first == emitted
        if want:
            m, p = h.block_records()
            assert m.shape[0] == want // B
            moms.append(m)
            pars.append(p)
        else:
            assert h.block_records()[0].shape[0] == 0
        emitted += want
        pos += c
        i += 1
    held = x.size - emitted
    assert h.held_items() == held
    if device:
        got, first = h.flush_device(buf.data_ptr() + 8 * emitted, held)
        assert (got, first) == (held, emitted)
        out = buf[:x.size].cpu().numpy()
    else:
        tail, first = h.flush()
        assert (tail.size, first) == (held, emitted)
        out = np.concatenate(outs + [tail])
    return out, np.concatenate(moms), np.concatenate(pars)


@pytest.mark.parametrize("B,W,n", SHAPES)
def test_chunking_is_bit_identical(torch_cuda, B, W, n):
    """One shot, chunks of B - 1, B, B + 1, a seeded random split with empty calls in it, and chunks of 1 (over the first
    3 B + 5 items): outputs, flushed tail and records are those of the one-shot call, bit for bit; host and device entry points."""
    torch = torch_cuda
    x = cc.synthetic("impaired", n)
    want = _one_shot("impaired", B, W, n)
    rng = np.random.default_rng(B + W)
    random_sizes = [int(v) for v in rng.integers(0, 3 * B, 200)]
    random_sizes[3] = random_sizes[10] = random_sizes[11] = 0
    h = capi.Conditioner(B, W)
    for k, sizes in enumerate(([n], [B - 1], [B], [B + 1], random_sizes, [1, B, 0, 2 * B + 1, 3, 50000])):
        got = _feed(torch, h, x, sizes, device=k % 2 == 0)
        for g, w in zip(got, want):
            assert g.shape == w.shape, "chunks of %s" % (sizes[:6],)
        assert np.array_equal(_bits(got[0]), _bits(want[0])), "chunks of %s" % (sizes[:6],)
        assert np.array_equal(_bits64(got[1]), _bits64(want[1])) and np.array_equal(_bits(got[2]), _bits(want[2])), "chunks of %s" % (sizes[:6],)
        h.reset()
    m = 3 * B + 5
    got = _feed(torch, h, x[:m], [1], device=True)
    assert np.array_equal(_bits(got[0][:3 * B]), _bits(want[0][:3 * B])) and np.array_equal(_bits64(got[1]), _bits64(want[1][:3]))
    assert np.array_equal(_bits(got[2]), _bits(want[2][:3]))
    assert np.array_equal(_bits(got[0][3 * B:]), _bits(cd.apply(x[3 * B:m], want[2][2])))          # the tail: block 2's parameters
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
    """Random full-range integers, default and explicit scale, the format changing between the calls of one stream (the second
    call starts inside a block, the third is shorter than a block): outputs, flushed tail and records equal those of the cf32
    entry points fed iqformat.to_cf32's items.  Host arrays through capi.Conditioner, torch tensors through lora.iq_conditioner."""
    n1, n2, n3 = 5003, 6002, 17
    qa, qb, qc = _raw(fmt_a, n1, 1), _raw(fmt_b, n2, 2), _raw(fmt_a, n3, 3)
    xa, xb, xc = iqformat.to_cf32(qa, fmt_a, scale_a), iqformat.to_cf32(qb, fmt_b, scale_b), iqformat.to_cf32(qc, fmt_a, scale_a)
    if not device_input:
        ref, dut = capi.Conditioner(256, 3), capi.Conditioner(256, 3)
        for x, q, fmt, scale in ((xa, qa, fmt_a, scale_a), (xb, qb, fmt_b, scale_b), (xc, qc, fmt_a, scale_a), (xb, qb.reshape(-1, 2), fmt_b, scale_b)):
            w, g = ref.work(x), dut.work_raw(q, fmt, scale)
            assert g[1] == w[1] and g[0].size == w[0].size and np.array_equal(_bits(g[0]), _bits(w[0]))
            (wm, wp), (gm, gp) = ref.block_records(), dut.block_records()
            assert np.array_equal(_bits64(gm), _bits64(wm)) and np.array_equal(_bits(gp), _bits(wp))
        w, g = ref.flush(), dut.flush()
        assert g[1] == w[1] and g[0].size == w[0].size == (n1 + 2 * n2 + n3) % 256 and np.array_equal(_bits(g[0]), _bits(w[0]))
        ref.close()
        dut.close()
        return
    torch = torch_cuda
    ref, dut, host = lora.iq_conditioner(256, 3), lora.iq_conditioner(256, 3), capi.Conditioner(256, 3)
    want = [ref.work(torch.from_numpy(xa).cuda()), ref.work(torch.from_numpy(xb.view(np.float32).copy()).cuda()),     # complex64, then float32 interleaved
            ref.work(torch.from_numpy(xc).cuda()), ref.work(xb), ref.flush()]                                          # ... and a host array
    got = [dut.work(torch.from_numpy(qa).cuda(), scale=scale_a), dut.work(torch.from_numpy(qb.reshape(-1, 2)).cuda(), scale=scale_b),
           dut.work(torch.from_numpy(qc).cuda(), scale=scale_a), dut.work(qb, scale=scale_b), dut.flush()]
    href = [host.work(xa)[0], host.work(xb)[0], host.work(xc)[0], host.work(xb)[0], host.flush()[0]]
    for i, (g, w, hr) in enumerate(zip(got, want, href)):
        assert (i >= 3) == isinstance(g, np.ndarray) == isinstance(w, np.ndarray)
        if i < 3:
            assert g.is_cuda and g.dtype == torch.complex64 and w.is_cuda
            g, w = g.cpu().numpy(), w.cpu().numpy()
        assert g.size == hr.size and np.array_equal(_bits(g), _bits(w)) and np.array_equal(_bits(g), _bits(hr))
    assert sum(h.size for h in href) == n1 + 2 * n2 + n3
    with pytest.raises(TypeError):
        ref.work(torch.from_numpy(xa).cuda(), scale=0.5)
    for s in (ref, dut, host):
        s.close()


@pytest.mark.parametrize("fmt", [iqformat.SC16, iqformat.SC8, iqformat.CU8])
def test_integer_input_at_any_item_offset(torch_cuda, fmt):
    """Device input starting 0, 1, 2 and 3 items into a tensor (aligned to its component only), in two calls (the second starts inside
    a block at an odd held count, so the item-by-item path runs too), gives the bits of the cf32 path."""
    torch = torch_cuda
    n = 256 * 9 + 77
    q = _raw(fmt, n + 3, 5 + fmt)
    qd = torch.from_numpy(q).cuda()
    ib = iqformat.ITEM_BYTES[fmt]
    out = torch.zeros(n, dtype=torch.complex64, device="cuda")
    for off in range(4):
        x = iqformat.to_cf32(q[2 * off:2 * (off + n)], fmt)
        ref, dut = capi.Conditioner(256, 3), capi.Conditioner(256, 3)
        want = np.concatenate([ref.work(x[:1001])[0], ref.work(x[1001:])[0], ref.flush()[0]])
        wrec = ref.block_records()
        g1, _ = dut.run_device_raw(qd.data_ptr() + ib * off, 1001, fmt, out.data_ptr(), n)
        g2, first = dut.run_device_raw(qd.data_ptr() + ib * (off + 1001), n - 1001, fmt, out.data_ptr() + 8 * g1, n - g1)
        grec = dut.block_records()
        g3, _ = dut.flush_device(out.data_ptr() + 8 * (g1 + g2), n - g1 - g2)
        assert (g1, g2, g3, first) == (768, 1536, 77, 768)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)), off
        assert np.array_equal(_bits64(grec[0]), _bits64(wrec[0])) and np.array_equal(_bits(grec[1]), _bits(wrec[1])), off
        ref.close()
        dut.close()


def test_argument_checks_consume_nothing(torch_cuda):
    """An unknown format, an unusable scale, a misaligned pointer, an output that overlaps the input and an output too small are
    refused (the last with *n_out set), and the stream is where it was."""
    torch = torch_cuda
    C = capi.C
    h = capi.Conditioner(256, 3)
    q = _raw(iqformat.SC16, 1025, 3)
    out = np.zeros(2048, dtype=np.complex64)
    n, first = C.c_size_t(0), C.c_uint64(0)
    for ptr, fmt, scale in ((q.ctypes.data, 7, 0.0), (q.ctypes.data, iqformat.SC16, float("inf")), (q.ctypes.data, iqformat.SC16, -1.0),
                            (q.ctypes.data + 1, iqformat.SC16, 0.0)):
        assert h.L.lora_hip_conditioner_work_raw(h.h, ptr, 1024, fmt, scale, out.ctypes.data, out.size, C.byref(n), C.byref(first)) == -6
    x = cc.synthetic("impaired", N_SMALL)
    buf = torch.zeros(4096, dtype=torch.complex64, device="cuda")
    buf[:1000] = torch.from_numpy(np.array(x[:1000])).cuda()
    for off in (0, 8 * 999, -8 * 767):                                     # the same range, its last item, the output's last item
        with pytest.raises(capi.LoraHipError) as e:
            h.run_device(buf.data_ptr(), 1000, buf.data_ptr() + off, 768)
        assert e.value.status == -6
    got, _ = h.run_device(buf.data_ptr(), 1000, buf.data_ptr() + 8 * 1000, 768)      # adjacent is fine
    assert got == 768 and h.held_items() == 232
    for max_out in (0, 511):
        st = h.L.lora_hip_conditioner_work(h.h, np.ascontiguousarray(x[1000:1600]).ctypes.data, 600, out.ctypes.data, max_out, C.byref(n), C.byref(first))
        assert st == -7 and n.value == 768 and first.value == 768 and h.held_items() == 232
    st = h.L.lora_hip_conditioner_flush(h.h, out.ctypes.data, 231, C.byref(n), C.byref(first))
    assert st == -7 and n.value == 232 and h.held_items() == 232
    y2, first2 = h.work(x[1000:1600])
    tail, first3 = h.flush()
    assert (first2, first3, tail.size) == (768, 1536, 64)
    want = _one_shot("impaired", 256, 3, N_SMALL)
    got_all = np.concatenate([buf[1000:1768].cpu().numpy(), y2])
    assert np.array_equal(_bits(got_all), _bits(want[0][:1536]))
    assert np.array_equal(_bits(tail), _bits(cd.apply(x[1536:1600], want[2][5])))
    h.close()


def test_set_fixed_applies_exactly_the_constants_given(torch_cuda):
    """Fixed mode: every item, the flushed tail included, is the three fp32 operations on the four constants; the records carry
    them; set_adaptive starts the window again at the next block, so what follows is the model of the remaining stream alone."""
    x = cc.synthetic("impaired", N_SMALL)
    k = np.float32([0.0123, -0.0456, -0.17632698, 0.80654])
    h = capi.Conditioner(256, 3)
    h.set_fixed(*k)
    y, first = h.work(x[:2000])
    mom, par = h.block_records()
    assert first == 0 and y.size == 1792 and np.array_equal(_bits(par), _bits(np.tile(k, (7, 1)))) and not _bits64(mom).any()
    assert np.array_equal(_bits(h.newest()[0]), _bits(k))
    tail, _ = h.flush()
    assert np.array_equal(_bits(np.concatenate([y, tail])), _bits(cd.apply(x[:2000], k)))
    h.set_adaptive()
    rest, first = h.work(x[2000:])
    want, wmom, wpar = cd.condition(x[2000:], 256, 3)
    gmom, gpar = h.block_records()
    assert first == 2000 and np.array_equal(_bits64(gmom), _bits64(wmom))
    assert np.array_equal(_bits(rest), _bits(cd.apply(x[2000:2000 + rest.size].reshape(-1, 256), gpar[:, None, :]).reshape(-1)))
    S, nw = cd.window_sums(wmom, 3)
    assert np.all(np.abs(gpar.astype(np.float64) - wpar) <= cd.parameter_bound(S, nw * 256.0))
    C = capi.C
    assert h.L.lora_hip_conditioner_set_fixed(h.h, C.c_float(float("nan")), 0.0, 0.0, 1.0) == -6
    h.close()


def test_reset_restarts_at_block_zero_and_flags_switch_the_halves_off(torch_cuda):
    x = cc.synthetic("dc40", N_SMALL)
    want = _one_shot("dc40", 256, 16, N_SMALL)
    h = capi.Conditioner(256, 16)
    h.work(x[:3000])
    h.reset()
    assert h.held_items() == 0 and np.array_equal(h.newest()[0], np.float32(cd.IDENTITY))
    y, first = h.work(x)
    mom, par = h.block_records()
    tail, _ = h.flush()
    assert first == 0 and np.array_equal(_bits(np.concatenate([y, tail])), _bits(want[0])) and np.array_equal(_bits(par), _bits(want[2]))
    h.close()
    for dc, iq in ((True, False), (False, True), (False, False)):
        h = capi.Conditioner(256, 16, dc=dc, iq=iq)
        y, _ = h.work(x)
        mom, par = h.block_records()
        h.close()
        assert np.array_equal(_bits64(mom), _bits64(want[1]))
        expect = np.array(want[2])
        if not dc:
            expect[:, :2] = 0.0
        if not iq:
            expect[:, 2:] = np.float32([0.0, 1.0])
        assert np.array_equal(_bits(par), _bits(expect))
        assert np.array_equal(_bits(y), _bits(cd.apply(x[:y.size].reshape(-1, 256), par[:, None, :]).reshape(-1)))
        if not dc and not iq:
            assert np.array_equal(_bits(y), _bits(x[:y.size]))


def test_estimate_reports_the_front_end(torch_cuda):
    """lora.iq_conditioner.estimate() is the model's estimate of the newest block's window (formed on the host from the device's
    fp64 estimates), and sits within the CPU test's five deviations of the impairment put in: 2 dB, 10 degrees, DC at -6 dBc."""
    n = 100003
    x = cc.synthetic("impaired", n)
    st = lora.iq_conditioner()
    assert st.estimate()["dc_dbfs"] == float("-inf") and st.estimate()["gain_db"] == 0.0
    y = st.work(x)
    est = st.estimate()
    st.close()
    _, mmom, _ = _model("impaired", 4096, 16, n)
    S, nw = cd.window_sums(mmom, 16)
    want = cd.estimate(S[-1], nw[-1] * 4096.0)
    assert y.size == n // 4096 * 4096
    assert abs(est["dc"] - want["dc"]) <= 1e-12 and abs(est["gain_db"] - want["gain_db"]) <= 1e-9 and abs(est["phase_deg"] - want["phase_deg"]) <= 1e-9
    k = 5.0 / np.sqrt(65536.0) + 4.0 / 65536.0
    assert abs(est["gain_db"] - 2.0) <= 20.0 / np.log(10.0) * k and abs(est["phase_deg"] - 10.0) <= np.degrees(k)
    d, s, g = abs(cc.dc_offset(-6.0, 0.1)), 0.1 / np.sqrt(2.0), 10.0 ** 0.1
    assert abs(est["dc_dbfs"] - 20.0 * np.log10(d)) <= 20.0 / np.log(10.0) * 5.0 * s * np.sqrt((1.0 + g * g) / 65536.0) / d * 1.1


@pytest.mark.parametrize("gain_db,phase_deg,dbc", cc.IMPAIRMENTS)
@pytest.mark.parametrize("sf", [7, 10])
def test_end_to_end_into_the_decoder_as_sc8(torch_cuda, sf, gain_db, phase_deg, dbc):
    """The CPU test's impaired capture as sc8 (0.9 mapped to full scale), in 65 536-item chunks through lora.iq_conditioner into
    lora.decoder (the reference's own estimator): all 8 payloads come out."""
    y = cc.impaired_capture(sf, gain_db, phase_deg, dbc)
    q = iqformat.quantize(y, "sc8", 127.0 / 0.9)
    st = lora.iq_conditioner()
    dec = lora.decoder(1e6, 125000, sf, False, 4, True, demod=capi.DEMOD_GRAD, verbose=False)
    seen = []
    dec.subscribe("frames", seen.append)
    n_out = 0
    for lo in range(0, y.size, 65536):
        z = st.work(q[2 * lo:2 * (lo + 65536)], scale=0.9 / 127.0)
        assert isinstance(z, np.ndarray) and z.dtype == np.complex64 and z.size % 4096 == 0
        n_out += z.size
        dec.work(z)
    tail = st.flush()
    dec.work(tail)
    dec.stop()
    dec.close()
    st.close()
    assert n_out + tail.size == y.size
    assert [bytes(b)[15:] for b in seen] == cc.tails(sf)


def test_in_front_of_the_resampler_and_the_receiver(torch_cuda):
    """The SF7 capture at 2.4 Msps, impaired there (2 dB, 10 degrees, DC at -6 dBc), as device tensors through lora.iq_conditioner and
    lora.rational_resampler(2.4e6, 1e6) into lora_receiver: all 8 payloads come out."""
    torch = torch_cuda
    hi = cc.capture_at_2400k()
    st = lora.iq_conditioner()
    rr = lora.rational_resampler(2.4e6, 1e6)
    rx = lora.lora_receiver(1e6, 868.1e6, [868.1e6], 125000, 7, False, 4, True, demod=capi.DEMOD_GRAD, verbose=False)
    seen = []
    rx.subscribe("frames", seen.append)

    def feed(z):
        assert z.is_cuda and z.dtype == torch.complex64
        if z.numel():
            rx.work(rr.work(z).cpu().numpy())

    for lo in range(0, hi.size, 100000):
        feed(st.work(torch.from_numpy(np.array(hi[lo:lo + 100000])).cuda()))
    feed(st.flush())
    rx.stop()
    rx.decoder.close()
    rx.channelizer._h.close()
    rr.close()
    st.close()
    assert [bytes(b)[15:] for b in seen] == cc.tails(7)


def test_receive_file_app_conditions_a_cu8_capture(torch_cuda, tmp_path):
    """apps/lora_receive_file_nogui.py --condition on a cu8 SigMF file (1.0 at 200 LSB) of the SF7 capture behind (2 dB, 10 degrees,
    DC at -6 dBc): the 8 frames come back over UDP."""
    import os
    import socket
    import sys
    from gr_lora_amd import sigmf
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "apps"))
    try:
        import lora_receive_file_nogui as app
    finally:
        sys.path.pop(0)
    base = str(tmp_path / "impaired_cu8")
    sigmf.write_trace(base, cc.impaired_capture(7, 2.0, 10.0, -6.0), 1e6, 868.1e6, 868.1e6, 7, "4/8", 125000, 8, True, False, "", 8, datatype="cu8",
                      full_scale=200.0)
    srv = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    srv.bind(("127.0.0.1", 0))
    srv.settimeout(5.0)                               # (the datagrams are queued by the time main returns: only a failure waits)
    app.main([base, "--port", str(srv.getsockname()[1]), "--chunk", "50001", "--condition"])
    got = [srv.recvfrom(4096)[0] for _ in range(cc.N_FRAMES)]
    srv.close()
    assert [g[15:] for g in got] == cc.tails(7)
