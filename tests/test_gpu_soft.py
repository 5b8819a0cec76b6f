"""Soft-decision decoding on the device (include/lora_hip_soft.h) against its float64 definition (gr_lora_amd/softdecode.py): the bit LLRs of
soft_symbols_kernel, the chain of soft_chain_kernel bit for bit on the device's own LLRs, whole frames against the definition, the gain over
lora_hip_decode_at_headers_device's hard decisions, and lora.weak_signal_receiver end to end.

The LLR bound: an fp32 transform of sps points errs by about eps * log2(sps) * ||x||, 2e-7 of the peak at these SNRs; 1e-4 of the peak leaves
over 100x of room and is still a thousandth of a typical LLR.  A codeword's margin is a sum over eight positions, each an LLR of two maxima:
a frame may differ from the float64 definition's only where some margin is below 16 * 1e-4 * peak, and at most 1 frame in 10 may be set
aside for that.

The hard demodulator (get_shift_fft) folds F[N/2] + F[sps - N/2] into its index N / 2 (decoder_impl.cc:447-450); the soft metric has no fold.  The
sign check against lora_hip_demod_symbols_device therefore holds on every window whose shift is not N / 2; a window whose shift IS N / 2 (at
SF7 and -8 dB the sum of two noise bins does outgrow the symbol's peak now and then) must show in float64 that the folded magnitude reaches the
peak - it is not skipped."""
import numpy as np
import pytest

import soft_cases as SC
from gr_lora_amd import softdecode as SD, synth

pytestmark = pytest.mark.gpu

TOL = 1e-4
RATE = {8: 1e6, 4: 5e5, 2: 2.5e5}


def _dev(iq):
    import torch
    return torch.from_numpy(np.ascontiguousarray(iq).view(np.float32)).cuda()


def _handle(cfg, **kw):
    from gr_lora_amd import capi
    return capi.Handle(samp_rate=cfg.samp_rate, bandwidth=cfg.bw, sf=cfg.sf, cr=cfg.cr, reduced_rate=cfg.reduced_rate, demod=capi.DEMOD_FFT,
                       disable_drift_correction=True, **kw)


def _noisy(sf, decim, reduced, snr_db, seed, n=2, length=12, cr=4):
    cfg = synth.TxConfig(sf=sf, cr=cr, reduced_rate=reduced, samp_rate=RATE[decim])
    rng = np.random.default_rng(seed)
    payloads = [bytes(rng.integers(0, 256, length, dtype=np.uint8)) for _ in range(n)]
    st = synth.build_stream(payloads, cfg, rng=rng, gap_symbols=(1.0, 2.0), noise_sigma=synth.awgn_sigma_for_snr(snr_db, cfg))
    return cfg, st


LLR_CASES = [(7, 8, False, -8.0), (9, 8, False, -13.5), (10, 4, False, -14.0), (12, 8, True, -19.0)]


@pytest.mark.parametrize("sf,decim,reduced,snr_db", LLR_CASES)
def test_llrs_equal_the_definition_and_agree_with_the_hard_demodulator(sf, decim, reduced, snr_db):
    from gr_lora_amd import capi
    cfg, st = _noisy(sf, decim, reduced, snr_db, seed=500 + sf, n=1 if sf == 12 else 2)
    down = SD._down(cfg)
    offs = [st.header_starts[0] + k * cfg.sps for k in range(32)]            # (symbol-aligned windows of a frame: real peaks in noise)
    assert offs[-1] + cfg.sps <= st.iq.size
    flags = [k % 2 for k in range(32)]
    dev = _dev(st.iq)
    h = _handle(cfg)
    L, k_out, peak = h.soft_symbols_device(dev.data_ptr(), st.iq.size, offs, flags)
    bins = h.demod_symbols_device(dev.data_ptr(), st.iq.size, offs, capi.DEMOD_FFT).astype(np.int64)
    h.close()
    worst, checked_k, checked_w, folded = 0.0, 0, 0, 0
    for i, p in enumerate(offs):
        Lm, km, pm, _tot, second = SD.llr_window(st.iq, p, cfg, bool(flags[i]), down)
        assert L[i].size == Lm.size == (sf - 2 if flags[i] else sf)
        err = float(np.abs(L[i].astype(np.float64) - Lm).max())
        worst = max(worst, err / pm)
        assert err <= TOL * pm and abs(float(peak[i]) - pm) <= TOL * pm, (i, err, pm)
        if pm - second > TOL * pm:
            assert int(k_out[i]) == km, (i, k_out[i], km)
            checked_k += 1
        if int(bins[i]) == cfg.nbins // 2:
            # get_shift_fft folds two bins of the sps-point transform into index N / 2 (F[N/2] + F[sps - N/2], :447-450); the soft metric is defined
            # without that fold.  Where the demodulator answers N / 2 its metric is another quantity: the window is held to exactly that instead
            F = np.fft.fft(st.iq[p:p + cfg.sps].astype(np.complex128) * down.astype(np.complex128))
            assert abs(F[cfg.nbins // 2] + F[cfg.sps - cfg.nbins // 2]) >= pm * (1 - TOL), (i, pm)
            folded += 1
            continue
        b = (int(bins[i]) - 1) % cfg.nbins                                  # the FFT demodulator's shift -> its bin (:500) -> its word
        if flags[i]:
            b = ((b + 2) // 4) % (cfg.nbins // 4)
        word = b ^ (b >> 1)
        for bit, v in enumerate(L[i]):
            if abs(float(v)) > TOL * float(peak[i]):
                assert int(v < 0) == (word >> bit) & 1, (i, bit, v, word)
                checked_w += 1
    print("SF%d decimation %d: largest LLR error %.3g of the peak; %d of 32 windows decided by the hard demodulator's folded bin" % (sf, decim, worst, folded))
    assert checked_k >= 24 and folded <= 4 and checked_w >= (32 - folded) * (sf - 2) * 3 // 4


def _model_on_device_llrs(h, dev, n_items, header_positions, cfg, stream_len, require=False):
    """softdecode.soft_chain(dtype=float32) on the LLRs lora_hip_soft_symbols_device returns for the same windows -> [(blob or None, report)]"""
    sps = cfg.sps
    ok = [hp for hp in header_positions if hp + 9 * sps <= stream_len]
    Lh, _, _ = h.soft_symbols_device(dev.data_ptr(), n_items, [hp + k * sps for hp in ok for k in range(8)], [1] * (8 * len(ok)))
    first, offs = {}, []
    for i, hp in enumerate(ok):
        _, rep = SD.soft_chain(np.array(Lh[8 * i:8 * i + 8]), None, cfg, np.float32, require)
        if rep["status"] == SD.STATUS_TRUNCATED and hp + (8 + SD.symbols_taken(rep["payload_symbols"]) + 1) * sps <= stream_len:
            first[hp] = (len(offs), rep["payload_symbols"])
            offs += [hp + (8 + k) * sps for k in range(rep["payload_symbols"])]
    Lp = h.soft_symbols_device(dev.data_ptr(), n_items, offs)[0] if offs else []
    out = []
    for hp in header_positions:
        if hp not in ok:
            out.append((None, dict(status=SD.STATUS_TRUNCATED, payload_symbols=0)))
            continue
        i = ok.index(hp)
        pay = None
        if hp in first:
            at, n_sym = first[hp]
            pay = Lp[at:at + n_sym]
        out.append(SD.soft_chain(np.array(Lh[8 * i:8 * i + 8]), pay, cfg, np.float32, require))
    return out


CHAIN_CASES = [(7, 4, False, -8.0, 12, 16), (7, 1, False, -5.0, 12, 16), (9, 2, False, -12.0, 12, 16), (12, 4, True, -19.0, 4, 8)]


@pytest.mark.parametrize("sf,cr,reduced,snr_db,n,length", CHAIN_CASES)
def test_chain_is_exact_on_the_device_llrs(sf, cr, reduced, snr_db, n, length):
    cfg, _p, iq, starts, _want = SC.gain_stream(sf, cr, length, n, snr_db, reduced, seed=700 + 10 * sf + cr)
    dev = _dev(iq)
    h = _handle(cfg)
    reports = h.soft_decode_at_headers_device(dev.data_ptr(), iq.size, [0], [iq.size], [(0, hp) for hp in starts])
    frames = h.drain()
    model = _model_on_device_llrs(h, dev, iq.size, starts, cfg, iq.size)
    h.close()
    k = 0
    for hp, rep, (blob, mrep) in zip(starts, reports, model):
        assert rep["status"] == mrep["status"], (hp, rep, mrep)
        for key in ("payload_symbols", "codewords", "changed", "cr", "payload_length", "header_checksum_ok", "has_crc", "crc_ok"):
            if key in mrep:
                assert rep[key] == mrep[key], (hp, key, rep, mrep)
        if "min_margin" in mrep:
            assert np.float32(rep["min_margin"]).tobytes() == np.float32(mrep["min_margin"]).tobytes(), (hp, rep["min_margin"], mrep["min_margin"])
            assert abs(rep["mean_abs_llr"] - mrep["mean_abs_llr"]) <= 1e-5 * max(mrep["mean_abs_llr"], 1e-30)
        if blob is not None:
            got, info = frames[k]
            k += 1
            assert got[15:] == blob and got[:15] == bytes(15), hp
            assert (info.stream, info.header_pos, info.end_pos) == (0, hp, hp + (8 + SD.symbols_taken(mrep["payload_symbols"])) * cfg.sps)
    assert k == len(frames) and k >= n // 2


def test_frames_equal_the_float64_definition_and_beat_the_hard_decoder():
    cfg, _p, iq, starts, want = SC.gain_stream(7, 4, 16, 40, -8.0)
    down = SD._down(cfg)
    dev = _dev(iq)
    h = _handle(cfg)
    pre = [(0, hp) for hp in starts]
    h.soft_decode_at_headers_device(dev.data_ptr(), iq.size, [0], [iq.size], pre)
    soft = {i.header_pos: b[15:] for b, i in h.drain()}
    h.decode_at_headers_device(dev.data_ptr(), iq.size, [0], [iq.size], pre)
    hard = {i.header_pos: b[15:] for b, i in h.drain()}
    h.close()
    aside = 0
    for hp in starts:
        blob, rep = SD.decode_frame(iq, hp, cfg, down=down)
        if soft.get(hp) != blob:
            assert rep["min_margin"] < 16 * TOL * rep["peak"], (hp, rep)
            aside += 1
    soft_ok = sum(soft.get(hp) == w for hp, w in zip(starts, want))
    hard_ok = sum(hard.get(hp) == w for hp, w in zip(starts, want))
    print("SF7 4/8 16 B -8 dB on the device: hard %d soft %d of 40, %d set aside" % (hard_ok, soft_ok, aside))
    assert aside <= 4 and soft_ok >= hard_ok + 10


@pytest.mark.parametrize("sf", [7, 8, 9, 10, 12])
def test_clean_frames_equal_the_hard_path(sf):
    from gr_lora_amd import capi
    for cr in (1, 2, 3, 4):
        cfg = synth.TxConfig(sf=sf, cr=cr, reduced_rate=(sf > 10))
        rng = np.random.default_rng(40 * sf + cr)
        payloads = [bytes(rng.integers(0, 256, int(rng.integers(1, 12 if sf > 10 else 30)), dtype=np.uint8)) for _ in range(4)]
        st = synth.build_stream(payloads, cfg, rng=rng, gap_symbols=(1.0, 3.0))
        dev = _dev(st.iq)
        h = _handle(cfg)
        pre = [(0, hp) for hp in st.header_starts]
        h.decode_at_headers_device(dev.data_ptr(), st.iq.size, [0], [st.iq.size], pre)
        hard = [(b[15:], i.stream, i.header_pos, i.end_pos) for b, i in h.drain()]
        reports = h.soft_decode_at_headers_device(dev.data_ptr(), st.iq.size, [0], [st.iq.size], pre)
        soft = [(b[15:], i.stream, i.header_pos, i.end_pos) for b, i in h.drain()]
        h.close()
        assert len(hard) == 4 and soft == hard, (sf, cr)
        assert [b for b, *_ in soft] == [synth.expected_frame_tail(p, cfg) for p in payloads]
        assert all(r["status"] == capi.SOFT_FRAME and r["changed"] == 0 and r["cr"] == cr for r in reports), (sf, cr, reports)


def test_weak_signal_receiver_end_to_end():
    from gr_lora_amd import capi, lora
    n = 30
    cfg, _p, iq, _starts, want = SC.gain_stream(7, 1, 64, n, -2.5, cfo_hz=-1100.0, valid=True)   # (seed: the default, 1000 + 10 sf + cr; on the CPU, with
    down = SD._down(cfg)                                                    # oracle/preamble_oracle.detect and the definition: soft 20, hard 12 of 30)
    got = {}
    for soft in (True, False):
        rx = lora.weak_signal_receiver(cfg.samp_rate, cfg.bw, 7, 1, True, soft=soft)
        pub = []
        rx.subscribe("frames", pub.append)
        got[soft] = rx.work(iq)
        assert pub == [d["frame"] for d in got[soft] if d["frame"] is not None]
        rx.close()
    aside = 0
    for d in got[True]:
        blob, rep = SD.decode_frame(iq, d["header_pos"], cfg, require_header_checksum=True, down=down)
        body = d["frame"][15:] if d["frame"] is not None else None
        if body != blob or d["status"] != rep["status"]:
            assert rep["min_margin"] < 16 * TOL * rep["peak"], (d, rep)
            aside += 1
        assert bool(d["crc_ok"]) == (body in want), d
        assert d["status"] == capi.SOFT_FRAME or d["frame"] is None
    soft_ok = sum(d["frame"] is not None and d["frame"][15:] in want for d in got[True])
    hard_ok = sum(d["frame"] is not None and d["frame"][15:] in want for d in got[False])
    print("SF7 4/5 64 B -2.5 dB, -1100 Hz, detector positions: hard %d soft %d of %d (%d detected), %d set aside" % (hard_ok, soft_ok, n, len(got[True]), aside))
    assert aside <= n // 10 and soft_ok >= hard_ok + n / 4


def test_sc16_capture_equals_its_cf32_conversion():
    from gr_lora_amd import iqformat, lora
    cfg, _p, iq, _starts, _want = SC.gain_stream(7, 4, 16, 4, 0.0, valid=True, seed=9)
    raw = np.clip(np.round(np.ascontiguousarray(iq).view(np.float32) * 2048.0), -32768, 32767).astype(np.int16)
    rx = lora.weak_signal_receiver(cfg.samp_rate, cfg.bw, 7, 4, True)
    a = rx.work(raw)
    b = rx.work(iqformat.to_cf32(raw))
    rx.close()
    assert len(a) == 4 and a == b and all(d["frame"] is not None and d["crc_ok"] for d in a)


def test_edges():
    from gr_lora_amd import capi
    cfg = synth.TxConfig(sf=7, cr=4)
    sps = cfg.sps
    rng = np.random.default_rng(21)
    payloads = [bytes(rng.integers(0, 256, 10, dtype=np.uint8)) for _ in range(3)]
    st = synth.build_stream(payloads, cfg, rng=rng, gap_symbols=(2.0, 3.0), tail_symbols=3.0)
    want = [synth.expected_frame_tail(p, cfg) for p in payloads]
    n_sym = len(st.shifts[0][1])
    noise = (rng.standard_normal(40 * sps) + 1j * rng.standard_normal(40 * sps)).astype(np.complex64)
    iq = np.concatenate([st.iq, noise])
    dev = _dev(iq)
    h = _handle(cfg)
    ptr, one = dev.data_ptr(), ([0], [st.iq.size])
    assert h.soft_decode_at_headers_device(ptr, iq.size, *one, []) == [] and h.drain() == []
    # the second frame's stream ends inside its payload: TRUNCATED, no frame, the neighbours (streams of their own) unaffected
    cut = st.header_starts[1] + (8 + n_sym) * sps                          # (its last symbol has one sps behind it, not two)
    streams = ([0, 0, 0], [st.iq.size, cut, st.iq.size])
    rep = h.soft_decode_at_headers_device(ptr, iq.size, *streams, [(0, st.header_starts[0]), (1, st.header_starts[1]), (2, st.header_starts[2])])
    frames = h.drain()
    assert [r["status"] for r in rep] == [capi.SOFT_FRAME, capi.SOFT_TRUNCATED, capi.SOFT_FRAME] and rep[1]["payload_symbols"] == n_sym
    assert [(b[15:], i.stream, i.header_pos) for b, i in frames] == [(want[0], 0, st.header_starts[0]), (want[2], 2, st.header_starts[2])]
    # the limit itself, against the hard path: a stream that ends exactly 2 sps behind the start of the last symbol publishes in both calls, one item less in neither
    limit = st.header_starts[1] + (8 + n_sym + 1) * sps
    for length, published in ((limit, True), (limit - 1, False)):
        at = ([0, 0], [st.iq.size, length])
        rep = h.soft_decode_at_headers_device(ptr, iq.size, *at, [(1, st.header_starts[1])])
        soft = [(b[15:], i.header_pos, i.end_pos) for b, i in h.drain()]
        h.decode_at_headers_device(ptr, iq.size, *at, [(1, st.header_starts[1])])
        hard = [(b[15:], i.header_pos, i.end_pos) for b, i in h.drain()]
        assert soft == hard == ([(want[1], st.header_starts[1], limit - sps)] if published else []), (length, soft, hard)
        assert rep[0]["status"] == (capi.SOFT_FRAME if published else capi.SOFT_TRUNCATED)
    h.decode_at_headers_device(ptr, iq.size, *streams, [(1, st.header_starts[1])])
    assert h.drain() == []                                                  # (the hard path publishes nothing there either)
    # a header inside the last 2 sps of its stream: ERR_ARG, as in the hard call
    for call in (h.soft_decode_at_headers_device, h.decode_at_headers_device):
        with pytest.raises(capi.LoraHipError) as e:
            call(ptr, iq.size, *one, [(0, st.iq.size - 2 * sps + 1)])
        assert e.value.status == -6
    with pytest.raises(capi.LoraHipError):
        h.soft_decode_at_headers_device(ptr, iq.size, *one, [(1, st.header_starts[0])])
    # pure noise passed as a header: rejected by the checksum flag, no payload demodulated
    npos = [st.iq.size + k * 3 * sps for k in range(8)]
    rep = h.soft_decode_at_headers_device(ptr, iq.size, [0], [iq.size], [(0, p) for p in npos], capi.SOFT_REQUIRE_HEADER_CHECKSUM)
    assert h.drain() == []
    for p, r in zip(npos, rep):
        _, m = SD.decode_frame(iq, p, cfg, require_header_checksum=True)
        assert r["status"] in (capi.SOFT_HEADER_REJECTED, capi.SOFT_CR_ZERO) and r["payload_symbols"] == 0 and r["status"] == m["status"], (r, m)
    assert sum(r["status"] == capi.SOFT_HEADER_REJECTED for r in rep) >= 6
    h.close()


def test_sf6_is_refused():
    """The soft decoder covers SF 7 .. 12: an SF6 handle (explicit header: its block holds 4 codewords, not the header's 5) gets BAD_CONFIG, no frame."""
    import torch
    from gr_lora_amd import capi, lora
    h = capi.Handle(sf=6, cr=4, samp_rate=5e5, demod=capi.DEMOD_FFT, disable_drift_correction=True)
    dev = torch.zeros(2 * 64 * h.sps, dtype=torch.float32, device="cuda")
    with pytest.raises(capi.LoraHipError) as e:
        h.soft_decode_at_headers_device(dev.data_ptr(), 64 * h.sps, [0], [64 * h.sps], [(0, 4 * h.sps)])
    assert e.value.status == -2 and h.drain() == []
    h.close()
    with pytest.raises(ValueError):
        lora.weak_signal_receiver(5e5, 125000, 6, 4, True)
