"""CRC-aided repair on the device (soft_repair_kernel; include/lora_hip_soft.h) against its definition (gr_lora_amd/softdecode.py crc_repair):
the kernel alone on codewords, bit for bit; in the decode call on the device's own LLRs; off again after having been on; and
lora.weak_signal_receiver(crc_repair=8) end to end against the float64 definition.

Everything the kernel does is integer arithmetic but the penalty, a sum of at most eight fp32 margins in a stated order: bodies and records are
compared exactly, the penalty by its bytes.  End to end the margins themselves carry the fp32 spectrum's error, so a frame may differ from the
float64 definition's where some margin is below 16 * TOL * peak (tests/test_gpu_soft.py has the bound's derivation)."""
import numpy as np
import pytest

import soft_cases as SC
import soft_repair_cases as RC
from gr_lora_amd import softdecode as SD

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _dev(iq):
    import torch
    return torch.from_numpy(np.ascontiguousarray(iq).view(np.float32)).cuda()


def _handle(cfg, **kw):
    from gr_lora_amd import capi
    return capi.Handle(samp_rate=cfg.samp_rate, bandwidth=cfg.bw, sf=cfg.sf, cr=cfg.cr, reduced_rate=cfg.reduced_rate, demod=capi.DEMOD_FFT,
                       disable_drift_correction=True, **kw)


def _same_record(got, want):
    assert set(got) == set(want)
    for key in want:
        if key == "penalty":
            assert np.float32(got[key]).tobytes() == np.float32(want[key]).tobytes(), (got, want)
        else:
            assert got[key] == want[key], (key, got, want)


def test_the_kernel_alone_equals_the_definition():
    from gr_lora_amd import capi, synth
    cases = list(RC.edge_cases()) + list(RC.random_cases())
    assert len(cases) >= 200 + 15
    h = _handle(synth.TxConfig(sf=7, cr=4))
    seen = {}
    for L in range(1, 9):                                                      # (the candidate count belongs to the call: one call per value)
        group = [c for c in cases if c[5] == L]
        if not group:
            continue
        bodies, recs = h.soft_crc_repair_codewords([c[1] for c in group], sum((c[2] for c in group), []), sum((c[3] for c in group), []),
                                                   sum((c[4] for c in group), []), L)
        for (name, length, nib, sec, mar, _L), body, rec in zip(group, bodies, recs):
            new, want = SD.crc_repair(nib, sec, mar, length + 2, L, np.float32)
            assert body == bytes(SD.body_bytes(new, length + 2)), (name, rec, want)
            _same_record(rec, want)
            seen[rec["status"]] = seen.get(rec["status"], 0) + 1
    # what is refused, on a real handle: the checks that need one
    rec = (capi.SoftRepair * 3)()
    assert h.L.lora_hip_soft_crc_repair_enable(h.h, 9) == -6
    assert h.L.lora_hip_soft_crc_repair_results(h.h, rec, 0) == 0              # (no decode call yet: no entries)
    assert h.L.lora_hip_soft_crc_repair_results(h.h, rec, 3) == -6             # a mismatching n
    with pytest.raises(capi.LoraHipError):
        h.soft_crc_repair_codewords([256], [0] * 516, [1] * 516, [0.0] * 516, 8)
    with pytest.raises(capi.LoraHipError):
        h.soft_crc_repair_codewords([0], [0, 16, 0, 0], [1] * 4, [0.0] * 4, 8)
    h.close()
    print("kernel alone: %d frames, by status %s" % (len(cases), seen))
    assert seen.get(SD.REPAIR_REPAIRED, 0) >= 40 and seen.get(SD.REPAIR_FAILED, 0) >= 10 and seen.get(SD.REPAIR_CRC_HELD, 0) >= 5


def _model_on_device_llrs(h, dev, n_items, header_positions, cfg, stream_len, require=False, crc_repair=0):
    """softdecode.soft_chain(dtype=float32, crc_repair) on the LLRs lora_hip_soft_symbols_device returns for the same windows -> [(blob or None, report)]
    (the way of tests/test_gpu_soft.py, with the repair)"""
    sps = cfg.sps
    ok = [hp for hp in header_positions if hp + 9 * sps <= stream_len]
    Lh, _, _ = h.soft_symbols_device(dev.data_ptr(), n_items, [hp + k * sps for hp in ok for k in range(8)], [1] * (8 * len(ok)))
    first, offs = {}, []
    for i, hp in enumerate(ok):
        _, rep = SD.soft_chain(np.array(Lh[8 * i:8 * i + 8]), None, cfg, np.float32, require, crc_repair)
        if rep["status"] == SD.STATUS_TRUNCATED and hp + (8 + SD.symbols_taken(rep["payload_symbols"]) + 1) * sps <= stream_len:
            first[hp] = (len(offs), rep["payload_symbols"])
            offs += [hp + (8 + k) * sps for k in range(rep["payload_symbols"])]
    Lp = h.soft_symbols_device(dev.data_ptr(), n_items, offs)[0] if offs else []
    out = []
    for hp in header_positions:
        if hp not in ok:
            out.append((None, dict(status=SD.STATUS_TRUNCATED, payload_symbols=0, repair=SD.no_repair(dtype=np.float32))))
            continue
        i = ok.index(hp)
        pay = None
        if hp in first:
            at, n_sym = first[hp]
            pay = Lp[at:at + n_sym]
        out.append(SD.soft_chain(np.array(Lh[8 * i:8 * i + 8]), pay, cfg, np.float32, require, crc_repair))
    return out


CHAIN_CASES = [(7, 1, 16, -7.0), (9, 2, 16, -14.0), (8, 4, 24, -11.5)]       # (SF9: the two spare header codewords are eligible)


@pytest.mark.parametrize("sf,cr,length,snr_db", CHAIN_CASES)
def test_in_the_chain_it_equals_the_definition_on_the_device_llrs(sf, cr, length, snr_db):
    cfg, _p, iq, starts, want = SC.gain_stream(sf, cr, length, 12, snr_db, valid=True, seed=99)
    dev = _dev(iq)
    h = _handle(cfg)
    h.soft_crc_repair_enable(8)
    reports = h.soft_decode_at_headers_device(dev.data_ptr(), iq.size, [0], [iq.size], [(0, hp) for hp in starts])
    records = h.soft_crc_repair_results()
    frames = h.drain()
    model = _model_on_device_llrs(h, dev, iq.size, starts, cfg, iq.size, crc_repair=8)
    h.close()
    k, by_status = 0, {}
    for hp, rep, rec, (blob, mrep) in zip(starts, reports, records, model):
        assert rep["status"] == mrep["status"], (hp, rep, mrep)
        for key in ("payload_symbols", "codewords", "changed", "cr", "payload_length", "header_checksum_ok", "has_crc", "crc_ok"):
            if key in mrep:
                assert rep[key] == mrep[key], (hp, key, rep, mrep)
        if "min_margin" in mrep:
            assert np.float32(rep["min_margin"]).tobytes() == np.float32(mrep["min_margin"]).tobytes(), (hp, rep["min_margin"], mrep["min_margin"])
        _same_record(rec, mrep["repair"])
        by_status[rec["status"]] = by_status.get(rec["status"], 0) + 1
        if blob is not None:
            got, _info = frames[k]
            k += 1
            assert got[15:] == blob and got[:15] == bytes(15), (hp, rec)
    print("SF%d 4/%d %.1f dB: %d frames of 12, repair records by status %s" % (sf, 4 + cr, snr_db, k, by_status))
    assert k == len(frames) and k >= 6 and by_status.get(SD.REPAIR_REPAIRED, 0) >= 1


def test_off_after_on_is_as_if_never_on():
    from gr_lora_amd import capi
    cfg, _p, iq, starts, _want = SC.gain_stream(7, 1, 16, 12, -7.0, valid=True, seed=99)
    dev = _dev(iq)
    pre = [(0, hp) for hp in starts]
    never, toggled = _handle(cfg), _handle(cfg)
    want_rep = never.soft_decode_at_headers_device(dev.data_ptr(), iq.size, [0], [iq.size], pre)
    want = [(b, i.stream, i.header_pos, i.end_pos) for b, i in never.drain()]
    assert [r["status"] for r in never.soft_crc_repair_results()] == [capi.SOFT_REPAIR_NOT_ATTEMPTED] * len(pre)
    toggled.soft_crc_repair_enable(8)
    on_rep = toggled.soft_decode_at_headers_device(dev.data_ptr(), iq.size, [0], [iq.size], pre)
    on = [(b, i.stream, i.header_pos, i.end_pos) for b, i in toggled.drain()]
    on_rec = toggled.soft_crc_repair_results()
    toggled.soft_crc_repair_enable(0)
    off_rep = toggled.soft_decode_at_headers_device(dev.data_ptr(), iq.size, [0], [iq.size], pre)
    off = [(b, i.stream, i.header_pos, i.end_pos) for b, i in toggled.drain()]
    off_rec = toggled.soft_crc_repair_results()
    never.close()
    toggled.close()
    assert off == want and off_rep == want_rep
    assert all(r == SD.no_repair(dtype=np.float32) for r in off_rec) and len(off_rec) == len(pre)
    # and while it was on: other bytes exactly in the frames it repaired, crc_ok that of the published frame
    assert len(on) == len(want)
    k = 0
    for r_on, r_off, rec in zip(on_rep, want_rep, on_rec):
        assert {key: v for key, v in r_on.items() if key != "crc_ok"} == {key: v for key, v in r_off.items() if key != "crc_ok"}
        if r_on["status"] != capi.SOFT_FRAME:
            assert rec["status"] == capi.SOFT_REPAIR_NOT_ATTEMPTED
            continue
        blob_on, blob_off = on[k][0], want[k][0]
        k += 1
        if not r_on["has_crc"]:                                                 # (a header lost to noise may say so)
            assert rec["status"] == capi.SOFT_REPAIR_NOT_ATTEMPTED and blob_on == blob_off
            continue
        assert r_on["crc_ok"] == capi.check_frame(blob_on).crc_ok
        assert (blob_on != blob_off) == (rec["status"] == capi.SOFT_REPAIR_REPAIRED) and blob_on[:18] == blob_off[:18]
        assert (rec["status"] == capi.SOFT_REPAIR_CRC_HELD) == bool(r_off["crc_ok"]) and rec["status"] != capi.SOFT_REPAIR_NOT_ATTEMPTED
    assert any(rec["status"] == capi.SOFT_REPAIR_REPAIRED for rec in on_rec)


def test_weak_signal_receiver_with_repair_end_to_end():
    from gr_lora_amd import capi, lora
    n = 60
    cfg, _p, iq, _starts, want = SC.gain_stream(7, 1, 16, n, -7.0, valid=True, seed=99)
    down = SD._down(cfg)
    got = {}
    for L in (0, 8):
        rx = lora.weak_signal_receiver(cfg.samp_rate, cfg.bw, 7, 1, True, crc_repair=L)
        got[L] = rx.work(iq)
        rx.close()
    assert all("repair" not in d for d in got[0]) and all("repair" in d for d in got[8])
    assert [d["header_pos"] for d in got[0]] == [d["header_pos"] for d in got[8]]
    aside = 0
    for d in got[8]:
        blob, rep = SD.decode_frame(iq, d["header_pos"], cfg, require_header_checksum=True, down=down, crc_repair=8)
        body = d["frame"][15:] if d["frame"] is not None else None
        if body != blob or d["status"] != rep["status"] or d["repair"]["status"] != rep["repair"]["status"]:
            assert rep["min_margin"] < 16 * TOL * rep["peak"], (d, rep)
            aside += 1
        assert d["status"] == capi.SOFT_FRAME or d["frame"] is None
        if d["frame"] is not None:
            assert bool(d["crc_ok"]) == bool(capi.check_frame(d["frame"]).crc_ok)
            assert bool(d["crc_ok"]) == (d["repair"]["status"] in (capi.SOFT_REPAIR_CRC_HELD, capi.SOFT_REPAIR_REPAIRED))
    good = {L: sum(d["frame"] is not None and d["frame"][15:] in want for d in got[L]) for L in (0, 8)}
    repaired = [d for d in got[8] if d["repair"]["status"] == capi.SOFT_REPAIR_REPAIRED]
    wrong = sum(d["frame"][15:] not in want for d in repaired)
    print("SF7 4/5 16 B -7 dB, detector positions: %d good of %d, %d with crc_repair=8; %d repaired, %d of them to bytes not sent; %d set aside" %
          (good[0], n, good[8], len(repaired), wrong, aside))
    assert aside <= 4 and good[8] >= good[0] + 10
