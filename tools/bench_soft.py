"""The soft-decision decoder on its own (gr_lora_amd/csrc/lora_soft.inc.hip), with HIP events, at SF7, SF9 and SF12:

  * lora_hip_soft_symbols_device per window (soft_symbols_kernel: one spectrum and the bit-metric epilogue), beside
    lora_hip_window_stats_device per window (detect_windows_kernel: two spectra and an arg-max) on the same windows;
  * lora_hip_soft_decode_at_headers_device per frame, beside lora_hip_decode_at_headers_device on the same frames.

    python tools/bench_soft.py [--windows 4096] [--frames 64] [--runs 9] [--out profiles/soft_bench.txt]

One JSON line per spreading factor: medians over --runs timed calls behind two warm-up calls, every call between two events on the
stream it runs on (the per-window figures include the upload of the offsets and the download of the results, which both calls make;
kernel times alone: the same command under rocprofv3 --kernel-trace --stats).  The line also records the host's load average when it
was taken: the box is shared.

    python tools/bench_soft.py --repair 8 [--frames 60] [--out profiles/soft_repair_bench.txt]

The CRC-aided repair (lora_hip_soft_crc_repair_enable) instead: per case - SF7 4/5 16 B, SF8 4/8 24 B, SF9 4/6 16 B, valid header
checksum and CRC, true header positions - one line with an SNR sweep in 0.5 dB steps from 3 dB above the working point down to where the soft
decoder alone gets no frame right (frames right with repair off and with 4, 6, 8 and L candidates, frames accepted on bytes that were not sent, the
50 % points and the gain in dB), and one line with the time of the decode call with repair off and on (three medians each) where about half
the frames fail.  With LORA_HIP_LIB naming a library of before the repair (tools/build_variant.sh in a checkout of that commit) the lines hold
the off figures only: the comparison against the parent."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, runs, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms))


def measure(sf, windows, frames, runs, snr_db):
    import torch
    from gr_lora_amd import capi, synth
    reduced = sf >= 11
    cfg = synth.TxConfig(sf=sf, cr=4, reduced_rate=reduced)
    rng = np.random.default_rng(sf)
    n_tx = min(frames, 8 if sf < 12 else 2)                                # frames synthesised; the requests repeat them
    payloads = [bytes(rng.integers(0, 256, 16, dtype=np.uint8)) for _ in range(n_tx)]
    st = synth.build_stream(payloads, cfg, rng=rng, noise_sigma=synth.awgn_sigma_for_snr(snr_db, cfg))
    dev = torch.from_numpy(st.iq.view(np.float32)).to("cuda:0")
    h = capi.Handle(sf=sf, cr=4, reduced_rate=reduced, demod=capi.DEMOD_FFT, disable_drift_correction=True)
    ptr, n = dev.data_ptr(), st.iq.size
    offs = (np.arange(windows, dtype=np.int64) * 977) % (n - cfg.sps)       # windows all over the stream, off the symbol grid
    llr = np.zeros(windows * 12, dtype=np.float32)                         # (the C calls themselves: the wrappers' per-window Python work is not the device's)
    k_out, peak = np.zeros(windows, dtype=np.int32), np.zeros(windows, dtype=np.float32)
    stats = (capi.WindowStats * windows)()

    def soft_symbols():
        h._check(h.L.lora_hip_soft_symbols_device(h.h, ptr, n, offs.ctypes.data, windows, None, llr.ctypes.data, k_out.ctypes.data, peak.ctypes.data, None))

    def window_stats():
        h._check(h.L.lora_hip_window_stats_device(h.h, ptr, n, offs.ctypes.data, windows, stats, None))

    sym_ms, sym_min = _timed(soft_symbols, runs)
    win_ms, win_min = _timed(window_stats, runs)
    pre = [(0, st.header_starts[i % n_tx]) for i in range(frames)]
    got = {}

    def soft():
        got["reports"] = h.soft_decode_at_headers_device(ptr, n, [0], [n], pre)
        got["soft"] = len(h.drain())

    def hard():
        h.decode_at_headers_device(ptr, n, [0], [n], pre)
        got["hard"] = len(h.drain())

    soft_ms, soft_min = _timed(soft, runs)
    hard_ms, hard_min = _timed(hard, runs)
    h.close()
    syms = 8 * frames + sum(r["payload_symbols"] for r in got["reports"])
    us = lambda ms, k: round(1e3 * ms / k, 4)
    return dict(bench="soft", sf=sf, sps=cfg.sps, snr_db=snr_db, windows=windows, frames=frames, runs=runs,
                soft_symbols_us_per_window=us(sym_ms, windows), soft_symbols_us_min=us(sym_min, windows),
                window_stats_us_per_window=us(win_ms, windows), window_stats_us_min=us(win_min, windows),
                soft_over_half_window_stats=round(sym_ms / (0.5 * win_ms), 3),
                soft_call_us_per_frame=us(soft_ms, frames), soft_call_us_min=us(soft_min, frames), soft_symbols_per_call=syms, soft_frames=got["soft"],
                hard_call_us_per_frame=us(hard_ms, frames), hard_call_us_min=us(hard_min, frames), hard_frames=got["hard"],
                soft_over_hard=round(soft_ms / hard_ms, 3), loadavg=[round(v, 2) for v in os.getloadavg()], device=torch.cuda.get_device_name(0))


REPAIR_CASES = [(7, 1, 16, -4.0), (8, 4, 24, -8.5), (9, 2, 16, -11.0)]        # sf, cr, payload bytes, the SNR the sweep starts at (3 dB above the working point)


def _valid_frames(sf, cr, length, n, seed):
    """n frames with a valid header checksum and payload CRC, each a stream of its own, back to back, noiseless
    -> (cfg, iq, header positions, wanted frame bodies)"""
    from gr_lora_amd import synth
    rng = np.random.default_rng(seed)
    cfg = synth.TxConfig(sf=sf, cr=cr, hdr_nibbles=synth.valid_hdr_nibbles(length, cr, True))
    pieces, starts, want, pos = [], [], [], 0
    for _ in range(n):
        p = bytes(rng.integers(0, 256, length, dtype=np.uint8))
        crc = synth.valid_crc_bytes(p)
        st = synth.build_stream([p], cfg, rng=rng, tail_symbols=0.0, crc_bytes=crc)
        pieces.append(st.iq)
        starts.append(pos + st.header_starts[0])
        want.append(synth.expected_frame_tail(p, cfg, crc))
        pos += st.iq.size
    pieces.append(np.zeros(3 * cfg.sps, dtype=np.complex64))
    return cfg, np.concatenate(pieces), starts, want


def _half_point(snrs, counts, n):
    """the SNR at which the count crosses n / 2, linear between the two sweep points around it (None: it never does)"""
    for (s0, c0), (s1, c1) in zip(zip(snrs, counts), zip(snrs[1:], counts[1:])):
        if c0 >= n / 2 > c1:
            return round(s1 + (s0 - s1) * (n / 2 - c1) / (c0 - c1), 2)
    return None


def measure_repair(L, frames, runs):
    """--repair L.  One JSON line per case with the sweep (frames right with repair off and with 4, 6, 8 and L candidates, frames whose CRC holds on
    bytes that were not sent - 'accepted wrong' - off and on, the 50 % points and the gain in dB), then one line with the time of the decode call
    with repair off and on at the SNR of the sweep where the soft decoder alone gets closest to half the frames."""
    import torch
    from gr_lora_amd import capi, synth
    have = hasattr(capi.load(), "lora_hip_soft_crc_repair_enable")           # (a library of before the repair, through LORA_HIP_LIB: the off time only)
    Ls = sorted({4, 6, 8, L}) if have else []
    lines = []
    for sf, cr, length, top in REPAIR_CASES:
        cfg, clean, starts, want = _valid_frames(sf, cr, length, frames, seed=99)
        rng = np.random.default_rng(1000 + sf)
        unit = (rng.standard_normal((clean.size, 2)).astype(np.float32) / np.float32(np.sqrt(2.0))).view(np.complex64)[:, 0]
        h = capi.Handle(samp_rate=cfg.samp_rate, bandwidth=cfg.bw, sf=sf, cr=cr, demod=capi.DEMOD_FFT, disable_drift_correction=True)
        pre = [(0, hp) for hp in starts]
        rows, snr = [], top
        while True:
            iq = clean + np.float32(synth.awgn_sigma_for_snr(snr, cfg)) * unit
            dev = torch.from_numpy(iq.view(np.float32)).to("cuda:0")
            row = dict(snr_db=snr)
            for cand in [0] + Ls:
                if have:
                    h.soft_crc_repair_enable(cand)
                rep = h.soft_decode_at_headers_device(dev.data_ptr(), iq.size, [0], [iq.size], pre)
                got = {i.header_pos: b[15:] for b, i in h.drain()}
                row["right_%d" % cand] = sum(got.get(hp) == w for hp, w in zip(starts, want))
                row["accepted_wrong_%d" % cand] = sum(bool(r["crc_ok"]) and got.get(hp) != w for hp, w, r in zip(starts, want, rep))
                if cand:
                    row["repaired_%d" % cand] = sum(r["status"] == capi.SOFT_REPAIR_REPAIRED for r in h.soft_crc_repair_results())
            rows.append(row)
            if row["right_0"] == 0 or snr < top - 15.0:
                break
            snr -= 0.5
        snrs = [r["snr_db"] for r in rows]
        half = {c: _half_point(snrs, [r["right_%d" % c] for r in rows], frames) for c in [0] + Ls}
        gain = {c: (round(half[0] - half[c], 2) if half[0] is not None and half[c] is not None else None) for c in Ls}
        line = dict(bench="soft_repair_sweep", sf=sf, cr=cr, payload=length, frames=frames, half_point_db=half, gain_db=gain, sweep=rows)
        # the cost, where the soft decoder alone gets closest to half the frames
        mid = min(rows, key=lambda r: abs(r["right_0"] - frames / 2))["snr_db"]
        iq = clean + np.float32(synth.awgn_sigma_for_snr(mid, cfg)) * unit
        dev = torch.from_numpy(iq.view(np.float32)).to("cuda:0")
        reports = (capi.SoftReport * len(pre))()
        o, l = np.zeros(1, dtype=np.uint64), np.array([iq.size], dtype=np.uint64)
        arr = (capi.Preamble * len(pre))()
        for i, (s, hp) in enumerate(pre):
            arr[i].stream, arr[i].header_pos = s, hp

        def call():                                                        # (the C call and the drain, not the wrapper's per-frame Python work)
            h._check(h.L.lora_hip_soft_decode_at_headers_device(h.h, dev.data_ptr(), iq.size, o.ctypes.data, l.ctypes.data, 1, arr, len(pre), 0, reports, None))
            h.drain()

        cost = dict(bench="soft_repair_cost", sf=sf, cr=cr, payload=length, frames=frames, snr_db=mid, runs=runs)
        for cand in [0] + ([L] if have else []):
            if have:
                h.soft_crc_repair_enable(cand)
            samples = [_timed(call, runs)[0] for _ in range(3)]            # three medians: their spread is what a difference is held against
            cost["call_us_per_frame_%s" % ("off" if cand == 0 else "on_%d" % cand)] = [round(1e3 * v / frames, 3) for v in samples]
        cost.update(loadavg=[round(v, 2) for v in os.getloadavg()], device=torch.cuda.get_device_name(0), library=os.path.relpath(os.environ["LORA_HIP_LIB"]) if os.environ.get("LORA_HIP_LIB") else "built")
        h.close()
        lines += [line, cost]
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--snr", type=float, default=0.0, help="in-band SNR of the synthesised frames, dB")
    ap.add_argument("--sf", type=int, action="append")
    ap.add_argument("--out", help="also append the lines to this file")
    ap.add_argument("--repair", type=int, metavar="L", help="instead: the CRC-aided repair with L candidates (1 .. 8) - its gain over an SNR sweep and its cost; "
                                                              "--frames per sweep point (60 there unless given)")
    a = ap.parse_args()
    if a.repair is not None:
        if not 1 <= a.repair <= 8:
            ap.error("--repair takes 1 .. 8")
        lines = [json.dumps(v) for v in measure_repair(a.repair, 60 if a.frames == 64 else a.frames, a.runs)]
    else:
        lines = (json.dumps(measure(sf, a.windows, a.frames, a.runs, a.snr)) for sf in a.sf or (7, 9, 12))
    for line in lines:
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
