"""The soft-decision decoder on its own (gr_lora_amd/csrc/lora_soft.inc.hip), with HIP events, at SF7, SF9 and SF12:

  * lora_hip_soft_symbols_device per window (soft_symbols_kernel: one spectrum and the bit-metric epilogue), beside
    lora_hip_window_stats_device per window (detect_windows_kernel: two spectra and an arg-max) on the same windows;
  * lora_hip_soft_decode_at_headers_device per frame, beside lora_hip_decode_at_headers_device on the same frames.

    python tools/bench_soft.py [--windows 4096] [--frames 64] [--runs 9] [--out profiles/soft_bench.txt]

One JSON line per spreading factor: medians over --runs timed calls behind two warm-up calls, every call between two events on the
stream it runs on (the per-window figures include the upload of the offsets and the download of the results, which both calls make;
kernel times alone: the same command under rocprofv3 --kernel-trace --stats).  The line also records the host's load average when it
was taken: the box is shared."""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--snr", type=float, default=0.0, help="in-band SNR of the synthesised frames, dB")
    ap.add_argument("--sf", type=int, action="append")
    ap.add_argument("--out", help="also append the lines to this file")
    a = ap.parse_args()
    for sf in a.sf or (7, 9, 12):
        line = json.dumps(measure(sf, a.windows, a.frames, a.runs, a.snr))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
