"""The traffic synthesiser's kernel (csrc/lora_tx.hip, lora.traffic_synthesizer) against the numpy path it replaces: one JSON line
per case.

    python tools/bench_tx.py [--case a|b|single] [--seconds S] [--passes P] [--no-host] [--out profiles/tx_bench_lines.jsonl]

Cases:
    a, b    tools/bench_gateway.py's plans (EU868-like: 8 channels at 2 Msps; US915-like: 64 channels at 16 Msps) continued per
            channel to --seconds of air (default 10): bench_gateway.layout
    single  one emitter at 1 Msps: SF7 frames back to back for --seconds of air
Device figure: the capture generated in chunks of 2^22 items into one reused HBM buffer; the time is the sum of the kernel times
of a pass (HIP events around each launch, lora_hip_tx_last_kernel_ms), median of --passes (7) passes after one warm-up pass, each
pass on a fresh stream with the same frames.  pairs_per_s counts (item, emitter) pairs the kernel evaluated: the items each
frame covers, summed.  bytes_per_s is the 8 bytes written per item.
Host figure (unless --no-host): wall time of the numpy construction in the same process, once: bench_gateway.synthesise(case) for a
and b - its own plan, 1.7 s of air of the same density, so the comparison is by rate - and synth.build_stream of the same frames
for single.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CHUNK = 1 << 22


def single_plan(seconds):
    """[(0, 7, start, payload)] at 1 Msps, 4 to 6 symbols apart, and the items of the capture."""
    from gr_lora_amd import synth
    rng = np.random.default_rng(7)
    n, sps = int(seconds * 1e6), 1024
    frames, pos = [], 2000
    while True:
        pl = bytes(rng.integers(0, 256, 16, dtype=np.uint8))
        items = (8 + 4 + 8 + synth.payload_symbol_count(18, 7, 4, False)) * sps + sps // 4
        if pos + items + 4 * sps > n:
            return frames, n
        frames.append((0, 7, pos, pl))
        pos += items + int(rng.integers(4 * sps, 6 * sps))


def device_pass(fs, freq_of, frames, n, buf):
    from gr_lora_amd import lora
    tx = lora.traffic_synthesizer(fs)
    for k, sf, start, pl in frames:
        tx.add_frame(pl, sf, 4, 125000, start, freq_of(k))
    ms = 0.0
    t0 = time.perf_counter()
    for i in range(0, n, CHUNK):
        m = min(CHUNK, n - i)
        tx.generate(m, out=buf[:m])
        ms += tx.kernel_ms()
    wall = time.perf_counter() - t0
    assert tx.pending == 0
    tx.close()
    return ms, wall


def measure(case, seconds, passes, host):
    import torch
    import bench_gateway as bg
    from gr_lora_amd import lora, synth
    if case == "single":
        fs, freq_of = 1e6, (lambda k: 0.0)
        frames, n = single_plan(seconds)
    else:
        w = bg.WORKLOADS[case]
        fs, freq_of = w["fs"], (lambda k: w["f0"] + k * w["fs"] / w["M"])
        frames, _expect, n = bg.layout(case, seconds)
    D = int(fs / 125000)
    pairs = sum((8 + 4 + 8 + synth.payload_symbol_count(len(pl) + 2, sf, 4, lora.lorawan_reduced_rate(sf, 125000))) * (D << sf) + (D << sf) // 4
                for _k, sf, _s, pl in frames)
    buf = torch.empty(min(CHUNK, n), dtype=torch.complex64, device="cuda:0")
    device_pass(fs, freq_of, frames, n, buf)               # warm-up
    res = [device_pass(fs, freq_of, frames, n, buf) for _ in range(passes)]
    ms = float(np.median([r[0] for r in res]))
    line = dict(bench="tx", case=case, samp_rate=fs, air_s=round(n / fs, 4), items=n, frames=len(frames), pairs=pairs,
                mean_emitters_per_item=round(pairs / n, 3), chunk_items=CHUNK, passes=passes, kernel_ms=round(ms, 3),
                kernel_ms_passes=[round(r[0], 3) for r in res], wall_s=round(float(np.median([r[1] for r in res])), 4),
                items_per_s=round(n / (ms * 1e-3), 1), pairs_per_s=round(pairs / (ms * 1e-3), 1), bytes_per_s=round(8 * n / (ms * 1e-3), 1))
    if host:
        t0 = time.perf_counter()
        if case == "single":
            pos, pieces = 0, []
            for _k, _sf, start, pl in frames:                # (build_stream takes one CRC for all its frames: one call per frame)
                cfg = synth.TxConfig(sf=7, cr=4, hdr_nibbles=synth.valid_hdr_nibbles(len(pl), 4, True))
                pieces.append(synth.build_stream([pl], cfg, gaps=[start - pos], tail_symbols=0.0, crc_bytes=synth.valid_crc_bytes(pl)).iq)
                pos += pieces[-1].size
            host_items = int(np.concatenate(pieces + [np.zeros(n - pos, dtype=np.complex64)]).size)
        else:
            host_items = int(bg.synthesise(case)[0].size)
        dt = time.perf_counter() - t0
        line.update(host_items=host_items, host_air_s=round(host_items / fs, 4), host_s=round(dt, 4), host_items_per_s=round(host_items / dt, 1),
                    device_over_host_rate=round((n / (ms * 1e-3)) / (host_items / dt), 1))
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--case", choices=["a", "b", "single"], action="append")
    ap.add_argument("--seconds", type=float, default=10.0, help="seconds of air the device generates")
    ap.add_argument("--passes", type=int, default=7, help="timed passes (median)")
    ap.add_argument("--no-host", action="store_true", help="the device only (profiler runs)")
    ap.add_argument("--out", help="also append the lines to this file")
    a = ap.parse_args()
    for case in a.case or ["a", "b", "single"]:
        line = json.dumps(measure(case, a.seconds, a.passes, not a.no_host))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
