"""The link-metrics window kernel (gr_lora_amd/csrc/lora_link.hip) on its own: milliseconds per 1 000 frames (6 000 windows) at
SF7, SF9 and SF12, through lora_hip_link_measure_device on a device-resident stream; the kernel's time from HIP events
(lora_hip_link_stats), the call's wall time beside it.

    python tools/bench_link.py [--frames 1000] [--runs 7] [--out profiles/link_bench_lines.jsonl]

One JSON line per spreading factor.  The stream is one synthesised frame in noise (25 dB); the requests are the same header
position 1 000 times, so every window is read from L2 after the first: the figure is the kernel's arithmetic and LDS time, not
an HBM rate.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def measure(sf, frames, runs):
    import torch
    from gr_lora_amd import capi, synth
    cfg = synth.TxConfig(sf=sf, cr=4, reduced_rate=sf >= 11)
    st = synth.build_stream([b"\x01\x02\x03\x04"], cfg, lead=4 * cfg.sps, noise_sigma=synth.awgn_sigma_for_snr(25.0, cfg))
    dev = torch.from_numpy(st.iq.view(np.float32)).to("cuda:0")
    h = capi.Handle(sf=sf, cr=4, reduced_rate=sf >= 11)
    req = [(0, st.header_starts[0])] * frames
    h.measure_link_device(dev.data_ptr(), st.iq.size, [0], [st.iq.size], req)      # warm-up (builds the Hann table)
    kernel, wall = [], []
    for _ in range(runs):
        before = h.link_stats()["kernel_ms"]
        t0 = time.perf_counter()
        mets = h.measure_link_device(dev.data_ptr(), st.iq.size, [0], [st.iq.size], req)
        wall.append(1e3 * (time.perf_counter() - t0))
        kernel.append(h.link_stats()["kernel_ms"] - before)
    h.close()
    scale = 1000.0 / frames
    return dict(bench="link_windows", sf=sf, sps=cfg.sps, frames=frames, windows=6 * frames, runs=runs,
                kernel_ms_per_1000_frames=round(float(np.median(kernel)) * scale, 4), kernel_ms_min=round(min(kernel) * scale, 4),
                call_ms_per_1000_frames=round(float(np.median(wall)) * scale, 4), snr_db=round(mets[0].snr_db, 2), flags=int(mets[0].flags))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--sf", type=int, action="append")
    ap.add_argument("--out", help="also append the lines to this file")
    a = ap.parse_args()
    for sf in a.sf or (7, 9, 12):
        line = json.dumps(measure(sf, a.frames, a.runs))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
