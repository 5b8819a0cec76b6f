"""Rational resampler (lora_hip_resampler_*) on device-resident captures: one JSON line per ratio and input format.

    python tools/bench_resampler.py [--ratio L/M ...] [--items N] [--runs R] [--format cf32|sc16|sc8|cu8 ...]

Ratios (default: all six): 5/6 (2.4 -> 2.0 Msps), 125/128 (2.048 -> 2.0), 25/32 (2.56 -> 2.0), 25/24 (1.92 -> 2.0), 5/12 (2.4 -> 1.0),
125/256 (2.048 -> 1.0), each on cf32 and cu8 unless --format names others, at 2^24 input items.
Time = kernel time by HIP events (lora_hip_resampler_last_kernel_ms: the one launch of a call), median of --runs runs after one
warm-up run; the timed runs continue one stream, so every run computes the same amount (to within one output).  Bytes moved = the
input items once (8 / 4 / 2 B each) + 8 B per output, i.e. 8 B + 8 B * L / M per input item for cf32; fractions against 8 TB/s (spec)
and 6.29 TB/s (measured float4 copy).  The fractions are those algorithmic bytes over the time, not measured HBM traffic: the same
buffer is read again in every run, and at 2^24 items the input (cf32: 128 MiB, cu8: 32 MiB) fits in the 256 MB Infinity Cache.  The
kernel also does Q fused multiply-adds per output and component, which is what bounds it: gflops is 4 Q flops per output over the time.
The last line is the channeliser (decimation 1, one channel, the 241-tap filter of tools/bench_channelizer.py) on the same cf32 buffer
on the same machine, as orientation: the stage the resampler's output goes into.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RATIOS = ["5/6", "125/128", "25/32", "25/24", "5/12", "125/256"]
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


def _time(run, kernel_ms, runs):
    run()                                      # warm-up (code object load, first touch)
    ms = []
    for _ in range(runs):
        run()
        ms.append(kernel_ms())
    return float(np.median(ms)), [round(m, 4) for m in ms]


def _input(items, fmt):
    import torch
    from gr_lora_amd import iqformat
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(items) + 1j * rng.standard_normal(items)).astype(np.complex64)
    if fmt == iqformat.CF32:
        return torch.from_numpy(x.view(np.float32)).to("cuda:0")
    info = np.iinfo(iqformat.DTYPES[fmt])
    return torch.from_numpy(iqformat.quantize(x, fmt, 0.9 * info.max / float(np.abs(x.view(np.float32)).max()))).to("cuda:0")


def measure(ratio, items, runs, fmt_name, d_in):
    import torch
    from gr_lora_amd import capi, iqformat
    fmt = iqformat.format_from_name(fmt_name)
    L, M = (int(v) for v in ratio.split("/"))
    rs = capi.Resampler(L, M)
    L, M, Q = rs.ratio()
    cap = items * L // M + 2
    d_out = torch.empty(cap, dtype=torch.complex64, device="cuda:0")
    outs = []

    def run():
        if fmt == iqformat.CF32:
            outs.append(rs.run_device(d_in.data_ptr(), items, d_out.data_ptr(), cap)[0])
        else:
            outs.append(rs.run_device_raw(d_in.data_ptr(), items, fmt, d_out.data_ptr(), cap)[0])

    ms, all_ms = _time(run, rs.kernel_ms, runs)
    n_out = int(np.median(outs[1:]))
    nbytes = float(iqformat.ITEM_BYTES[fmt]) * items + 8.0 * n_out
    tile, per_group, stride, lds = rs.plan()
    line = dict(ratio="%d/%d" % (L, M), format=fmt_name, q=Q, tile=tile, tiles_per_group=per_group, lds_bytes=lds, items=items, outputs=n_out,
                resampler_ms=round(ms, 4), resampler_runs_ms=all_ms, gitems_in_per_s=round(items / ms / 1e6, 3), gb_per_s=round(nbytes / ms / 1e6, 1),
                frac_hbm_spec=round(nbytes / ms * 1e3 / HBM_SPEC, 4), frac_hbm_copy=round(nbytes / ms * 1e3 / HBM_COPY, 4),
                gflops=round(4.0 * Q * n_out / ms / 1e6, 1))
    rs.close()
    return line


def channelizer_line(items, runs, d_in):
    import torch
    from gr_lora_amd import capi
    ch = capi.Channelizer(1e6, 868.0e6, [868.1e6], 125000, 1)
    no = ch.output_items(items)
    d_out = torch.empty(2 * no, dtype=torch.float32, device="cuda:0")
    ms, all_ms = _time(lambda: ch.run_device(d_in.data_ptr(), items, d_out.data_ptr(), no), ch.kernel_ms, runs)
    ch.close()
    return dict(orientation="channelizer, decimation 1, 1 channel, cf32", items=items, channelizer_ms=round(ms, 4), channelizer_runs_ms=all_ms,
                gitems_in_per_s=round(items / ms / 1e6, 3), gb_per_s=round(16.0 * items / ms / 1e6, 1))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ratio", action="append", help="L/M (default: the six of the module text)")
    ap.add_argument("--items", type=int, default=1 << 24, help="input items per run (default 2^24)")
    ap.add_argument("--runs", type=int, default=7, help="timed runs per measurement (median; at least 5)")
    ap.add_argument("--format", choices=["cf32", "sc16", "sc8", "cu8"], action="append", help="input format (default: cf32 and cu8)")
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: at least 5")
    from gr_lora_amd import iqformat
    cf32 = None
    for fmt in a.format or ["cf32", "cu8"]:
        d_in = _input(a.items, iqformat.format_from_name(fmt))
        if fmt == "cf32":
            cf32 = d_in
        for ratio in a.ratio or RATIOS:
            print(json.dumps(measure(ratio, a.items, a.runs, fmt, d_in)), flush=True)
    print(json.dumps(channelizer_line(a.items, a.runs, cf32 if cf32 is not None else _input(a.items, iqformat.CF32))), flush=True)


if __name__ == "__main__":
    main()
