"""IQ conditioner (lora_hip_conditioner_*) on device-resident captures: one JSON line per input format and size.

    python tools/bench_conditioner.py [--items N ...] [--runs R] [--format cf32|sc16|sc8|cu8 ...] [--block B] [--window W]

Defaults: every format at 2^22 and 2^26 items, B = 4096, W = 16.  Time = kernel time by HIP events (lora_hip_conditioner_last_kernel_ms:
both launches of a call), median of --runs runs after one warm-up run; the items are a whole number of blocks, so every run
computes the same amount.  The input is read twice, once by each kernel.  Two byte models, per item:
    twice   2 x item bytes read + 8 written (cf32 24 B, sc16 16 B, sc8 / cu8 12 B): both reads come from HBM
    once    item bytes read + 8 written (cf32 16 B, sc16 12 B, sc8 / cu8 10 B): the second read hits the 256 MiB Infinity Cache
Each line gives both as GB/s and as a fraction of 6.29 TB/s, the measured float4 copy.  A fraction above 1 under "twice" says the
second read did not come from HBM.  These are algorithmic bytes over the time, not measured traffic, and the same buffer is read
again in every run: at 2^22 items the whole input (cf32: 32 MiB) stays in the Infinity Cache from run to run.
"""
from __future__ import annotations

import argparse
import functools
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_COPY = 6.29e12


@functools.lru_cache(maxsize=1)
def _capture(items):
    """Circular noise behind 2 dB / 10 degrees of mismatch and a DC offset (float32 throughout: 2^26 items are made once)."""
    rng = np.random.default_rng(1)
    v = rng.standard_normal((items, 2), dtype=np.float32) * np.float32(0.2)
    g, phi = 10.0 ** 0.1, np.radians(10.0)
    v[:, 1] = np.float32(g * np.cos(phi)) * v[:, 1] + np.float32(g * np.sin(phi)) * v[:, 0] + np.float32(0.05)
    v[:, 0] += np.float32(0.1)
    return v.reshape(-1).view(np.complex64)


def _input(items, fmt):
    import torch
    from gr_lora_amd import iqformat
    x = _capture(items)
    if fmt == iqformat.CF32:
        return torch.from_numpy(x.view(np.float32)).to("cuda:0")
    info = np.iinfo(iqformat.DTYPES[fmt])
    return torch.from_numpy(iqformat.quantize(x, fmt, 0.9 * info.max / float(np.abs(x.view(np.float32)).max()))).to("cuda:0")


def measure(items, runs, fmt_name, block, window):
    import torch
    from gr_lora_amd import capi, iqformat
    fmt = iqformat.format_from_name(fmt_name)
    items = items // block * block
    d_in = _input(items, fmt)
    d_out = torch.empty(items, dtype=torch.complex64, device="cuda:0")
    h = capi.Conditioner(block, window)

    def run():
        if fmt == iqformat.CF32:
            got = h.run_device(d_in.data_ptr(), items, d_out.data_ptr(), items)[0]
        else:
            got = h.run_device_raw(d_in.data_ptr(), items, fmt, d_out.data_ptr(), items)[0]
        assert got == items

    run()                                      # warm-up (code object load, first touch)
    ms = []
    for _ in range(runs):
        run()
        ms.append(h.kernel_ms())
    h.close()
    med = float(np.median(ms))
    ib = float(iqformat.ITEM_BYTES[fmt])
    twice, once = (2.0 * ib + 8.0) * items, (ib + 8.0) * items
    return dict(format=fmt_name, items=items, block=block, window=window, conditioner_ms=round(med, 4), runs_ms=[round(m, 4) for m in ms],
                gitems_per_s=round(items / med / 1e6, 3), gb_per_s_read_twice=round(twice / med / 1e6, 1), gb_per_s_read_once=round(once / med / 1e6, 1),
                frac_copy_read_twice=round(twice / med * 1e3 / HBM_COPY, 4), frac_copy_read_once=round(once / med * 1e3 / HBM_COPY, 4))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--items", type=int, action="append", help="input items per run (default: 2^22 and 2^26)")
    ap.add_argument("--runs", type=int, default=7, help="timed runs per measurement (median; at least 5)")
    ap.add_argument("--format", choices=["cf32", "sc16", "sc8", "cu8"], action="append", help="input format (default: all four)")
    ap.add_argument("--block", type=int, default=4096)
    ap.add_argument("--window", type=int, default=16)
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: at least 5")
    for items in a.items or [1 << 22, 1 << 26]:
        for fmt in a.format or ["cf32", "sc16", "sc8", "cu8"]:
            print(json.dumps(measure(items, a.runs, fmt, a.block, a.window)), flush=True)


if __name__ == "__main__":
    main()
