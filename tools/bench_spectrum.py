"""Spectral scan (lora_hip_spectrum_*) on device-resident captures: one JSON line per case and input format.

    python tools/bench_spectrum.py [--case a|b|c] [--items N] [--runs R] [--format cf32|sc16|sc8|cu8] [--bands N]

Cases:
    a  nfft 1024, hop 512,  n_avg 16     (the gateway's default scan)
    b  nfft 256,  hop 256,  n_avg 64     (no overlap, long averages)
    c  nfft 4096, hop 2048, n_avg 8      (the finest resolution)
Each runs on cf32 and on sc16 unless --format names one.  Time = kernel time by HIP events (lora_hip_spectrum_last_kernel_ms: the
scan and the band sums), median of --runs runs after one warm-up run; the timed runs continue one stream, so every run computes
the same amount.  Bytes moved = the input items once (8 / 4 / 2 B each) + the rows written (4 B per bin, per band); fractions
against 8 TB/s (spec) and 6.29 TB/s (measured float4 copy).  With hop < nfft the overlap is read once per workgroup and re-read
by the next row's workgroup only: the bytes counted are what the algorithm needs, not what the kernel requests.
The fractions are those algorithmic bytes over the time, not measured HBM traffic: the same buffer is read again in every run, and
at the default 2^25 items the sc16 input (128 MiB; sc8 / cu8: 64 MiB) fits in the 256 MB Infinity Cache, so its runs after the
first need not reach HBM at all (cf32, 256 MiB, does not fit).  A timed window is 0.25 - 0.55 ms at the default size: short, so
read the per-run times in spectrum_runs_ms beside the median, or raise --items.
The rate to hold beside these lines is the filter bank's on the same kind of input (tools/bench_filterbank.py).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {
    "a": dict(nfft=1024, hop=512, n_avg=16),
    "b": dict(nfft=256, hop=256, n_avg=64),
    "c": dict(nfft=4096, hop=2048, n_avg=8),
}
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


def _time(run, kernel_ms, runs):
    run()                                      # warm-up (code object load, first touch)
    ms = []
    for _ in range(runs):
        run()
        ms.append(kernel_ms())
    return float(np.median(ms)), [round(m, 4) for m in ms]


def measure(key, items, runs, fmt_name, n_bands):
    import torch
    from gr_lora_amd import capi, iqformat
    fmt = iqformat.format_from_name(fmt_name)
    c = CASES[key]
    nfft, hop, n_avg = c["nfft"], c["hop"], c["n_avg"]
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(items) + 1j * rng.standard_normal(items)).astype(np.complex64)
    if fmt == iqformat.CF32:
        d_in = torch.from_numpy(x.view(np.float32)).to("cuda:0")
    else:
        info = np.iinfo(iqformat.DTYPES[fmt])
        d_in = torch.from_numpy(iqformat.quantize(x, fmt, 0.9 * info.max / float(np.abs(x.view(np.float32)).max()))).to("cuda:0")
    bands = [(b * (nfft // n_bands), nfft // n_bands) for b in range(n_bands)]
    sp = capi.Spectrum(16e6, nfft, hop, n_avg, bands=bands)
    max_rows = items // (n_avg * hop) + 2
    d_psd = torch.empty((max_rows, nfft), dtype=torch.float32, device="cuda:0")
    d_band = torch.empty((max_rows, max(n_bands, 1)), dtype=torch.float32, device="cuda:0")
    band_ptr = d_band.data_ptr() if n_bands else None
    rows = []

    def run():
        if fmt == iqformat.CF32:
            rows.append(sp.run_device(d_in.data_ptr(), items, d_psd.data_ptr(), None, band_ptr, nfft, max_rows)[0])
        else:
            rows.append(sp.run_device_raw(d_in.data_ptr(), items, fmt, d_psd.data_ptr(), None, band_ptr, nfft, max_rows)[0])

    ms, all_ms = _time(run, sp.kernel_ms, runs)
    n_rows = int(np.median(rows[1:]))
    nbytes = float(iqformat.ITEM_BYTES[fmt]) * items + 4.0 * n_rows * (nfft + n_bands)
    line = dict(case=key, format=fmt_name, nfft=nfft, hop=hop, n_avg=n_avg, bands=n_bands, items=items, rows=n_rows, spectrum_ms=round(ms, 4),
                spectrum_runs_ms=all_ms, gsamples_per_s=round(items / ms / 1e6, 3), gb_per_s=round(nbytes / ms / 1e6, 1),
                frac_hbm_spec=round(nbytes / ms * 1e3 / HBM_SPEC, 4), frac_hbm_copy=round(nbytes / ms * 1e3 / HBM_COPY, 4))
    sp.close()
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--case", choices=sorted(CASES), action="append")
    ap.add_argument("--items", type=int, default=1 << 25, help="input items per run (default 2^25)")
    ap.add_argument("--runs", type=int, default=7, help="timed runs per measurement (median; at least 5)")
    ap.add_argument("--format", choices=["cf32", "sc16", "sc8", "cu8"], action="append", help="input format (default: cf32 and sc16)")
    ap.add_argument("--bands", type=int, default=8, help="equal bands over the spectrum (0: none; default 8)")
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs: at least 5")
    for key in a.case or sorted(CASES):
        for fmt in a.format or ["cf32", "sc16"]:
            print(json.dumps(measure(key, a.items, a.runs, fmt, a.bands)), flush=True)


if __name__ == "__main__":
    main()
