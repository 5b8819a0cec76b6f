"""Spectral scan of a SigMF capture: per band the mean and the maximum over the scan's rows, in dBFS.

    python tools/spectrum_scan.py CAPTURE [--nfft 1024] [--hop N] [--n-avg 16] [--window hann|rect]
                                  [--band=LO:HI ...] [--grid=OFFSET:N_GRID:BANDWIDTH --channels=K0:K1] [--chunk ITEMS] [--model] [--json]

CAPTURE is the path of a .sigmf-meta / .sigmf-data pair, with or without the extension (cf32_le, ci16_le, ci8 or cu8; integer
items go to the device as they are).  Bands are given in Hz from the capture's centre, either one by one (--band=-462500:-337500;
the = keeps a leading minus sign from reading as an option) or as a gateway's grid: --grid=0:10:125000 --channels=-4:4 makes one band per channel OFFSET + k * samp_rate / N_GRID, BANDWIDTH
wide, for k = K0 .. K1.  Without bands the whole capture is one band.  The rows come from lora.spectrum_scanner (the device,
fed --chunk items at a time), or with --model from the float64 definition gr_lora_amd.spectrum.welch_rows, which needs no GPU.
0 dBFS is a unit-amplitude complex tone.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _base(path):
    for ext in (".sigmf-meta", ".sigmf-data"):
        if path.endswith(ext):
            return path[: -len(ext)]
    return path


def _bands(a, fs):
    out = []
    for b in a.band or []:
        lo, hi = b.split(":")
        out.append((float(lo), float(hi)))
    if a.grid:
        off, n_grid, bw = a.grid.split(":")
        if not a.channels:
            raise SystemExit("--grid needs --channels K0:K1")
        k0, k1 = (int(v) for v in a.channels.split(":"))
        for k in range(k0, k1 + 1):
            f = float(off) + k * fs / int(n_grid)
            out.append((f - float(bw) / 2.0, f + float(bw) / 2.0))
    return out or [(-fs / 2.0, fs / 2.0)]


def scan(a):
    from gr_lora_amd import iqformat, sigmf, spectrum
    base = _base(a.capture)
    meta = sigmf.read_meta(base + ".sigmf-meta")
    datatype = sigmf.read_datatype(base + ".sigmf-meta")
    fs = float(meta["sample_rate"])
    data = sigmf.read_data(base + ".sigmf-data", datatype)
    hop = a.hop or a.nfft // 2
    bands = _bands(a, fs)
    bins = [spectrum.band_bins(fs, a.nfft, lo, hi) for lo, hi in bands]
    if a.model:
        x = data if data.dtype == np.complex64 else iqformat.to_cf32(data)
        _, _, band, first = spectrum.welch_rows(x, a.nfft, hop, a.n_avg, a.window, bins)
    else:
        from gr_lora_amd import lora
        sc = lora.spectrum_scanner(fs, a.nfft, hop, a.n_avg, a.window, False, bands)
        step = a.chunk if data.dtype == np.complex64 else 2 * a.chunk
        parts = [sc.work(data[i:i + step]) for i in range(0, data.size, step)]
        sc.close()
        band = np.concatenate([p.band for p in parts]).astype(np.float64)
        first = np.concatenate([p.first_sample for p in parts])
    rows = int(band.shape[0])
    out = dict(capture=os.path.basename(base), datatype=datatype, samp_rate=fs, nfft=a.nfft, hop=hop, n_avg=a.n_avg, window=a.window,
               source="model" if a.model else "device", rows=rows, row_samples=(a.n_avg - 1) * hop + a.nfft, bands=[])
    for b, (lo, hi) in enumerate(bands):
        mean = float(spectrum.to_dbfs(band[:, b].mean())) if rows else None
        peak = float(spectrum.to_dbfs(band[:, b].max())) if rows else None
        out["bands"].append(dict(f_lo=lo, f_hi=hi, first_bin=bins[b][0], n_bins=bins[b][1], mean_dbfs=mean, max_dbfs=peak,
                                 max_row_sample=int(first[int(band[:, b].argmax())]) if rows else None))
    return out


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("capture")
    ap.add_argument("--nfft", type=int, default=1024)
    ap.add_argument("--hop", type=int, default=0, help="default nfft / 2")
    ap.add_argument("--n-avg", type=int, default=16, dest="n_avg")
    ap.add_argument("--window", default="hann", choices=["hann", "rect"])
    ap.add_argument("--band", action="append", help="LO:HI in Hz from the capture's centre (repeatable)")
    ap.add_argument("--grid", help="OFFSET:N_GRID:BANDWIDTH (Hz, count, Hz)")
    ap.add_argument("--channels", help="K0:K1, grid indices (inclusive)")
    ap.add_argument("--chunk", type=int, default=1 << 22, help="items per device call (default 2^22)")
    ap.add_argument("--model", action="store_true", help="the float64 definition instead of the device")
    ap.add_argument("--json", action="store_true", help="one JSON line instead of the table")
    return ap


def main(argv=None):
    a = parser().parse_args(argv)
    out = scan(a)
    if a.json:
        print(json.dumps(out))
        return 0
    print("%s: %s, %g sps, nfft %d hop %d n_avg %d %s, %d rows of %d samples (%s)" % (out["capture"], out["datatype"], out["samp_rate"], out["nfft"],
                                                                                     out["hop"], out["n_avg"], out["window"], out["rows"],
                                                                                     out["row_samples"], out["source"]))
    print("%14s %14s %6s %10s %10s" % ("f_lo (Hz)", "f_hi (Hz)", "bins", "mean dBFS", "max dBFS"))
    for b in out["bands"]:
        if b["mean_dbfs"] is None:
            print("%14.1f %14.1f %6d %10s %10s" % (b["f_lo"], b["f_hi"], b["n_bins"], "-", "-"))
        else:
            print("%14.1f %14.1f %6d %10.2f %10.2f" % (b["f_lo"], b["f_hi"], b["n_bins"], b["mean_dbfs"], b["max_dbfs"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
