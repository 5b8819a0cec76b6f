"""The multi-SF gateway (lora.multi_sf_gateway_receiver, include/lora_hip_gateway.h) end to end on the two gateway workloads of
tools/bench_filterbank.py with mixed-SF traffic, against six single-SF gateway_receivers on the same capture: one JSON line per
workload.

    python tools/bench_gateway.py [--workload a|b] [--runs R] [--out profiles/gateway_bench_lines.jsonl] [--no-baseline]
    python tools/bench_gateway.py --link [--workload a|b] [--runs R]      # link metrics off against on

Workloads (one wide-band capture -> every grid channel at 1 Msps -> SF7..SF12 decoders on every channel):
    a  EU868-like:  fs 2 Msps,  M 10, D 2,  8 channels, 2-3 frames per channel at different SFs
    b  US915-like:  fs 16 Msps, M 80, D 16, 64 channels, 1-2 frames per channel (SF11/12 on a few channels, SF7-10 elsewhere)
The capture is synthesised once (LORA_BENCH_CACHE=<dir> keeps it between runs, as bench.py) and stays resident in HBM.
Gateway time: work_device over the whole capture (chunks of 2^22 items) + flush + drain, wall clock, median of --runs fresh
receivers after one warm-up.  Baseline: six gateway_receiver(sf=s), host capture in chunks of 2^22 items, each with its own
filter bank and host round trip of every row, run one after the other (the only way before), median of --runs.
Filter-bank kernel ms: run_device_rows over 2^24 items with n_dst = 6 against n_dst = 1 (HIP events, median of 7).
Frames: each transmitted payload counted once when found on its own (grid index, SF).

    python tools/bench_gateway.py --format sc16|sc8|cu8 [--workload a|b] [--runs R] [--out FILE]

--format: the ingress comparison instead (one line per workload, "bench": "gateway_host_ingest").  The capture is quantised the
way the radio would deliver it (every transmitter at 2000 LSB of sc16, 12 LSB of sc8 / cu8) and fed from HOST memory in chunks
of 2^22 items: as the integers (lora_hip_gateway_work_raw) against the same items converted to complex64 on the host beforehand
(lora_hip_gateway_work; the conversion itself is not timed).  Wall clock, median of --runs fresh receivers after one warm-up each.

    python tools/bench_gateway.py --device-synth [--seconds S] [--workload a|b] [--runs R] [--out FILE]

--device-synth: the capture never exists on the host (one line per workload, "bench": "gateway_device_synth").  The same plan
(without --seconds: frame for frame the default path's; with it: continued per channel until S seconds of air are full) goes
through lora.traffic_synthesizer, which writes chunks of 2^22 items into one HBM buffer that multi_sf_gateway_receiver.work reads.
Reported apart, wall clock with the device idle at each boundary: the time in generate (and its kernel time, HIP events) and
the time in work + stop; median of --runs after one warm-up.  The default path and its cached files are untouched by it.
"""
from __future__ import annotations

import argparse
import json
import os
import pickle
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SFS = (7, 8, 9, 10, 11, 12)
WORKLOADS = {
    "a": dict(name="eu868", fs=2e6, M=10, f0=100e3, ks=list(range(-4, 4)), D=2),
    "b": dict(name="us915", fs=16e6, M=80, f0=100e3, ks=list(range(-32, 32)), D=16),
}
CHUNK = 1 << 22


def _plan(key, n_ch, rng):
    if key == "a":
        return [[12, 7], [11, 8, 7], [10, 9, 7], [8, 12], [9, 11], [10, 7, 8], [9, 11], [8, 10, 7]]
    plan = []
    for i in range(n_ch):
        if i % 16 == 3:
            plan.append([12])
        elif i % 16 == 9:
            plan.append([11, int(rng.integers(7, 9))])
        else:
            plan.append([int(s) for s in rng.choice([7, 8, 9, 10], size=int(rng.integers(1, 3)), replace=False)])
    return plan


def synthesise(key):
    """(wide complex64, {(grid index, sf): [expected blob tails]})"""
    from gr_lora_amd import lora, synth
    w = WORKLOADS[key]
    fs, M, f0, ks = w["fs"], w["M"], w["f0"], w["ks"]
    rng = np.random.default_rng(4242)
    per, expect = [], {}
    for k, sfs in zip(ks, _plan(key, len(ks), rng)):
        pieces = [np.zeros(int(rng.integers(1000, 40000)), dtype=np.complex64)]
        for sf in sfs:
            pl = bytes(rng.integers(0, 256, int(rng.integers(4, 12)), dtype=np.uint8))
            cfg = synth.TxConfig(sf=sf, cr=4, samp_rate=fs, reduced_rate=lora.lorawan_reduced_rate(sf, 125000),
                                 hdr_nibbles=synth.valid_hdr_nibbles(len(pl), 4, True))
            crc = synth.valid_crc_bytes(pl)
            st = synth.build_stream([pl], cfg, gaps=[int(rng.integers(2 * cfg.sps, 4 * cfg.sps))], tail_symbols=2.0, crc_bytes=crc)
            pieces.append(st.iq)
            expect.setdefault((k, sf), []).append(synth.expected_frame_tail(pl, cfg, crc))
        per.append(np.concatenate(pieces))
    n = max(s.size for s in per) + 3 * (1 << 12) * int(fs / 125000)
    wide = np.zeros(n, dtype=np.complex128)
    for k, s in zip(ks, per):
        ph = (f0 + k * fs / M) / fs * np.arange(s.size, dtype=np.float64)
        wide[: s.size] += s * np.exp(2j * np.pi * (ph - np.floor(ph)))
    return wide.astype(np.complex64), expect


def layout(key, seconds=None):
    """The plan of synthesise(key) as frames for lora.traffic_synthesizer: ([(grid index, sf, start item, payload)], expect, items).
    Its random draws are synthesise's in synthesise's order, so without `seconds` the frames are the default capture's; with it
    each channel's list of SFs repeats until the next frame would not fit into `seconds` of air."""
    from gr_lora_amd import lora, synth
    w = WORKLOADS[key]
    fs, ks = w["fs"], w["ks"]
    D = int(fs / 125000)
    tail = 3 * (1 << 12) * D
    limit = None if seconds is None else int(seconds * fs) - tail
    rng = np.random.default_rng(4242)
    frames, expect, ends = [], {}, []

    def place(k, sf, pos):
        pl = bytes(rng.integers(0, 256, int(rng.integers(4, 12)), dtype=np.uint8))
        rr = lora.lorawan_reduced_rate(sf, 125000)
        sps = D << sf
        gap = int(rng.integers(2 * sps, 4 * sps))
        items = (8 + 4 + 8 + synth.payload_symbol_count(len(pl) + 2, sf, 4, rr)) * sps + sps // 4
        end = pos + gap + items + 2 * sps
        if limit is not None and end > limit:
            return None
        cfg = synth.TxConfig(sf=sf, cr=4, samp_rate=fs, reduced_rate=rr, hdr_nibbles=synth.valid_hdr_nibbles(len(pl), 4, True))
        frames.append((k, sf, pos + gap, pl))
        expect.setdefault((k, sf), []).append(synth.expected_frame_tail(pl, cfg, synth.valid_crc_bytes(pl)))
        return end

    plan = _plan(key, len(ks), rng)
    for k, sfs in zip(ks, plan):
        pos = int(rng.integers(1000, 40000))
        for sf in sfs:
            pos = place(k, sf, pos) or pos
        ends.append(pos)
    if limit is not None:
        for i, (k, sfs) in enumerate(zip(ks, plan)):
            j = 0
            while True:
                end = place(k, sfs[j % len(sfs)], ends[i])
                if end is None:
                    break
                ends[i], j = end, j + 1
    return frames, expect, (max(ends) + tail if seconds is None else int(seconds * fs))


def run_device_synth(w, frames, n):
    """One pass: (seconds in generate, its kernel ms, seconds in work + stop, frames, stats)."""
    import torch
    from gr_lora_amd import lora
    tx = lora.traffic_synthesizer(w["fs"])
    for k, sf, start, pl in frames:
        tx.add_frame(pl, sf, 4, 125000, start, w["f0"] + k * w["fs"] / w["M"])
    rx = lora.multi_sf_gateway_receiver(w["fs"], 0.0, w["f0"], w["M"], w["ks"], 125000, sfs=SFS, decimation=w["D"])
    got = []
    rx.subscribe("sf_frames", got.append)
    buf = torch.empty(min(CHUNK, n), dtype=torch.complex64, device="cuda:0")
    torch.cuda.synchronize()
    t_syn = t_gw = ms = 0.0
    for i in range(0, n, CHUNK):
        m = min(CHUNK, n - i)
        t0 = time.perf_counter()
        tx.generate(m, out=buf[:m])                        # (returns when the items are written)
        t1 = time.perf_counter()
        rx.work(buf[:m])
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        t_syn, t_gw, ms = t_syn + (t1 - t0), t_gw + (t2 - t1), ms + tx.kernel_ms()
    t0 = time.perf_counter()
    rx.stop()
    t_gw += time.perf_counter() - t0
    stats = rx.stats()
    assert tx.pending == 0, tx.pending
    rx.close()
    tx.close()
    return t_syn, ms, t_gw, got, stats


def measure_device_synth(key, runs, seconds):
    w = WORKLOADS[key]
    t0 = time.perf_counter()
    frames, expect, n = layout(key, seconds)
    t_layout = time.perf_counter() - t0
    run_device_synth(w, frames, n)                         # warm-up
    res = [run_device_synth(w, frames, n) for _ in range(runs)]
    syn, ms, gw = (float(np.median([r[j] for r in res])) for j in range(3))
    got = res[0][3]
    return dict(bench="gateway_device_synth", workload=key, name=w["name"], samp_rate=w["fs"], channels=len(w["ks"]), items=n, air_s=round(n / w["fs"], 4),
                chunk_items=CHUNK, transmitted=len(frames), frames_published=len(got), payloads_found=matched(got, expect),
                layout_host_s=round(t_layout, 4), synth_s=round(syn, 4), synth_kernel_ms=round(ms, 3), gateway_s=round(gw, 4),
                synth_runs_s=[round(r[0], 4) for r in res], gateway_runs_s=[round(r[2], 4) for r in res],
                synth_items_per_s=round(n / syn, 1), synth_kernel_items_per_s=round(n / (ms * 1e-3), 1), gateway_items_per_s=round(n / gw, 1),
                synth_over_gateway=round(syn / gw, 4), filterbank_calls=res[0][4]["filterbank_calls"])


def cached(key):
    d = os.environ.get("LORA_BENCH_CACHE")
    if not d:
        return synthesise(key)
    f_iq, f_meta = os.path.join(d, "gateway_%s.npy" % key), os.path.join(d, "gateway_%s.pkl" % key)
    if os.path.exists(f_iq) and os.path.exists(f_meta):
        with open(f_meta, "rb") as f:
            return np.load(f_iq), pickle.load(f)
    wide, expect = synthesise(key)
    os.makedirs(d, exist_ok=True)
    np.save(f_iq, wide)
    with open(f_meta, "wb") as f:
        pickle.dump(expect, f)
    return wide, expect


def run_gateway(w, d_wide, n, link=False):
    import torch
    from gr_lora_amd import lora
    rx = lora.multi_sf_gateway_receiver(w["fs"], 0.0, w["f0"], w["M"], w["ks"], 125000, sfs=SFS, decimation=w["D"], link_metrics=link)
    frames = []
    rx.subscribe("sf_frames", frames.append)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(0, n, CHUNK):
        rx.work(d_wide[i:i + CHUNK])
    rx.stop()
    dt = time.perf_counter() - t0
    stats = rx.stats()
    rx.close()
    return dt, frames, stats


def run_gateway_host(w, arr, width):
    """arr: the host capture (complex64: width 1; flat integer components: width 2), fed in chunks of CHUNK items."""
    from gr_lora_amd import lora
    rx = lora.multi_sf_gateway_receiver(w["fs"], 0.0, w["f0"], w["M"], w["ks"], 125000, sfs=SFS, decimation=w["D"])
    frames = []
    rx.subscribe("sf_frames", frames.append)
    t0 = time.perf_counter()
    for i in range(0, arr.size, CHUNK * width):
        rx.work(arr[i:i + CHUNK * width])
    rx.stop()
    dt = time.perf_counter() - t0
    rx.close()
    return dt, frames


def measure_host_ingest(key, runs, fmt_name):
    from gr_lora_amd import iqformat
    w = WORKLOADS[key]
    wide, expect = cached(key)
    fmt = iqformat.format_from_name(fmt_name)
    raw = iqformat.quantize(wide, fmt, 2000.0 if fmt == iqformat.SC16 else 12.0)
    conv = iqformat.to_cf32(raw, fmt)
    n = wide.size
    out = dict(bench="gateway_host_ingest", workload=key, name=w["name"], format=fmt_name, items=n, chunk_items=CHUNK,
               transmitted=sum(len(t) for t in expect.values()), bytes_cf32=8 * n, bytes_raw=iqformat.ITEM_BYTES[fmt] * n)
    for tag, arr, width in (("cf32", conv, 1), (fmt_name, raw, 2)):
        run_gateway_host(w, arr, width)                    # warm-up
        res = [run_gateway_host(w, arr, width) for _ in range(runs)]
        dts = [r[0] for r in res]
        dt = float(np.median(dts))
        out.update({tag + "_s": round(dt, 4), tag + "_runs_s": [round(x, 4) for x in dts], tag + "_items_per_s": round(n / dt, 1),
                    tag + "_payloads_found": matched(res[0][1], expect), tag + "_frames": [(int(k), int(sf), b.hex()) for k, sf, b in res[0][1]]})
    out["frames_equal"] = out.pop("cf32_frames") == out.pop(fmt_name + "_frames")
    out["speedup"] = round(out["cf32_s"] / out[fmt_name + "_s"], 3)
    return out


def run_baseline(w, wide):
    from gr_lora_amd import lora
    frames = []
    t0 = time.perf_counter()
    for sf in SFS:
        gw = lora.gateway_receiver(w["fs"], 0.0, w["f0"], w["M"], w["ks"], 125000, sf, False, 4, True, decimation=w["D"],
                                   reduced_rate=lora.lorawan_reduced_rate(sf, 125000))
        gw.subscribe("channel_frames", lambda kb, sf=sf: frames.append((kb[0], sf, kb[1])))
        for i in range(0, wide.size, CHUNK):
            gw.work(wide[i:i + CHUNK])
        gw.stop()
        gw.close()
    return time.perf_counter() - t0, frames


def matched(frames, expect):
    got = {}
    for k, sf, blob in frames:
        got.setdefault((int(k), int(sf)), []).append(blob[15:])
    return sum(sum(1 for t in tails if t in got.get(kk, [])) for kk, tails in expect.items())


def fb_kernel_ms(w, d_wide, items, n_dst):
    import torch
    from gr_lora_amd import capi
    fb = capi.FilterBank(w["fs"], w["f0"], w["M"], w["ks"], 125000, w["D"])
    no = fb.output_items(items)
    nch = len(w["ks"])
    bufs = [torch.empty((nch, 2 * no), dtype=torch.float32, device="cuda") for _ in range(n_dst)]
    ptrs = [bufs[d][c].data_ptr() for d in range(n_dst) for c in range(nch)]
    src = d_wide.data_ptr()
    ms = []
    for r in range(8):                                 # one stream: every run the same amount (first run: warm-up)
        fb.run_device_rows(src, items, ptrs, n_dst, no)
        if r:
            ms.append(fb.kernel_ms())
    fb.close()
    return float(np.median(ms))


def measure(key, runs, baseline):
    import torch
    w = WORKLOADS[key]
    wide, expect = cached(key)
    n = wide.size
    d_wide = torch.from_numpy(wide).to("cuda:0")
    n_tx = sum(len(t) for t in expect.values())
    run_gateway(w, d_wide, n)                          # warm-up
    res = [run_gateway(w, d_wide, n) for _ in range(runs)]
    dts = [r[0] for r in res]
    dt = float(np.median(dts))
    _, frames, stats = res[0]
    air_s = n / w["fs"]
    fb_items = min(1 << 24, n)
    line = dict(workload=key, name=w["name"], samp_rate=w["fs"], n_grid=w["M"], channels=len(w["ks"]), decimation=w["D"], sfs=list(SFS),
                items=n, air_s=round(air_s, 4), transmitted=n_tx, frames_published=len(frames), payloads_found=matched(frames, expect),
                gateway_s=round(dt, 4), gateway_runs_s=[round(x, 4) for x in dts], items_per_s=round(n / dt, 1),
                realtime_factor=round(air_s / dt, 2), passes_per_sf={str(k): v for k, v in stats["passes"].items()},
                filterbank_calls=stats["filterbank_calls"], filterbank_ms_total=round(stats["filterbank_ms"], 3),
                fb_kernel_items=fb_items, fb_kernel_ms_ndst6=round(fb_kernel_ms(w, d_wide, fb_items, 6), 4),
                fb_kernel_ms_ndst1=round(fb_kernel_ms(w, d_wide, fb_items, 1), 4))
    line["fb_ndst6_over_ndst1"] = round(line["fb_kernel_ms_ndst6"] / line["fb_kernel_ms_ndst1"], 3)
    if baseline:
        run_baseline(w, wide)                          # warm-up
        bres = [run_baseline(w, wide) for _ in range(runs)]
        bdts = [r[0] for r in bres]
        bdt = float(np.median(bdts))
        line.update(baseline_s=round(bdt, 4), baseline_runs_s=[round(x, 4) for x in bdts], baseline_items_per_s=round(n / bdt, 1),
                    baseline_realtime_factor=round(air_s / bdt, 2), baseline_payloads_found=matched(bres[0][1], expect),
                    speedup=round(bdt / dt, 2))
    return line


def measure_link(key, runs):
    """The gateway with link metrics (include/lora_hip_link.h) off and on, runs interleaved in one process."""
    import torch
    w = WORKLOADS[key]
    wide, expect = cached(key)
    n = wide.size
    d_wide = torch.from_numpy(wide).to("cuda:0")
    for link in (False, True):
        run_gateway(w, d_wide, n, link)                # warm-up
    dts = {False: [], True: []}
    frames = {}
    for _ in range(runs):
        for link in (False, True):
            dt, fr, _ = run_gateway(w, d_wide, n, link)
            dts[link].append(dt)
            frames[link] = fr
    off, on = float(np.median(dts[False])), float(np.median(dts[True]))
    return dict(bench="gateway_link", workload=key, name=w["name"], items=n, frames_published=len(frames[True]),
                frames_equal=[(int(k), int(sf), b) for k, sf, b in frames[False]] == [(int(k), int(sf), b) for k, sf, b in frames[True]],
                link_off_s=round(off, 4), link_off_runs_s=[round(x, 4) for x in dts[False]], link_off_items_per_s=round(n / off, 1),
                link_on_s=round(on, 4), link_on_runs_s=[round(x, 4) for x in dts[True]], link_on_items_per_s=round(n / on, 1),
                link_on_over_off=round(on / off, 4))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workload", choices=sorted(WORKLOADS), action="append")
    ap.add_argument("--runs", type=int, default=5, help="timed runs (median)")
    ap.add_argument("--out", help="also append the lines to this file")
    ap.add_argument("--no-baseline", action="store_true", help="the gateway only (profiler runs)")
    ap.add_argument("--format", choices=["sc16", "sc8", "cu8"], help="the host-ingest comparison: integers against complex64, both from host memory")
    ap.add_argument("--device-synth", action="store_true", help="synthesise the capture on the device (lora.traffic_synthesizer) and feed work_device from HBM")
    ap.add_argument("--seconds", type=float, help="with --device-synth: seconds of air (default: the default path's plan, frame for frame)")
    ap.add_argument("--link", action="store_true", help="throughput with link metrics off and on (interleaved runs)")
    a = ap.parse_args()
    if a.seconds is not None and not a.device_synth:
        ap.error("--seconds goes with --device-synth")
    for key in a.workload or sorted(WORKLOADS):
        if a.link:
            line = json.dumps(measure_link(key, a.runs))
        elif a.device_synth:
            line = json.dumps(measure_device_synth(key, a.runs, a.seconds))
        else:
            line = json.dumps(measure_host_ingest(key, a.runs, a.format) if a.format else measure(key, a.runs, not a.no_baseline))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
