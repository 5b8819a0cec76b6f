#!/usr/bin/env python3
"""GNU-Radio-free equivalent of the reference's apps/lora_receive_file_nogui.py:
SigMF trace -> lora_receiver (channeliser + MI355X decoder) -> message_socket_sink (UDP).
The capture is fed in its own datatype: cf32_le as complex64, ci16_le / ci8 / cu8 as the integers in the file, which the
channeliser converts on the device (gr_lora_amd/iqformat.py).  --resample-to HZ puts a rational_resampler in front of the receiver for
a capture whose rate is no multiple of the bandwidth (2.4 Msps from an RTL-SDR: --resample-to 1000000).  --condition puts an
iq_conditioner first of all: it removes the DC offset and the I/Q imbalance of a direct-conversion front end."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gr_lora_amd import lora, sigmf  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description="Decode a SigMF LoRa capture on the MI355X")
    ap.add_argument("file", nargs="?", default="example-trace", help="base name of .sigmf-data / .sigmf-meta")
    ap.add_argument("--ip", default="127.0.0.1")
    ap.add_argument("--port", type=int, default=40868)
    ap.add_argument("--chunk", type=int, default=1 << 16, help="items per work() call")
    ap.add_argument("--resample-to", type=float, default=None, metavar="HZ",
                    help="resample the capture to this rate on the device before the receiver (HZ / sample_rate must be L / M with L, M <= 512)")
    ap.add_argument("--condition", action="store_true",
                    help="remove the capture's DC offset and correct its I/Q imbalance on the device first (before --resample-to)")
    args = ap.parse_args(argv)
    meta = sigmf.read_meta(args.file + ".sigmf-meta")
    cfg = sigmf.LoRaConfig(meta["transmit_freq"], meta["sf"], meta["cr"], meta["bw"], meta["prlen"], meta["crc"], meta["implicit"])
    print("[+] Configuration: %s" % cfg.string_repr())
    print("[+] Decoding. You should see a header, followed by '%s'%s %d times." % (
        meta["expected"], " and a CRC" if meta["crc"] else "", meta["times"]))
    resampler = lora.rational_resampler(meta["sample_rate"], args.resample_to) if args.resample_to else None
    conditioner = lora.iq_conditioner() if args.condition else None
    rx = lora.lora_receiver(args.resample_to if resampler else meta["sample_rate"], meta["capture_freq"], [meta["transmit_freq"]], cfg.bw, cfg.sf,
                            cfg.implicit, cfg.cr_num, cfg.crc)
    sink = lora.message_socket_sink(args.ip, args.port, 0)
    lora.msg_connect(rx, "frames", sink, "in")
    datatype = sigmf.read_datatype(args.file + ".sigmf-meta")
    iq = sigmf.read_data(args.file + ".sigmf-data", datatype)
    step = args.chunk * (1 if datatype == "cf32_le" else 2)   # (integer captures: two components per item)
    def feed(items):
        if items.size:
            rx.work(resampler.work(items) if resampler else items)

    for i in range(0, iq.size, step):
        feed(conditioner.work(iq[i:i + step]) if conditioner else iq[i:i + step])
    if conditioner:
        feed(conditioner.flush())
        conditioner.close()
    rx.stop()
    if resampler:
        resampler.close()
    rx.decoder.close()
    if rx.channelizer is not None:
        rx.channelizer._h.close()
    sink.close()
    print("[+] Done")


if __name__ == "__main__":
    main()
