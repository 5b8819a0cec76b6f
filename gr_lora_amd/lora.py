"""GNU-Radio-free mirror of the reference's block API for the decoder path.

Same names, argument order and meaning as the reference module `lora`:
  lora.decoder(samp_rate, bandwidth, sf, implicit, cr, crc, reduced_rate, disable_drift_correction)
      (python/bindings/decoder_python.cc:36-66, include/lora/decoder.h:705)
  lora.lora_receiver(samp_rate, center_freq, channel_list, bandwidth, sf, implicit, cr, crc,
                     reduced_rate=False, conj=False, decimation=1, disable_channelization=False,
                     disable_drift_correction=False)            (python/lora_receiver.py:30)
  lora.gateway_receiver(samp_rate, center_freq, grid_offset, n_grid, channels, bandwidth, sf, implicit, cr, crc,
                        decimation)                  (not upstream: every channel of a uniform grid, one filter bank + one mux)
  lora.multi_sf_gateway_receiver(samp_rate, center_freq, grid_offset, n_grid, channels, bandwidth, sfs, ...)
                                              (not upstream: every channel x every SF, one filter bank feeding one mux per SF
                                              on the device)
  lora.modulator(samp_rate, bandwidth, sf, implicit, cr, crc, reduced_rate)
                                              (not upstream, which only receives: the decoder's mirror, one frame per call)
  lora.traffic_synthesizer(samp_rate, ...)    (not upstream: a wide-band capture of many concurrent emitters, made on the device)
  lora.spectrum_scanner(samp_rate, nfft, hop, n_avg, window, peak, bands)
                                              (not upstream: Welch power-spectrum rows and per-channel band powers of the capture,
                                              on the device, beside the receivers and fed the same array)
  lora.rational_resampler(in_rate, out_rate, zero_crossings, beta, cutoff)
                                              (not upstream, which leaves it to a GNU Radio block: rate in_rate -> in_rate * L / M on
                                              the device, in front of any receiver, for captures at 2.4, 2.048, 1.92 ... Msps)
  lora.iq_conditioner(block, window, dc, iq)  (not upstream: removes a direct-conversion front end's DC offset and IQ imbalance on the
                                              device, estimated from block moments; the first stage, in front of the resampler)
  lora.weak_signal_receiver(samp_rate, bandwidth, sf, cr, crc, reduced_rate, threshold, require_header_checksum, soft, crc_repair=0)
                                              (not upstream: the low-SNR receive path on one whole capture - the FFT-domain preamble
                                              detector, then the soft-decision decoder at its header positions; batch, not streaming.
                                              crc_repair = 1 .. 8: a frame whose payload CRC fails is repaired on the device by giving
                                              up to that many of its least reliable codewords their runner-up nibble; off by default)
  lora.message_socket_sink(ip, port, layer)   (lib/message_socket_sink_impl.cc:93-122)
  lora.message_file_sink(path)                (lib/message_file_sink_impl.cc)
Blocks exchange frames through message ports named as upstream ("frames",
"control"); `msg_connect(src, "frames", dst, "in")` wires them.  Samples are
pushed with `work(items)` the way the GNU Radio scheduler calls
decoder_impl::work (any chunking), and `stop()` plays the end of the flowgraph.

The decoder runs on the MI355X through the C ABI (include/lora_hip.h); there is
no CPU path here.  The channeliser of lora_receiver is host code (the step before
the hot path).
"""
from __future__ import annotations

import socket
import sys
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from . import capi, iqformat

LORATAP_LEN = 15   # sizeof(loratap_header_t), include/lora/loratap.h:35-55
LORAPHY_LEN = 3    # sizeof(loraphy_header_t), include/lora/loraphy.h:25-32
MAC_CRC_SIZE = 2   # include/lora/utilities.h:29


def _integer_iq(x, scale=0):
    """Integer IQ handed to a block's work(): a numpy array of dtype int16 (sc16), int8 (sc8) or uint8 (cu8), flat interleaved
    (I, Q, I, Q ...) or shaped (n, 2) -> (flat components, format, items); None for anything else (today's complex64 path).
    A wrong shape or an unusable scale is refused here (ValueError), before anything reaches the library."""
    if not (isinstance(x, np.ndarray) and x.dtype in (np.int16, np.int8, np.uint8)):
        if scale:
            raise TypeError("scale applies to integer IQ (an int16 / int8 / uint8 array), not to %s" % type(x).__name__)
        return None
    iqformat.check_scale(scale)
    return iqformat.as_components(x)


class _MsgBlock:
    """Minimal message-port plumbing (gr::basic_block::message_port_pub/register)."""

    def __init__(self):
        self._out: Dict[str, List[Callable[[bytes], None]]] = {}
        self._in: Dict[str, Callable[[bytes], None]] = {}

    def message_port_register_out(self, name: str):
        self._out.setdefault(name, [])

    def message_port_register_in(self, name: str, handler: Callable[[bytes], None]):
        self._in[name] = handler

    def message_port_pub(self, name: str, blob: bytes):
        for cb in self._out.get(name, []):
            cb(blob)

    def subscribe(self, name: str, cb: Callable[[bytes], None]):
        if name not in self._out:
            raise KeyError("no message port '%s'" % name)
        self._out[name].append(cb)


def msg_connect(src: _MsgBlock, src_port: str, dst, dst_port: str = "in"):
    """top_block.msg_connect((src, port), (dst, port))"""
    if callable(dst) and not isinstance(dst, _MsgBlock):
        src.subscribe(src_port, dst)
    else:
        src.subscribe(src_port, dst._in[dst_port])


def _hex_line(data: bytes, endline: bool, ascii_part: bool) -> str:
    """print_vector_hex (include/lora/utilities.h:351-368)"""
    s = "".join(" %02x" % b for b in data)
    if ascii_part:
        s += " (" + "".join(chr(b) for b in data if 0x20 <= b <= 0x7e) + ")"
    return s + ("\n" if endline else "")


def _link_message(blob, info, metrics, **where) -> dict:
    """What the "link" port carries for one frame: the metrics of include/lora_hip_link.h, the frame's blob and header position,
    and where it came from (the gateways: row, grid_index, sf, freq_hz)."""
    d = metrics.as_dict()
    d.update(blob=blob, header_pos=int(info.header_pos), end_pos=int(info.end_pos))
    d.update(where)
    return d


class decoder(_MsgBlock):
    """gr::lora::decoder on the MI355X.  demod: capi.DEMOD_FFT_COMPAT (default; dechirp x FFT x
    argmax, byte-identical to the upstream default path's bin convention), DEMOD_FFT, or
    DEMOD_GRAD (the upstream default estimator itself)."""

    def __init__(self, samp_rate, bandwidth, sf, implicit, cr, crc, reduced_rate=False,
                 disable_drift_correction=False, *, device=0, demod=capi.DEMOD_FFT_COMPAT, verbose=True,
                 batch_items=0, segment_symbols=0, cfo_estimates=False, link_metrics=False):
        super().__init__()
        self._link = bool(link_metrics)                # each "frames" message is followed by its metrics on "link" (include/lora_hip_link.h)
        self._where = dict(sf=int(sf), bandwidth=int(bandwidth), row_rate=float(samp_rate))
        self._cfo = bool(cfo_estimates)
        self._hist = None                              # cfo_estimates: ring buffer of the most recent input, for the preamble windows
        self._hist_end = 0                             # absolute item index one past the newest item in the ring
        self.cfo_dropped = 0                           # estimates not published because their window had left the ring
        if sf < 6 or sf > 12:  # decoder_impl.cc:57-61 -- the reference prints this and exit(1)s
            sys.stderr.write("[LoRa Decoder] ERROR : Spreading factor should be between 6 and 12 (inclusive)!\n"
                             "                       Other values are currently not supported.\n")
            raise SystemExit(1)
        self._verbose = verbose
        self._h = capi.Handle(samp_rate=samp_rate, bandwidth=bandwidth, sf=sf, implicit=implicit, cr=cr, crc=crc,
                              reduced_rate=reduced_rate, disable_drift_correction=disable_drift_correction,
                              device=device, demod=demod, batch_items=batch_items, segment_symbols=segment_symbols)
        self.samples_per_symbol = self._h.sps
        self.number_of_bins = self._h.nbins
        self.decim_factor = self._h.decim
        if verbose:  # decoder_impl.cc:93-103
            bits_per_symbol = float(sf) * (4.0 / (4.0 + cr))
            print("Bits (nominal) per symbol: \t%g" % bits_per_symbol)
            print("Bins per symbol: \t%d" % self.number_of_bins)
            print("Samples per symbol: \t%d" % self.samples_per_symbol)
            print("Decimation: \t\t%d" % self.decim_factor)
            if disable_drift_correction:
                print("Warning: clock drift correction disabled")
            if implicit:
                print("CR: \t\t%d" % cr)
                print("CRC: \t\t%d" % int(bool(crc)))
        if self._cfo:
            # A frame surfaces at most two device passes after its last sample (one being filled, one in flight) and its
            # preamble lies a whole packet further back: the ring holds 2 passes of the library's EFFECTIVE batch size
            # (lora_hip_stream_info; 2M items at SF12, not the constructor argument) + the longest packet + a margin.
            eff_batch = int(self._h.stream_info().batch_items)
            ppm = int(sf) - 2 if reduced_rate else int(sf)          # bits per payload symbol (decoder_impl.cc:842-847)
            longest = (14 + 8 + 8 * -(-(2 * 257 * 8) // (8 * ppm))) * self._h.sps   # preamble + header + ceil(257 B at CR 4/8 / block) blocks of 8
            self._hist = np.zeros(2 * eff_batch + longest + 8 * self._h.sps, dtype=np.complex64)
        self.message_port_register_out("frames")    # decoder_impl.cc:120
        self.message_port_register_out("control")   # :121 (registered, never published upstream)
        self.message_port_register_out("link")
        if self._link:
            self._h.enable_link(True)

    # scheduler-facing ------------------------------------------------------
    def output_multiple(self) -> int:
        return 2 * self.samples_per_symbol           # set_output_multiple (:91)

    def work(self, input_items, scale=0) -> int:
        """Consumes every item handed in (buffers internally); publishes finished frames.  Integer IQ (an int16 / int8 / uint8
        array, flat interleaved or (n, 2); scale: gr_lora_amd.iqformat) crosses the link as it is and is converted on the device."""
        raw = _integer_iq(input_items, scale)
        x = np.asarray(input_items) if raw is None else (iqformat.to_cf32(raw[0], raw[1], scale) if self._cfo else None)
        if self._cfo:   # preallocated ring: one copy of the new items, nothing re-copied
            xc = x.astype(np.complex64, copy=False).ravel()
            cap = self._hist.size
            if xc.size >= cap:
                xc = xc[-cap:]
                self._hist_end += int(x.size) - cap
            w = self._hist_end % cap
            first = min(xc.size, cap - w)
            self._hist[w:w + first] = xc[:first]
            self._hist[:xc.size - first] = xc[first:]
            self._hist_end += xc.size
        n = self._h.work(x) if raw is None else self._h.work_raw(raw[0], raw[1], scale)
        self._publish()
        return n

    def stop(self):
        """End of stream: decode what is buffered, like the scheduler draining its last buffers."""
        self._h.flush()
        self._publish()

    def _publish(self):
        for blob, _info, *met in (self._h.drain_link() if self._link else self._h.drain()):
            if self._verbose:  # :832 and :872
                sys.stdout.write(_hex_line(blob[LORATAP_LEN:LORATAP_LEN + LORAPHY_LEN], False, False))
                sys.stdout.write(_hex_line(blob[LORATAP_LEN + LORAPHY_LEN:], True, True))
            self.message_port_pub("frames", blob)
            if self._link:
                self.message_port_pub("link", _link_message(blob, _info, met[0], **self._where))
            if self._cfo:
                self._publish_cfo(_info)

    def _publish_cfo(self, info):
        """What decoder_impl.cc:774-776 (commented out upstream) would publish: ("cfo", Hz) on the "control" port, from
        experimental_determine_cfo (:730-738) over a preamble upchirp.  The window is the last unmodulated upchirp but one
        in front of the frame (header - 6.25 symbols: 2.25 SFD + 2 sync words + 2), on the symbol clock the SFD search
        settled; the estimate is the mean over the window (mode 1), not upstream's single sample."""
        import torch
        sps = self.samples_per_symbol
        cap = self._hist.size
        a0 = int(info.header_pos) - (25 * sps) // 4           # absolute item index of the window
        if a0 < max(self._hist_end - cap, 0) or a0 + sps > self._hist_end:
            self.cfo_dropped += 1                                # (counted, not silent: the ring was sized too small for this traffic)
            return
        idx = (a0 + np.arange(sps)) % cap
        d = torch.from_numpy(np.ascontiguousarray(self._hist[idx]).view(np.float32)).to("cuda:%d" % self._h.device)
        hz = float(self._h.estimate_cfo_device(d.data_ptr(), sps, [0], mode=1)[0])
        self.message_port_pub("control", ("cfo", hz, a0))      # (the window's position lets a consumer ignore stale estimates)

    # decoder.h:708-709 ------------------------------------------------------
    def set_sf(self, sf):
        self._h.L.lora_hip_set_sf(self._h.h, int(sf))

    def set_samp_rate(self, samp_rate):
        self._h.L.lora_hip_set_samp_rate(self._h.h, float(samp_rate))

    def close(self):
        self._h.close()


def low_pass_taps(gain, fs, cutoff, transition):
    """gr::filter::firdes::low_pass(gain, fs, cutoff, transition, WIN_HAMMING) as GNU Radio 3.9 computes it:
    ntaps = int(53 * fs / (22 * transition)) made odd, float Hamming window, float taps, normalised so that the DC
    gain (taps[M] + 2 * sum of one side) is `gain`.  Same steps as firdes_low_pass in csrc/lora_channelizer.hip."""
    ntaps = int(53.0 * fs / (22.0 * transition))
    if ntaps % 2 == 0:
        ntaps += 1
    m = (ntaps - 1) // 2
    fw = 2.0 * np.pi * cutoff / fs
    w = (0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(ntaps) / (ntaps - 1))).astype(np.float32)
    n = np.arange(-m, m + 1, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        taps = np.where(n == 0, fw / np.pi * w, np.sin(n * fw) / (n * np.pi) * w).astype(np.float32)
    fmax = float(taps[m]) + 2.0 * float(taps[m + 1:].astype(np.float64).sum())
    return (taps.astype(np.float64) * (gain / fmax)).astype(np.float32)


class channelizer:
    """gr::lora::channelizer: freq_xlating_fir_filter_ccf(decimation, low_pass(1, fs, bw/2 + 15 kHz,
    10 kHz, Hamming), channel_list[0] - center_freq, fs)  (lib/channelizer_impl.cc:46-57), on the GPU through
    lora_hip_channelizer_* (include/lora_hip_channelizer.h).  Like the reference only channel_list[0] is output.
    There is no host fall-back: without the HIP library and a device the constructor raises."""

    def __init__(self, samp_rate, center_freq, channel_list, bandwidth, decimation=1, device=0):
        from . import capi
        self.fs = float(samp_rate)
        self.center_freq = float(center_freq)
        self.channel_list = list(channel_list)
        self.bandwidth = int(bandwidth)
        self.decimation = int(decimation)
        self.device = device
        self._h = capi.Channelizer(samp_rate, center_freq, self.channel_list[:1], bandwidth, decimation, device)
        self.taps = self._h.taps()

    def work(self, x, scale=0) -> np.ndarray:
        """complex64[n_in], or integer IQ (int16 / int8 / uint8, flat interleaved or (n, 2)) converted by the kernel."""
        raw = _integer_iq(x, scale)
        if raw is not None:
            return self._h.work_raw(raw[0], raw[1], scale)[0] if raw[2] else np.zeros(0, dtype=np.complex64)
        x = np.asarray(x, dtype=np.complex64)
        if x.size == 0:
            return x
        return self._h.work(x)[0]

    def apply_cfo(self, cfo):                       # channelizer_impl.cc:68-71
        self._h.apply_cfo(cfo)

    def retune(self, center_freq):
        """A new capture centre frequency (filter history and oscillator phase start over)."""
        from . import capi
        self._h.close()
        self.center_freq = float(center_freq)
        self._h = capi.Channelizer(self.fs, self.center_freq, self.channel_list[:1], self.bandwidth, self.decimation, self.device)


class filterbank_channelizer:
    """Like `channelizer`, for channels on a uniform grid, and every selected row is output: row c is the channeliser's output
    at center_freq + grid_offset + channels[c] * samp_rate / n_grid, computed by the polyphase DFT filter bank
    (include/lora_hip_filterbank.h) in one launch for all of them.  No host fall-back."""

    def __init__(self, samp_rate, center_freq, grid_offset, n_grid, channels, bandwidth, decimation=1, device=0):
        self.fs = float(samp_rate)
        self.center_freq = float(center_freq)
        self.grid_offset = float(grid_offset)
        self.n_grid = int(n_grid)
        self.channels = [int(k) for k in channels]
        self.bandwidth = int(bandwidth)
        self.decimation = int(decimation)
        self.device = device
        self._h = capi.FilterBank(samp_rate, grid_offset, n_grid, self.channels, bandwidth, decimation, device)
        self.taps = self._h.taps()

    def channel_freq(self, kappa) -> float:
        """Absolute centre frequency (Hz) of grid index kappa."""
        return self.center_freq + self.grid_offset + int(kappa) * self.fs / self.n_grid

    def work(self, x, scale=0) -> np.ndarray:
        """complex64[n_in], or integer IQ (int16 / int8 / uint8, flat interleaved or (n, 2)) -> complex64[len(channels), n_out]."""
        raw = _integer_iq(x, scale)
        if raw is not None:
            return self._h.work_raw(raw[0], raw[1], scale)
        x = np.asarray(x, dtype=np.complex64)
        return self._h.work(x)

    def close(self):
        self._h.close()


class gateway_receiver(_MsgBlock):
    """A gateway's receiver: one wide-band capture -> filterbank_channelizer (every grid channel of the band plan in one launch)
    -> one capi.Mux with a decoder per channel.  Each frame is published unchanged on "frames" and as (grid_index, blob) on
    "channel_frames"; per channel the frames are what lora_receiver on that channel alone publishes from the same channel samples."""

    def __init__(self, samp_rate, center_freq, grid_offset, n_grid, channels, bandwidth, sf, implicit, cr, crc, decimation=1,
                 reduced_rate=False, disable_drift_correction=False, device=0, demod=capi.DEMOD_FFT_COMPAT, batch_items=0, latency_ms=None,
                 link_metrics=False):
        super().__init__()
        self._link = bool(link_metrics)
        self.samp_rate = samp_rate
        self.center_freq = center_freq
        self.channels = [int(k) for k in channels]
        self.sf = sf
        self.decimation = int(decimation)
        if sf < 6 or sf > 12:  # as decoder (decoder_impl.cc:57-61)
            sys.stderr.write("[LoRa Decoder] ERROR : Spreading factor should be between 6 and 12 (inclusive)!\n"
                             "                       Other values are currently not supported.\n")
            raise SystemExit(1)
        self.filterbank = filterbank_channelizer(samp_rate, center_freq, grid_offset, n_grid, self.channels, bandwidth, decimation, device)
        self.mux = capi.Mux(len(self.channels), samp_rate=samp_rate / self.decimation, bandwidth=bandwidth, sf=sf, implicit=implicit, cr=cr,
                            crc=crc, reduced_rate=reduced_rate, disable_drift_correction=disable_drift_correction, device=device, demod=demod,
                            batch_items=batch_items)
        if latency_ms is not None:
            self.mux.set_latency(float(latency_ms))
        self.message_port_register_out("frames")
        self.message_port_register_out("channel_frames")
        self.message_port_register_out("link")
        if self._link:
            self.mux.enable_link(True)

    def work(self, input_items, scale=0) -> int:
        raw = _integer_iq(input_items, scale)
        if raw is not None:
            rows, n = self.filterbank.work(raw[0], scale), raw[2]
        else:
            x = np.asarray(input_items, dtype=np.complex64)
            rows, n = self.filterbank.work(x), x.size
        for c in range(len(self.channels)):
            if rows.shape[1]:
                self.mux.work(c, rows[c])
        self._publish()
        return n

    def stop(self):
        self.mux.flush()
        self._publish()

    def _publish(self):
        for blob, info, *met in (self.mux.drain_link() if self._link else self.mux.drain()):
            self.message_port_pub("frames", blob)
            self.message_port_pub("channel_frames", (self.channels[info.stream], blob))
            if self._link:
                k = self.channels[info.stream]
                self.message_port_pub("link", _link_message(blob, info, met[0], row=int(info.stream), grid_index=k, sf=int(self.sf),
                                                            freq_hz=self.filterbank.channel_freq(k), bandwidth=self.filterbank.bandwidth,
                                                            row_rate=float(self.samp_rate) / self.decimation))

    def close(self):
        self.mux.close()
        self.filterbank.close()


def lorawan_reduced_rate(sf, bandwidth) -> bool:
    """LoRaWAN's low-data-rate rule: on where the symbol time 2^SF / bandwidth is at least 16 ms (SF11 and SF12 at 125 kHz)."""
    return (1 << int(sf)) / float(bandwidth) >= 16e-3


class multi_sf_gateway_receiver(_MsgBlock):
    """A gateway's receiver for every spreading factor at once: one wide-band capture -> the polyphase filter bank, run once per
    step, whose rows go straight into one decoder mux per SF on the device (capi.Gateway, include/lora_hip_gateway.h).
    Each frame is published unchanged on "frames", as (grid_index, blob) on "channel_frames" and as (grid_index, sf, blob) on
    "sf_frames"; per (channel, SF) the frames are gateway_receiver(sf=SF)'s on the same capture.
    reduced_rate: None = LoRaWAN's rule per SF (lorawan_reduced_rate), a bool for every SF, or a dict {sf: bool}."""

    def __init__(self, samp_rate, center_freq, grid_offset, n_grid, channels, bandwidth, sfs=(7, 8, 9, 10, 11, 12), implicit=False, cr=4,
                 crc=True, reduced_rate=None, decimation=1, device=0, demod=capi.DEMOD_FFT_COMPAT, latency_ms=None, link_metrics=False):
        super().__init__()
        self._link = bool(link_metrics)
        self._grid = (float(center_freq) + float(grid_offset), float(samp_rate) / int(n_grid))   # frequency of grid channel 0, channel spacing
        self.bandwidth = int(bandwidth)
        self.samp_rate = samp_rate
        self.center_freq = center_freq
        self.channels = [int(k) for k in channels]
        self.sfs = [int(s) for s in sfs]
        self.decimation = int(decimation)
        self.device = int(device)
        for sf in self.sfs:
            if sf < 6 or sf > 12:  # as decoder (decoder_impl.cc:57-61)
                sys.stderr.write("[LoRa Decoder] ERROR : Spreading factor should be between 6 and 12 (inclusive)!\n"
                                 "                       Other values are currently not supported.\n")
                raise SystemExit(1)

        def ldro(sf):
            if reduced_rate is None:
                return lorawan_reduced_rate(sf, bandwidth)
            if isinstance(reduced_rate, dict):
                return bool(reduced_rate.get(sf, lorawan_reduced_rate(sf, bandwidth)))
            return bool(reduced_rate)

        self.reduced_rate = {sf: ldro(sf) for sf in self.sfs}
        decoders = [dict(sf=sf, implicit=implicit, cr=cr, crc=crc, reduced_rate=self.reduced_rate[sf], demod=demod) for sf in self.sfs]
        self.gateway = capi.Gateway(samp_rate, grid_offset, n_grid, self.channels, bandwidth, decoders, self.decimation, device)
        if latency_ms is not None:
            self.gateway.set_latency(float(latency_ms))
        self.message_port_register_out("frames")
        self.message_port_register_out("channel_frames")
        self.message_port_register_out("sf_frames")
        self.message_port_register_out("link")
        if self._link:
            self.gateway.enable_link(True)

    def work(self, input_items, scale=0) -> int:
        """numpy complex64 (host), or a torch CUDA tensor (complex64, or float32 interleaved) read on the current stream; or integer
        IQ: a numpy array or a torch CUDA tensor of dtype int16 / int8 / uint8, flat interleaved or (n, 2), with an optional scale."""
        if hasattr(input_items, "is_cuda") and input_items.is_cuda:
            import torch
            t = input_items.contiguous()
            if t.device.index != self.device:
                raise ValueError("multi_sf_gateway_receiver.work: the tensor is on %s, the gateway on cuda:%d" % (t.device, self.device))
            fmt = {torch.int16: iqformat.SC16, torch.int8: iqformat.SC8, torch.uint8: iqformat.CU8}.get(t.dtype)
            if fmt is not None:
                if not (t.dim() == 1 or (t.dim() == 2 and t.shape[1] == 2)) or t.numel() % 2:
                    raise ValueError("multi_sf_gateway_receiver.work: integer IQ must be flat interleaved pairs or shaped (n, 2), not %s" % (tuple(t.shape),))
                n = t.numel() // 2
                self.gateway.work_device_raw(t.data_ptr(), n, fmt, iqformat.check_scale(scale), torch.cuda.current_stream(t.device).cuda_stream)
                self._publish()
                return n
            if scale:
                raise TypeError("multi_sf_gateway_receiver.work: scale applies to integer IQ, not to %s" % t.dtype)
            if t.dtype == torch.complex64:
                n = t.numel()
            elif t.dtype == torch.float32:
                if t.numel() % 2:
                    raise ValueError("multi_sf_gateway_receiver.work: a float32 tensor holds interleaved I/Q pairs, not %d floats" % t.numel())
                n = t.numel() // 2
            else:
                raise TypeError("multi_sf_gateway_receiver.work: a device tensor must be complex64 or float32 interleaved, not %s" % t.dtype)
            self.gateway.work_device(t.data_ptr(), n, torch.cuda.current_stream(t.device).cuda_stream)
        else:
            raw = _integer_iq(input_items, scale)
            if raw is not None:
                n = raw[2]
                self.gateway.work_raw(raw[0], raw[1], scale)
            else:
                x = np.asarray(input_items, dtype=np.complex64)
                n = x.size
                self.gateway.work(x)
        self._publish()
        return n

    def stop(self):
        self.gateway.flush()
        self._publish()

    def stats(self) -> dict:
        return self.gateway.stats()

    def _publish(self):
        for blob, info, *met in (self.gateway.drain_link() if self._link else self.gateway.drain()):
            self.message_port_pub("frames", blob)
            self.message_port_pub("channel_frames", (info.grid_index, blob))
            self.message_port_pub("sf_frames", (info.grid_index, info.sf, blob))
            if self._link:
                self.message_port_pub("link", _link_message(blob, info, met[0], row=int(info.row), grid_index=int(info.grid_index), sf=int(info.sf),
                                                            freq_hz=self._grid[0] + self._grid[1] * int(info.grid_index), bandwidth=self.bandwidth,
                                                            row_rate=float(self.samp_rate) / self.decimation))

    def close(self):
        self.gateway.close()


class traffic_synthesizer:
    """The transmit side (include/lora_hip_tx.h, csrc/lora_tx.hip): frames placed in time and frequency, then the wide-band
    capture they add up to, written into device memory by one kernel per generate() - the shapes multi_sf_gateway_receiver.work
    takes.  gr_lora_amd.synth.build_wideband is the definition.  No host fall-back: without a device the constructor raises."""

    def __init__(self, samp_rate, device=0, noise_sigma=0.0, seed=0):
        self.samp_rate = float(samp_rate)
        self.device = int(device)
        self._h = capi.Tx(samp_rate, device=device, noise_sigma=noise_sigma, seed=seed)

    def add_frame(self, payload, sf, cr, bandwidth, start, freq_hz, amplitude=1.0, crc=True, implicit=False, reduced_rate=None):
        """One emitter: first sample at absolute index start, centre freq_hz from the capture's centre.  reduced_rate None:
        LoRaWAN's rule (lorawan_reduced_rate).  Header checksum and payload CRC are the valid ones.
        -> (the blob tail a decoder publishes for it, as synth.expected_frame_tail; the frame's item count)."""
        from . import synth
        pl = bytes(payload)
        rr = lorawan_reduced_rate(sf, bandwidth) if reduced_rate is None else bool(reduced_rate)
        f = capi.tx_frame(pl, sf, cr, bandwidth, start=start, freq_hz=freq_hz, amplitude=amplitude, crc=crc, implicit=implicit, reduced_rate=rr)
        items = capi.tx_frame_items(f, self.samp_rate)
        self._h.add_frames([f])
        cfg = synth.TxConfig(sf=int(sf), cr=int(cr), bw=int(bandwidth), crc=bool(crc), implicit=bool(implicit), reduced_rate=rr,
                             hdr_nibbles=synth.valid_hdr_nibbles(len(pl), int(cr), bool(crc)))
        return synth.expected_frame_tail(pl, cfg, synth.valid_crc_bytes(pl)), items

    def generate(self, n, fmt="cf32", full_scale=None, out=None):
        """The next n items as a torch CUDA tensor, written on the current stream: complex64[n], or for fmt sc16 / sc8 / cu8 flat
        interleaved int16 / int8 / uint8[2 n] equal to iqformat.quantize(the complex64 items, fmt, full_scale) (full_scale None:
        the type's largest value, 32767 or 127).  out: a tensor of that dtype and size to fill instead."""
        import torch
        f = iqformat.format_from_name(fmt)
        dtype = {iqformat.CF32: torch.complex64, iqformat.SC16: torch.int16, iqformat.SC8: torch.int8, iqformat.CU8: torch.uint8}[f]
        numel = int(n) if f == iqformat.CF32 else 2 * int(n)
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.empty(numel, dtype=dtype, device=dev)
        elif not (out.is_cuda and out.device.index == self.device and out.dtype == dtype and out.numel() == numel and out.is_contiguous()):
            raise ValueError("traffic_synthesizer.generate: out must be a contiguous %s tensor of %d elements on cuda:%d" % (dtype, numel, self.device))
        stream = torch.cuda.current_stream(dev).cuda_stream
        if f == iqformat.CF32:
            self._h.generate_device(out.data_ptr(), int(n), stream)
        else:
            fs = float(full_scale) if full_scale is not None else (32767.0 if f == iqformat.SC16 else 127.0)
            self._h.generate_device_raw(out.data_ptr(), int(n), f, fs, stream)
        return out

    @property
    def position(self) -> int:
        return self._h.position

    @property
    def pending(self) -> int:
        return self._h.pending

    def kernel_ms(self) -> float:
        return self._h.kernel_ms()

    def close(self):
        self._h.close()


class spectrum_record:
    """What spectrum_scanner.work returns: psd[rows, nfft] (full-scale^2 per bin, centred: index nfft / 2 is DC), peak[rows, nfft] or
    None, band[rows, n_bands] or None (float32 numpy), first_sample[rows] (absolute index of each row's first sample) and
    freqs[nfft] (Hz from the capture's centre)."""

    def __init__(self, psd, peak, band, first_sample, freqs):
        self.psd, self.peak, self.band, self.first_sample, self.freqs = psd, peak, band, first_sample, freqs

    def __len__(self):
        return int(self.psd.shape[0])


class spectrum_scanner:
    """The spectral scan (include/lora_hip_spectrum.h, csrc/lora_spectrum.hip): Welch rows of the capture's power spectrum and
    the power in each band, computed on the device in one pass.  Feed it what multi_sf_gateway_receiver.work is fed, in any
    chunking: the rows are the same.  gr_lora_amd.spectrum.welch_rows is the definition.  hop None: nfft // 2.  bands: (f_lo, f_hi)
    pairs in Hz from the capture's centre (a bin belongs to a band when its centre lies in [f_lo, f_hi)).  No host fall-back."""

    def __init__(self, samp_rate, nfft=1024, hop=None, n_avg=16, window="hann", peak=False, bands=None, device=0, _bins=None):
        from . import spectrum
        self.samp_rate = float(samp_rate)
        self.nfft = int(nfft)
        self.hop = self.nfft // 2 if hop is None else int(hop)
        self.n_avg = int(n_avg)
        self.device = int(device)
        self.bands = [(float(lo), float(hi)) for lo, hi in (bands or [])]
        self.band_bins = list(_bins) if _bins is not None else [spectrum.band_bins(self.samp_rate, self.nfft, lo, hi) for lo, hi in self.bands]
        self.freqs = spectrum.freqs(self.samp_rate, self.nfft)
        self._h = capi.Spectrum(self.samp_rate, self.nfft, self.hop, self.n_avg, spectrum.window_id(window), bool(peak), self.band_bins, self.device)
        self.window = self._h.window()

    @classmethod
    def for_grid(cls, samp_rate, grid_offset, n_grid, channels, bandwidth, nfft=1024, hop=None, n_avg=16, window="hann", peak=False, device=0):
        """One band per filter-bank channel (spectrum.grid_bands): band c is grid_offset + channels[c] * samp_rate / n_grid, +- bandwidth / 2."""
        from . import spectrum
        bins = spectrum.grid_bands(samp_rate, nfft, grid_offset, n_grid, channels, bandwidth)
        f = [float(grid_offset) + int(k) * float(samp_rate) / int(n_grid) for k in channels]
        return cls(samp_rate, nfft, hop, n_avg, window, peak, [(x - bandwidth / 2.0, x + bandwidth / 2.0) for x in f], device, _bins=bins)

    def _record(self, psd, peak, band, first_row):
        first = (int(first_row) + np.arange(psd.shape[0], dtype=np.int64)) * (self.n_avg * self.hop)
        return spectrum_record(psd, peak, band, first, self.freqs)

    def work(self, x, scale=0) -> spectrum_record:
        """numpy complex64 (host), or a torch CUDA tensor (complex64, or float32 interleaved) read on the current stream; or integer
        IQ: a numpy array or a torch CUDA tensor of dtype int16 / int8 / uint8, flat interleaved or (n, 2), with an optional scale."""
        if hasattr(x, "is_cuda") and x.is_cuda:
            import torch
            t = x.contiguous()
            if t.device.index != self.device:
                raise ValueError("spectrum_scanner.work: the tensor is on %s, the scanner on cuda:%d" % (t.device, self.device))
            fmt = {torch.int16: iqformat.SC16, torch.int8: iqformat.SC8, torch.uint8: iqformat.CU8}.get(t.dtype)
            if fmt is not None:
                if not (t.dim() == 1 or (t.dim() == 2 and t.shape[1] == 2)) or t.numel() % 2:
                    raise ValueError("spectrum_scanner.work: integer IQ must be flat interleaved pairs or shaped (n, 2), not %s" % (tuple(t.shape),))
                n = t.numel() // 2
                sc = iqformat.check_scale(scale)
            else:
                if scale:
                    raise TypeError("spectrum_scanner.work: scale applies to integer IQ, not to %s" % t.dtype)
                if t.dtype == torch.complex64:
                    n = t.numel()
                elif t.dtype == torch.float32:
                    if t.numel() % 2:
                        raise ValueError("spectrum_scanner.work: a float32 tensor holds interleaved I/Q pairs, not %d floats" % t.numel())
                    n = t.numel() // 2
                else:
                    raise TypeError("spectrum_scanner.work: a device tensor must be complex64 or float32 interleaved, not %s" % t.dtype)
            rows = self._h.output_rows(n)
            r = max(rows, 1)
            psd = torch.empty((r, self.nfft), dtype=torch.float32, device=t.device)
            peak = torch.empty((r, self.nfft), dtype=torch.float32, device=t.device) if self._h.peak else None
            band = torch.empty((r, self._h.n_bands), dtype=torch.float32, device=t.device) if self._h.n_bands else None
            stream = torch.cuda.current_stream(t.device).cuda_stream
            ptrs = (psd.data_ptr(), None if peak is None else peak.data_ptr(), None if band is None else band.data_ptr())
            if fmt is not None:
                got, first = self._h.run_device_raw(t.data_ptr(), n, fmt, *ptrs, self.nfft, rows, sc, stream)
            else:
                got, first = self._h.run_device(t.data_ptr(), n, *ptrs, self.nfft, rows, stream)
            return self._record(psd[:got].cpu().numpy(), None if peak is None else peak[:got].cpu().numpy(),
                                None if band is None else band[:got].cpu().numpy(), first)
        raw = _integer_iq(x, scale)
        if raw is not None:
            return self._record(*self._h.work_raw(raw[0], raw[1], scale))
        return self._record(*self._h.work(np.asarray(x, dtype=np.complex64)))

    def reset(self):
        """Drops the samples and the row in progress: the next item is sample 0."""
        self._h.reset()

    def kernel_ms(self) -> float:
        return self._h.kernel_ms()

    def close(self):
        self._h.close()


class rational_resampler:
    """The stage in front of the receivers for a capture whose rate is no multiple of the LoRa bandwidth (include/
    lora_hip_resampler.h, csrc/lora_resampler.hip): the stream at in_rate -> the stream at out_rate = in_rate * L / M, on the device,
    in any chunking.  gr_lora_amd.resampler.resample is the definition.  Frame positions reported downstream refer to the
    resampled stream; `delay` is the filter's group delay in output items.  No host fall-back."""

    def __init__(self, in_rate, out_rate, zero_crossings=16, beta=8.0, cutoff=0.8, device=0):
        from . import resampler
        self.in_rate, self.out_rate = float(in_rate), float(out_rate)
        self.interpolation, self.decimation = resampler.ratio(in_rate, out_rate)
        self.device = int(device)
        self._h = capi.Resampler(self.interpolation, self.decimation, zero_crossings, beta, cutoff, self.device)
        self.delay = self._h.delay()

    def work(self, input_items, scale=0):
        """numpy complex64 (host), or a torch CUDA tensor (complex64, or float32 interleaved) read on the current stream; or integer
        IQ: a numpy array or a torch CUDA tensor of dtype int16 / int8 / uint8, flat interleaved or (n, 2), with an optional scale.
        -> the complex64 outputs these items complete: a numpy array for host input, a CUDA tensor written on the current stream
        for device input."""
        x = input_items
        if hasattr(x, "is_cuda") and x.is_cuda:
            import torch
            t = x.contiguous()
            if t.device.index != self.device:
                raise ValueError("rational_resampler.work: the tensor is on %s, the resampler on cuda:%d" % (t.device, self.device))
            fmt = {torch.int16: iqformat.SC16, torch.int8: iqformat.SC8, torch.uint8: iqformat.CU8}.get(t.dtype)
            if fmt is not None:
                if not (t.dim() == 1 or (t.dim() == 2 and t.shape[1] == 2)) or t.numel() % 2:
                    raise ValueError("rational_resampler.work: integer IQ must be flat interleaved pairs or shaped (n, 2), not %s" % (tuple(t.shape),))
                n = t.numel() // 2
                sc = iqformat.check_scale(scale)
            else:
                if scale:
                    raise TypeError("rational_resampler.work: scale applies to integer IQ, not to %s" % t.dtype)
                if t.dtype == torch.complex64:
                    n = t.numel()
                elif t.dtype == torch.float32:
                    if t.numel() % 2:
                        raise ValueError("rational_resampler.work: a float32 tensor holds interleaved I/Q pairs, not %d floats" % t.numel())
                    n = t.numel() // 2
                else:
                    raise TypeError("rational_resampler.work: a device tensor must be complex64 or float32 interleaved, not %s" % t.dtype)
            cap = self._h.output_items(n)
            y = torch.empty(max(cap, 1), dtype=torch.complex64, device=t.device)
            stream = torch.cuda.current_stream(t.device).cuda_stream
            if fmt is not None:
                got, _first = self._h.run_device_raw(t.data_ptr(), n, fmt, y.data_ptr(), cap, sc, stream)
            else:
                got, _first = self._h.run_device(t.data_ptr(), n, y.data_ptr(), cap, stream)
            return y[:got]
        raw = _integer_iq(x, scale)
        if raw is not None:
            return self._h.work_raw(raw[0], raw[1], scale)[0]
        return self._h.work(np.asarray(x, dtype=np.complex64))[0]

    def reset(self):
        """Drops the carried items: the next item is sample 0 of a new stream."""
        self._h.reset()

    def kernel_ms(self) -> float:
        return self._h.kernel_ms()

    def close(self):
        self._h.close()


class iq_conditioner:
    """The first stage for a capture from a direct-conversion front end (include/lora_hip_conditioner.h, csrc/lora_conditioner.hip):
    removes the DC offset and corrects the gain / phase mismatch between I and Q, both estimated over the last `window` blocks of
    `block` items, on the device, in any chunking.  cf32 out at the input's rate, item for item; up to block - 1 items wait for
    their block to complete (flush() emits them).  gr_lora_amd.conditioner.condition is the definition.  No host fall-back."""

    def __init__(self, block=4096, window=16, dc=True, iq=True, device=0):
        self.block, self.window, self.dc, self.iq = int(block), int(window), bool(dc), bool(iq)
        self.device = int(device)
        self._h = capi.Conditioner(self.block, self.window, self.dc, self.iq, self.device)
        self._last_device = None                      # the device of the last device tensor: flush() answers in kind

    def work(self, input_items, scale=0):
        """numpy complex64 (host), or a torch CUDA tensor (complex64, or float32 interleaved) read on the current stream; or integer
        IQ: a numpy array or a torch CUDA tensor of dtype int16 / int8 / uint8, flat interleaved or (n, 2), with an optional scale.
        -> the complex64 items of the blocks these items complete: a numpy array for host input, a CUDA tensor written on the
        current stream for device input."""
        x = input_items
        if hasattr(x, "is_cuda") and x.is_cuda:
            import torch
            t = x.contiguous()
            if t.device.index != self.device:
                raise ValueError("iq_conditioner.work: the tensor is on %s, the conditioner on cuda:%d" % (t.device, self.device))
            fmt = {torch.int16: iqformat.SC16, torch.int8: iqformat.SC8, torch.uint8: iqformat.CU8}.get(t.dtype)
            if fmt is not None:
                if not (t.dim() == 1 or (t.dim() == 2 and t.shape[1] == 2)) or t.numel() % 2:
                    raise ValueError("iq_conditioner.work: integer IQ must be flat interleaved pairs or shaped (n, 2), not %s" % (tuple(t.shape),))
                n = t.numel() // 2
                sc = iqformat.check_scale(scale)
            else:
                if scale:
                    raise TypeError("iq_conditioner.work: scale applies to integer IQ, not to %s" % t.dtype)
                if t.dtype == torch.complex64:
                    n = t.numel()
                elif t.dtype == torch.float32:
                    if t.numel() % 2:
                        raise ValueError("iq_conditioner.work: a float32 tensor holds interleaved I/Q pairs, not %d floats" % t.numel())
                    n = t.numel() // 2
                else:
                    raise TypeError("iq_conditioner.work: a device tensor must be complex64 or float32 interleaved, not %s" % t.dtype)
            cap = self._h.output_items(n)
            y = torch.empty(max(cap, 1), dtype=torch.complex64, device=t.device)
            stream = torch.cuda.current_stream(t.device).cuda_stream
            if fmt is not None:
                got, _first = self._h.run_device_raw(t.data_ptr(), n, fmt, y.data_ptr(), cap, sc, stream)
            else:
                got, _first = self._h.run_device(t.data_ptr(), n, y.data_ptr(), cap, stream)
            self._last_device = t.device
            return y[:got]
        self._last_device = None
        raw = _integer_iq(x, scale)
        if raw is not None:
            return self._h.work_raw(raw[0], raw[1], scale)[0]
        return self._h.work(np.asarray(x, dtype=np.complex64))[0]

    def flush(self):
        """The held items, corrected with the newest block's parameters: a CUDA tensor if the last work() took one, else numpy."""
        if self._last_device is not None:
            import torch
            cap = self._h.held_items()
            y = torch.empty(max(cap, 1), dtype=torch.complex64, device=self._last_device)
            got, _first = self._h.flush_device(y.data_ptr(), cap, torch.cuda.current_stream(self._last_device).cuda_stream)
            return y[:got]
        return self._h.flush()[0]

    def estimate(self) -> dict:
        """What the newest block's window says about the front end: dc (complex), dc_dbfs (|dc| against full scale 1.0), gain_db and
        phase_deg of the I/Q mismatch (g = sqrt(q), phi = asin(r / sqrt(q)), formed here from the device's fp64 estimates)."""
        from . import conditioner
        _par, est = self._h.newest()
        return conditioner.mismatch(*est)

    def set_fixed(self, d_i, d_q, a, b):
        """Calibrated constants instead of estimates: zI = I - d_i, zQ = a zI + b (Q - d_q)."""
        self._h.set_fixed(d_i, d_q, a, b)

    def set_adaptive(self):
        self._h.set_adaptive()

    def reset(self):
        """Drops the held items and the window: the next item is sample 0 of a new stream."""
        self._h.reset()

    def kernel_ms(self) -> float:
        return self._h.kernel_ms()

    def close(self):
        self._h.close()


class modulator:
    """The mirror of `decoder`: payload bytes in, the frame's baseband samples out, made on the device by traffic_synthesizer
    with one emitter at the capture's centre.  samp_rate / bandwidth must be an integer."""

    def __init__(self, samp_rate, bandwidth, sf, implicit, cr, crc, reduced_rate=False, device=0):
        self.samp_rate, self.bandwidth, self.sf, self.implicit, self.cr, self.crc = samp_rate, int(bandwidth), int(sf), bool(implicit), int(cr), bool(crc)
        self.reduced_rate = bool(reduced_rate)
        self._tx = traffic_synthesizer(samp_rate, device=device)

    def modulate(self, payload, gap_items=0, amplitude=1.0, device_out=False):
        """gap_items of silence, then the frame: complex64 numpy, or a torch CUDA tensor with device_out=True."""
        gap = int(gap_items)
        _tail, items = self._tx.add_frame(payload, self.sf, self.cr, self.bandwidth, self._tx.position + gap, 0.0, amplitude=amplitude, crc=self.crc,
                                          implicit=self.implicit, reduced_rate=self.reduced_rate)
        t = self._tx.generate(gap + items)
        return t if device_out else t.cpu().numpy()

    def close(self):
        self._tx.close()


class weak_signal_receiver(_MsgBlock):
    """The low-SNR receive path on one whole capture: lora_hip_detect_preambles_device finds the preambles in the dechirped spectrum, where
    the reference's time-domain gates acquire nothing, and lora_hip_soft_decode_at_headers_device decodes from those header positions with
    soft decisions (include/lora_hip_soft.h; soft=False: lora_hip_decode_at_headers_device's hard decisions, for comparison).  Explicit
    header, FFT demodulator, no drift correction.  Frames are published on "frames".

    SF 7 .. 12 (the soft decoder needs the five header codewords an SF6 header block has no room for: ValueError).

    crc_repair = L in 1 .. 8 (soft only; 0, the default: off): lora_hip_soft_crc_repair_enable.  A published frame whose payload CRC fails takes the
    cheapest pattern of runner-up nibbles among its L least reliable body codewords that makes the CRC hold; every result then carries
    "repair", the record of what was changed.  A 16-bit CRC also accepts wrong patterns (DESIGN.md 4.19.1 has the measured rate): a frame with
    repair["status"] == capi.SOFT_REPAIR_REPAIRED is less certain than one whose CRC held.

    Batch, not streaming: every call of work() is a capture of its own, nothing is carried from one call to the next, and a frame cut by
    the end of the capture is lost."""

    def __init__(self, samp_rate, bandwidth, sf, cr, crc, reduced_rate=False, threshold=0, require_header_checksum=True, soft=True, device=0, crc_repair=0):
        super().__init__()
        if not 7 <= int(sf) <= 12:
            raise ValueError("weak_signal_receiver: sf must be 7 .. 12, not %r" % (sf,))
        if not 0 <= int(crc_repair) <= capi.SOFT_REPAIR_MAX_CANDIDATES or (crc_repair and not soft):
            raise ValueError("weak_signal_receiver: crc_repair is 0 .. %d and needs soft=True, not %r" % (capi.SOFT_REPAIR_MAX_CANDIDATES, crc_repair))
        self.crc_repair = int(crc_repair)
        self.threshold, self.soft, self.device = float(threshold), bool(soft), int(device)
        self.flags = capi.SOFT_REQUIRE_HEADER_CHECKSUM if require_header_checksum else 0
        self._h = capi.Handle(samp_rate=samp_rate, bandwidth=bandwidth, sf=sf, implicit=False, cr=cr, crc=crc, reduced_rate=reduced_rate,
                              disable_drift_correction=True, device=device, demod=capi.DEMOD_FFT)
        if self.crc_repair:
            self._h.soft_crc_repair_enable(self.crc_repair)
        self.message_port_register_out("frames")

    def _device_cf32(self, capture, scale):
        """(tensor that owns the complex64 items on the device, their count)"""
        import torch
        x = capture
        dev = torch.device("cuda", self.device)
        if not (hasattr(x, "is_cuda") and x.is_cuda):
            raw = _integer_iq(x, scale)
            x = torch.from_numpy(raw[0]).to(dev) if raw is not None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.complex64).view(np.float32)).to(dev)
        t = x.contiguous()
        if t.device.index != self.device:
            raise ValueError("weak_signal_receiver.work: the tensor is on %s, the receiver on cuda:%d" % (t.device, self.device))
        fmt = {torch.int16: iqformat.SC16, torch.int8: iqformat.SC8, torch.uint8: iqformat.CU8}.get(t.dtype)
        if fmt is not None:
            if not (t.dim() == 1 or (t.dim() == 2 and t.shape[1] == 2)) or t.numel() % 2:
                raise ValueError("weak_signal_receiver.work: integer IQ must be flat interleaved pairs or shaped (n, 2), not %s" % (tuple(t.shape),))
            n = t.numel() // 2
            y = torch.empty(max(n, 1), dtype=torch.complex64, device=dev)
            capi.unpack_device(t.data_ptr(), n, fmt, y.data_ptr(), iqformat.check_scale(scale), self.device, torch.cuda.current_stream(dev).cuda_stream)
            return y, n
        if scale:
            raise TypeError("weak_signal_receiver.work: scale applies to integer IQ, not to %s" % t.dtype)
        if t.dtype == torch.complex64:
            return t, t.numel()
        if t.dtype == torch.float32 and t.numel() % 2 == 0:
            return t, t.numel() // 2
        raise TypeError("weak_signal_receiver.work: a capture is complex64, float32 interleaved or int16 / int8 / uint8 IQ, not %s" % t.dtype)

    def work(self, capture, scale=0) -> List[dict]:
        """One whole capture: numpy complex64, integer IQ (int16 / int8 / uint8, flat interleaved or (n, 2), with an optional scale), or a
        torch CUDA tensor of either kind.  -> one dict per detected preamble, in the detector's order: its fields (header_pos, cfo_hz, pmr ...),
        the decoder's report (soft: status, cr, payload_length, crc_ok, changed, min_margin ...; with crc_repair also "repair": status,
        candidates, pattern, changed, syndrome, penalty, codewords) and "frame": the published blob or None."""
        import torch
        t, n = self._device_cf32(capture, scale)
        stream = torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream
        det = self._h.detect_preambles_device(t.data_ptr(), n, [0], [n], self.threshold, stream)
        det = [d for d in det if d["header_pos"] + 2 * self._h.sps <= n]   # (a header inside the capture's last two symbols: cut by its end)
        if self.soft:
            reports = self._h.soft_decode_at_headers_device(t.data_ptr(), n, [0], [n], det, self.flags, stream)
            if self.crc_repair:
                reports = [dict(r, repair=rec) for r, rec in zip(reports, self._h.soft_crc_repair_results())]
        else:
            self._h.decode_at_headers_device(t.data_ptr(), n, [0], [n], det, stream)
            reports = [dict() for _ in det]
        frames = self._h.drain()
        out, k = [], 0
        for d, r in zip(det, reports):
            blob = None
            if k < len(frames) and frames[k][1].header_pos == d["header_pos"]:
                blob = frames[k][0]
                k += 1
            out.append(dict(d, **r, frame=blob))
        for blob, _info in frames:
            self.message_port_pub("frames", blob)
        return out

    def close(self):
        self._h.close()


class lora_receiver(_MsgBlock):
    """python/lora_receiver.py:26-89: [conjugate] o (channelizer | resampler) -> decoder."""

    def __init__(self, samp_rate, center_freq, channel_list, bandwidth, sf, implicit, cr, crc, reduced_rate=False,
                 conj=False, decimation=1, disable_channelization=False, disable_drift_correction=False, cfo_correction=False,
                 **decoder_kw):
        super().__init__()
        self.samp_rate = samp_rate
        self.center_freq = center_freq
        self.channel_list = channel_list
        self.bandwidth = bandwidth
        self.sf = sf
        self.implicit = implicit
        self.cr = cr
        self.crc = crc
        self.decimation = decimation
        self.conj = conj
        self.disable_channelization = disable_channelization
        self.disable_drift_correction = disable_drift_correction
        self.channelizer = None if disable_channelization else channelizer(samp_rate, center_freq, channel_list, bandwidth, decimation)
        self.decoder = decoder(samp_rate / decimation, bandwidth, sf, implicit, cr, crc, reduced_rate,
                               disable_drift_correction, cfo_estimates=bool(cfo_correction), **decoder_kw)
        self.cfo_log = []                             # estimates in Hz, as applied
        self._fed = 0                                 # items handed to the decoder so far
        self._cfo_valid_from = 0
        if cfo_correction and self.channelizer is not None:
            # msg_connect((self.decoder, 'control'), (self.channelizer, 'control')) (python/lora_receiver.py:67) with the
            # message upstream left commented out; conj flips the spectrum in front of the decoder, hence the sign
            def on_control(msg):
                if isinstance(msg, tuple) and msg[0] == "cfo":
                    if msg[2] < self._cfo_valid_from:   # measured on samples filtered before the last correction: already accounted for
                        return
                    hz = -msg[1] if self.conj else msg[1]
                    self.cfo_log.append(hz)
                    self.channelizer.apply_cfo(hz)
                    self._cfo_valid_from = self._fed    # decoder-input index from which the new tuning holds
            self.decoder.subscribe("control", on_control)
        self.message_port_register_out("frames")     # message_port_register_hier_out('frames')
        self.decoder.subscribe("frames", lambda blob: self.message_port_pub("frames", blob))

    def work(self, input_items, scale=0) -> int:
        raw = _integer_iq(input_items, scale)
        if raw is not None:
            return self._work_integer(raw, scale)
        x = np.asarray(input_items, dtype=np.complex64)
        if self.disable_channelization:
            y = x[:: int(self.decimation)] if self.decimation != 1 else x   # fractional_resampler_cc(0, decimation)
        else:
            y = self.channelizer.work(x)
        if self.conj:
            y = np.conj(y)
        self._fed += int(np.asarray(y).size)
        self.decoder.work(y)
        return x.size

    def _work_integer(self, raw, scale) -> int:
        """Integer IQ: the channeliser converts it as it filters; without one the decoder takes the (decimated) integers themselves.
        Only a conjugation in front of a decoder that has no channeliser needs complex samples on the host."""
        a, fmt, n = raw
        if not self.disable_channelization:
            y = self.channelizer.work(a, scale)
            y = np.conj(y) if self.conj else y
            self._fed += int(y.size)
            self.decoder.work(y)
            return n
        y = a.reshape(-1, 2)[:: int(self.decimation)].reshape(-1) if self.decimation != 1 else a
        self._fed += y.size // 2
        if self.conj:
            self.decoder.work(np.conj(iqformat.to_cf32(y, fmt, scale)))
        else:
            self.decoder.work(np.ascontiguousarray(y), scale)
        return n

    def stop(self):
        self.decoder.stop()

    def get_sf(self):
        return self.sf

    def set_sf(self, sf):
        self.sf = sf
        self.decoder.set_sf(self.sf)

    def get_center_freq(self):
        return self.center_freq

    def set_center_freq(self, center_freq):
        # upstream calls a channelizer method that does not exist (lora_receiver.py:89); here it retunes
        self.center_freq = center_freq
        if self.channelizer is not None:
            self.channelizer.retune(center_freq)


class message_socket_sink(_MsgBlock):
    """PMT blob -> UDP datagram; `layer` strips headers (lib/message_socket_sink_impl.cc:93-122):
    0 LORATAP: whole blob; 1 LORAPHY: drop loratap; 2 LORAMAC: drop loratap + PHY header and the 2 CRC bytes."""

    def __init__(self, ip="127.0.0.1", port=40868, layer=0):
        super().__init__()
        self.addr = (ip, int(port))
        self.layer = int(layer)
        self._sock = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        self.message_port_register_in("in", self.handle)

    def handle(self, blob: bytes):
        if self.layer == 0:
            data = blob
        elif self.layer == 1:
            data = blob[LORATAP_LEN:]
        else:
            phy = blob[LORATAP_LEN:LORATAP_LEN + LORAPHY_LEN]
            has_mac_crc = (phy[1] >> 4) & 1
            end = len(blob) - (MAC_CRC_SIZE if has_mac_crc else 0)
            data = blob[LORATAP_LEN + LORAPHY_LEN:end]
        self._sock.sendto(data, self.addr)

    def close(self):
        self._sock.close()


class packet_forwarder_sink(_MsgBlock):
    """"link" messages -> Semtech UDP packet-forwarder PUSH_DATA datagrams (gr_lora_amd/forwarder.py), one per message.  A message
    that carries no freq_hz (lora.decoder's) is reported at the `freq_hz` given here."""

    def __init__(self, host, port, gateway_eui, rssi_offset_db=0.0, freq_hz=0.0):
        super().__init__()
        from . import forwarder
        self._fw = forwarder
        self.addr = (host, int(port))
        self.eui = forwarder.eui_bytes(gateway_eui)
        self.rssi_offset_db = float(rssi_offset_db)
        self.freq_hz = float(freq_hz)
        self.sent = 0
        self._sock = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        self.message_port_register_in("link", self.handle)
        self.message_port_register_in("in", self.handle)

    def handle(self, link: dict):
        pk = self._fw.rxpk(link["blob"], link, freq_hz=link.get("freq_hz", self.freq_hz), sf=link["sf"], bandwidth=link["bandwidth"],
                           row_rate=link["row_rate"], rssi_offset_db=self.rssi_offset_db)
        self._sock.sendto(self._fw.push_data(self.eui, [pk]), self.addr)
        self.sent += 1

    def close(self):
        self._sock.close()


class message_file_sink(_MsgBlock):
    """PMT blob -> appended to a binary file, flushed (lib/message_file_sink_impl.cc)."""

    def __init__(self, path):
        super().__init__()
        self._f = open(path, "ab")
        self.message_port_register_in("in", self.handle)

    def handle(self, blob: bytes):
        self._f.write(blob)
        self._f.flush()

    def close(self):
        self._f.close()


class LoRaUDPServer:
    """python/lorasocket.py:18-34: collect n datagrams as hex strings."""

    def __init__(self, ip="127.0.0.1", port=40868, timeout=10):
        self.s = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        self.s.bind((ip, port))
        self.s.settimeout(timeout)

    def get_payloads(self, number_of_payloads):
        out = []
        for _ in range(number_of_payloads):
            try:
                data = self.s.recvfrom(65535)[0]
                out.append(data.hex() if data else "")
            except socket.timeout:
                pass
        return out

    def close(self):
        self.s.close()
