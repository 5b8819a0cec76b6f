"""ctypes binding of the C ABI declared in include/lora_hip.h (liblora_hip.so).

The library is loaded on first use; if it is missing or no MI355X is visible the
calls raise -- there is no CPU fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LORA_HIP_LIB") or os.path.join(_HERE, "liblora_hip.so")  # (LORA_HIP_LIB: a library variant, tools/ab.sh)

DEMOD_GRAD, DEMOD_FFT, DEMOD_FFT_COMPAT = 0, 1, 2
FLAG_TRACE = 1
FLAG_PIN_HOST = 2
FLAG_FAST_SYNC = 4  # keep SYNC's closed-form maximum (no exact re-evaluation of near-tied shifts)
FLAG_NO_DECOUPLED = 8  # never run a pass decoupled (header-only jobs + the symbol-parallel payload pass)
IQ_CF32, IQ_SC16, IQ_SC8, IQ_CU8 = 0, 1, 2, 3  # lora_hip_iq_format (include/lora_hip.h); the conversion in numpy: gr_lora_amd/iqformat.py

EXPORTS = [
    "lora_hip_abi_version", "lora_hip_strerror", "lora_hip_last_error", "lora_hip_create", "lora_hip_destroy",
    "lora_hip_get_geometry", "lora_hip_set_sf", "lora_hip_set_samp_rate", "lora_hip_work", "lora_hip_flush",
    "lora_hip_decode_device", "lora_hip_frames_available", "lora_hip_poll_frame", "lora_hip_drain_frames", "lora_hip_drain_slots", "lora_hip_demod_symbols_device", "lora_hip_demod_symbols_ex_device",
    "lora_hip_last_timing", "lora_hip_last_plan", "lora_hip_last_sync_stops", "lora_hip_get_table", "lora_hip_last_payload_pass", "lora_hip_gap_starts_device", "lora_hip_decode_device_begin", "lora_hip_decode_device_end", "lora_hip_decode_device_prepass", "lora_hip_trace", "lora_hip_trace_clear", "lora_hip_check_frame", "lora_hip_estimate_cfo_device", "lora_hip_ref_ifreq_device",
    "lora_hip_set_stream_latency", "lora_hip_stream_info", "lora_hip_stream_info_ex", "lora_hip_walker_kernel_name", "lora_hip_window_stats_device", "lora_hip_detect_preambles_device", "lora_hip_decode_at_headers_device",
    "lora_hip_mux_create", "lora_hip_mux_destroy", "lora_hip_mux_work", "lora_hip_mux_flush", "lora_hip_mux_set_latency", "lora_hip_mux_set_max_ahead", "lora_hip_mux_frames_available",
    "lora_hip_mux_poll_frame", "lora_hip_mux_passes", "lora_hip_mux_last_error",
    "lora_hip_iq_item_bytes", "lora_hip_iq_unpack_device", "lora_hip_work_raw",
]


EXPORTS_CHANNELIZER = [
    "lora_hip_channelizer_create", "lora_hip_channelizer_destroy", "lora_hip_channelizer_last_error", "lora_hip_channelizer_taps",
    "lora_hip_channelizer_output_items", "lora_hip_channelizer_run_device", "lora_hip_channelizer_work", "lora_hip_channelizer_apply_cfo",
    "lora_hip_channelizer_last_kernel_ms", "lora_hip_channelizer_run_device_raw", "lora_hip_channelizer_work_raw",
]


EXPORTS_FILTERBANK = [
    "lora_hip_filterbank_create", "lora_hip_filterbank_destroy", "lora_hip_filterbank_last_error", "lora_hip_filterbank_taps",
    "lora_hip_filterbank_output_items", "lora_hip_filterbank_run_device", "lora_hip_filterbank_run_device_rows", "lora_hip_filterbank_work",
    "lora_hip_filterbank_last_kernel_ms", "lora_hip_filterbank_run_device_raw", "lora_hip_filterbank_run_device_rows_raw", "lora_hip_filterbank_work_raw",
    "lora_hip_filterbank_get_plan",
]


EXPORTS_GATEWAY = [
    "lora_hip_gateway_create", "lora_hip_gateway_destroy", "lora_hip_gateway_last_error", "lora_hip_gateway_work", "lora_hip_gateway_work_device",
    "lora_hip_gateway_flush", "lora_hip_gateway_set_latency", "lora_hip_gateway_frames_available", "lora_hip_gateway_poll_frame", "lora_hip_gateway_stats",
    "lora_hip_gateway_work_raw", "lora_hip_gateway_work_device_raw",
]

EXPORTS_TX = [
    "lora_hip_tx_encode", "lora_hip_tx_frame_items", "lora_hip_tx_create", "lora_hip_tx_destroy", "lora_hip_tx_last_error", "lora_hip_tx_add_frames",
    "lora_hip_tx_generate_device", "lora_hip_tx_generate_device_raw", "lora_hip_tx_generate", "lora_hip_tx_position", "lora_hip_tx_pending",
    "lora_hip_tx_last_kernel_ms",
]

EXPORTS_LINK = [
    "lora_hip_link_measure_device", "lora_hip_link_combine", "lora_hip_link_enable", "lora_hip_link_poll_frame", "lora_hip_link_drain_frames",
    "lora_hip_link_mux_enable", "lora_hip_link_mux_poll_frame", "lora_hip_link_gateway_enable", "lora_hip_link_gateway_poll_frame",
    "lora_hip_link_stats",
]

EXPORTS_SPECTRUM = [
    "lora_hip_spectrum_create", "lora_hip_spectrum_destroy", "lora_hip_spectrum_last_error", "lora_hip_spectrum_window",
    "lora_hip_spectrum_output_rows", "lora_hip_spectrum_run_device", "lora_hip_spectrum_run_device_raw", "lora_hip_spectrum_work",
    "lora_hip_spectrum_work_raw", "lora_hip_spectrum_reset", "lora_hip_spectrum_last_kernel_ms",
]

EXPORTS_RESAMPLER = [
    "lora_hip_resampler_create", "lora_hip_resampler_destroy", "lora_hip_resampler_last_error", "lora_hip_resampler_taps",
    "lora_hip_resampler_ratio", "lora_hip_resampler_delay", "lora_hip_resampler_get_plan", "lora_hip_resampler_output_items",
    "lora_hip_resampler_run_device", "lora_hip_resampler_run_device_raw", "lora_hip_resampler_work", "lora_hip_resampler_work_raw",
    "lora_hip_resampler_reset", "lora_hip_resampler_last_kernel_ms",
]

EXPORTS_CONDITIONER = [
    "lora_hip_conditioner_create", "lora_hip_conditioner_destroy", "lora_hip_conditioner_last_error", "lora_hip_conditioner_output_items",
    "lora_hip_conditioner_get_plan", "lora_hip_conditioner_run_device", "lora_hip_conditioner_run_device_raw", "lora_hip_conditioner_work",
    "lora_hip_conditioner_work_raw", "lora_hip_conditioner_flush_device", "lora_hip_conditioner_flush", "lora_hip_conditioner_reset",
    "lora_hip_conditioner_set_fixed", "lora_hip_conditioner_set_adaptive", "lora_hip_conditioner_block_records", "lora_hip_conditioner_last_kernel_ms",
]

EXPORTS_SOFT = ["lora_hip_soft_symbols_device", "lora_hip_soft_decode_at_headers_device", "lora_hip_soft_crc_repair_enable",
                "lora_hip_soft_crc_repair_results", "lora_hip_soft_crc_repair_codewords"]

SOFT_REQUIRE_HEADER_CHECKSUM = 1   # include/lora_hip_soft.h
SOFT_FRAME, SOFT_HEADER_REJECTED, SOFT_CR_ZERO, SOFT_TRUNCATED = 0, 1, 2, 3   # lora_hip_soft_report_t.status
SOFT_REPAIR_NOT_ATTEMPTED, SOFT_REPAIR_CRC_HELD, SOFT_REPAIR_REPAIRED, SOFT_REPAIR_FAILED = 0, 1, 2, 3   # lora_hip_soft_repair_t.status
SOFT_REPAIR_MAX_CANDIDATES = 8
FILTERBANK_MAX_DST = 8        # include/lora_hip_filterbank.h
CONDITIONER_FLAG_DC, CONDITIONER_FLAG_IQ = 1, 2   # include/lora_hip_conditioner.h
SPECTRUM_WINDOW_HANN, SPECTRUM_WINDOW_RECT = 0, 1   # include/lora_hip_spectrum.h
SPECTRUM_FLAG_PEAK = 1
GATEWAY_MAX_DECODERS = 7      # include/lora_hip_gateway.h
GATEWAY_STEP_OUTPUTS = 65536  # include/lora_hip_gateway.h


class FilterBankConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("samp_rate", C.c_double), ("grid_offset_hz", C.c_double), ("n_grid", C.c_uint32),
                ("channels", C.POINTER(C.c_int32)), ("n_channels", C.c_uint32), ("bandwidth", C.c_uint32), ("decimation", C.c_uint32),
                ("device", C.c_int32), ("cutoff_hz", C.c_float), ("transition_hz", C.c_float), ("flags", C.c_uint32)]


class SpectrumConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("samp_rate", C.c_double), ("nfft", C.c_uint32), ("hop", C.c_uint32), ("n_avg", C.c_uint32),
                ("window", C.c_uint32), ("flags", C.c_uint32), ("bands", C.POINTER(C.c_uint32)), ("n_bands", C.c_uint32), ("device", C.c_int32)]


class ResamplerConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("interpolation", C.c_uint32), ("decimation", C.c_uint32), ("zero_crossings", C.c_uint32),
                ("beta", C.c_double), ("cutoff", C.c_double), ("device", C.c_int32), ("flags", C.c_uint32)]


class ConditionerConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("block", C.c_uint32), ("window", C.c_uint32), ("flags", C.c_uint32), ("device", C.c_int32)]


class ChannelizerConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("samp_rate", C.c_float), ("center_freq", C.c_float), ("channel_list", C.POINTER(C.c_float)),
                ("n_channels", C.c_uint32), ("bandwidth", C.c_uint32), ("decimation", C.c_uint32), ("device", C.c_int32),
                ("cutoff_hz", C.c_float), ("transition_hz", C.c_float), ("flags", C.c_uint32)]


CHANNELIZER_FLAG_UINT32_OFFSET = 1  # d_freq_offset in upstream's uint32_t arithmetic (a negative offset wraps), include/lora_hip_channelizer.h


class Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("samp_rate", C.c_float), ("bandwidth", C.c_uint32),
                ("sf", C.c_uint8), ("implicit", C.c_uint8), ("cr", C.c_uint8), ("crc", C.c_uint8),
                ("reduced_rate", C.c_uint8), ("disable_drift_correction", C.c_uint8), ("reserved0", C.c_uint8 * 2),
                ("device", C.c_int32), ("demod", C.c_int32), ("flags", C.c_uint32),
                ("segment_symbols", C.c_uint32), ("batch_items", C.c_uint32)]


class FrameInfo(C.Structure):
    _fields_ = [("stream", C.c_uint32), ("length", C.c_uint32), ("header_pos", C.c_int64), ("end_pos", C.c_int64)]


class Step(C.Structure):
    _fields_ = [("state", C.c_int32), ("consumed", C.c_int32), ("pos", C.c_int64), ("bin", C.c_int32),
                ("fine", C.c_int32), ("value", C.c_float), ("stream", C.c_uint32), ("cycles", C.c_uint32), ("reserved", C.c_uint32)]


class Timing(C.Structure):
    _fields_ = [("walker_ms", C.c_float), ("total_device_ms", C.c_float), ("walker_launches", C.c_uint32),
                ("jobs", C.c_uint32), ("probes", C.c_uint32), ("slow_path_relaunches", C.c_uint32),
                ("items", C.c_uint64)]


class FrameCheck(C.Structure):
    _fields_ = [("has_header", C.c_uint8), ("header_checksum_ok", C.c_uint8), ("has_crc", C.c_uint8), ("crc_ok", C.c_uint8),
                ("header_checksum_rx", C.c_uint8), ("header_checksum_calc", C.c_uint8), ("crc_rx", C.c_uint16), ("crc_calc", C.c_uint16),
                ("reserved", C.c_uint16)]


class StreamInfo(C.Structure):
    _fields_ = [("batch_items", C.c_uint64), ("buffered_items", C.c_uint64), ("passes", C.c_uint64), ("passes_by_latency", C.c_uint64),
                ("consumed_base", C.c_int64), ("max_latency_ms", C.c_float), ("pass_in_flight", C.c_uint32),
                ("resume_pos", C.c_int64), ("resume_cr", C.c_uint32), ("reserved", C.c_uint32)]   # (lora_hip_stream_info_ex)


class WindowStats(C.Structure):
    _fields_ = [("bin_down", C.c_int32), ("peak_down", C.c_float), ("total_down", C.c_float), ("bin_up", C.c_int32), ("peak_up", C.c_float), ("total_up", C.c_float)]


class Preamble(C.Structure):
    _fields_ = [("header_pos", C.c_int64), ("run_pos", C.c_int64), ("stream", C.c_uint32), ("run_len", C.c_uint32), ("bin", C.c_int32), ("sfd_index", C.c_int32),
                ("pmr", C.c_float), ("cfo_bins", C.c_float), ("cfo_hz", C.c_float), ("delta", C.c_int32)]


class SoftReport(C.Structure):
    _fields_ = [("status", C.c_uint32), ("cr", C.c_uint32), ("payload_length", C.c_uint32), ("payload_symbols", C.c_uint32),
                ("header_checksum_ok", C.c_uint8), ("has_crc", C.c_uint8), ("crc_ok", C.c_uint8), ("reserved", C.c_uint8),
                ("codewords", C.c_uint32), ("changed", C.c_uint32), ("min_margin", C.c_float), ("mean_abs_llr", C.c_float)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _t in self._fields_ if k != "reserved"}


class SoftRepair(C.Structure):
    _fields_ = [("status", C.c_uint32), ("candidates", C.c_uint32), ("pattern", C.c_uint32), ("changed", C.c_uint32), ("syndrome", C.c_uint16),
                ("reserved", C.c_uint16), ("penalty", C.c_float), ("codeword", C.c_uint16 * 8)]

    def as_dict(self) -> dict:
        """the keys of softdecode.crc_repair's record; codewords: the candidates' body codeword indices, candidate 0 first"""
        return dict(status=self.status, candidates=self.candidates, pattern=self.pattern, changed=self.changed, syndrome=self.syndrome,
                    penalty=np.float32(self.penalty), codewords=list(self.codeword[: self.candidates]))


class GatewayConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("filterbank", FilterBankConfig), ("decoders", C.POINTER(Config)), ("n_decoders", C.c_uint32),
                ("flags", C.c_uint32)]


class GatewayFrameInfo(C.Structure):
    _fields_ = [("row", C.c_uint32), ("grid_index", C.c_int32), ("sf", C.c_uint32), ("decoder", C.c_uint32), ("length", C.c_uint32),
                ("reserved", C.c_uint32), ("header_pos", C.c_int64), ("end_pos", C.c_int64)]


class GatewayStats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_decoders", C.c_uint32), ("passes", C.c_uint64 * GATEWAY_MAX_DECODERS),
                ("passes_by_latency", C.c_uint64 * GATEWAY_MAX_DECODERS), ("filterbank_calls", C.c_uint64), ("filterbank_ms", C.c_double),
                ("items_in", C.c_uint64), ("step_outputs", C.c_uint64)]


TX_FRAME_HDR_NIBBLES, TX_FRAME_CRC_BYTES = 1, 2  # lora_hip_tx_frame_t.flags (include/lora_hip_tx.h)
TX_MAX_SHIFTS = 2048                             # include/lora_hip_tx.h


class TxFrame(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("bandwidth", C.c_uint32), ("sf", C.c_uint8), ("implicit", C.c_uint8), ("cr", C.c_uint8),
                ("crc", C.c_uint8), ("reduced_rate", C.c_uint8), ("reserved0", C.c_uint8 * 3), ("preamble_len", C.c_uint32),
                ("sync_shifts", C.c_int32 * 2), ("flags", C.c_uint32), ("hdr_nibbles", C.c_uint8 * 2), ("crc_bytes", C.c_uint8 * 2),
                ("start", C.c_int64), ("freq_hz", C.c_double), ("amplitude", C.c_float), ("length", C.c_uint32),
                ("payload", C.POINTER(C.c_uint8))]


class TxConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("samp_rate", C.c_double), ("noise_sigma", C.c_double),
                ("seed", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


LINK_FLAG_PREAMBLE, LINK_FLAG_SYNC, LINK_FLAG_SFD = 1, 2, 4  # lora_hip_link_metrics_t.flags (include/lora_hip_link.h)


class LinkWindow(C.Structure):
    _fields_ = [("peak_bin", C.c_int32), ("frac", C.c_float), ("lobe_power", C.c_float), ("total_power", C.c_float), ("peak_power", C.c_float),
                ("valid", C.c_uint32)]


class LinkMetrics(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("reserved0", C.c_uint32), ("signal_power", C.c_double), ("noise_power", C.c_double),
                ("rssi_dbfs", C.c_double), ("snr_db", C.c_double), ("cfo_bins", C.c_double), ("cfo_hz", C.c_double),
                ("timing_samples", C.c_double), ("sync_shift", C.c_int32 * 2), ("reserved", C.c_uint64)]

    def as_dict(self) -> dict:
        d = {k: getattr(self, k) for k in ("flags", "signal_power", "noise_power", "rssi_dbfs", "snr_db", "cfo_bins", "cfo_hz", "timing_samples")}
        d["sync_shift"] = [int(self.sync_shift[0]), int(self.sync_shift[1])]
        return d


class LinkRequest(C.Structure):
    _fields_ = [("stream", C.c_uint32), ("reserved", C.c_uint32), ("header_pos", C.c_int64)]


class LoraHipError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__("lora_hip status %d: %s" % (status, msg))
        self.status = status


_lib = None


def load():
    """Loads liblora_hip.so; raises if it was not built (run __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: torch bundles its own libamdhip64.so (SONAME
    # libamdhip64.so.7).  Importing torch first makes the dynamic loader bind this
    # library to that same runtime; loading /opt/rocm's copy beside it leaves one
    # of the two without devices.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError("liblora_hip.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.lora_hip_abi_version.restype = C.c_uint32
    L.lora_hip_strerror.restype = C.c_char_p
    L.lora_hip_strerror.argtypes = [C.c_int]
    L.lora_hip_last_error.restype = C.c_char_p
    L.lora_hip_last_error.argtypes = [vp]
    L.lora_hip_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.lora_hip_destroy.argtypes = [vp]
    L.lora_hip_destroy.restype = None
    L.lora_hip_get_geometry.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.lora_hip_set_sf.argtypes = [vp, C.c_uint8]
    L.lora_hip_set_samp_rate.argtypes = [vp, C.c_float]
    L.lora_hip_work.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lora_hip_flush.argtypes = [vp]
    L.lora_hip_decode_device.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_uint32, vp]
    L.lora_hip_frames_available.restype = C.c_size_t
    L.lora_hip_frames_available.argtypes = [vp]
    L.lora_hip_poll_frame.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(FrameInfo)]
    L.lora_hip_drain_frames.argtypes = [vp, vp, C.c_size_t, C.POINTER(FrameInfo), C.c_size_t, C.POINTER(C.c_size_t)]
    L.lora_hip_drain_slots.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lora_hip_demod_symbols_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_int, vp, vp]
    L.lora_hip_demod_symbols_ex_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_int, vp, vp, vp]
    L.lora_hip_last_timing.argtypes = [vp, C.POINTER(Timing)]
    L.lora_hip_last_plan.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    if hasattr(L, "lora_hip_last_sync_stops") or not os.environ.get("LORA_HIP_LIB"):   # (a library variant of an older ABI under tools/ab.sh does without)
        L.lora_hip_last_sync_stops.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.lora_hip_last_payload_pass.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
    L.lora_hip_decode_device_begin.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_uint32, vp, C.c_uint32]
    L.lora_hip_decode_device_end.argtypes = [vp]
    L.lora_hip_decode_device_prepass.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_uint32, vp, C.c_uint32]
    L.lora_hip_gap_starts_device.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_uint32, vp, C.c_size_t, vp, vp]
    L.lora_hip_trace.restype = C.c_size_t
    L.lora_hip_trace.argtypes = [vp, C.POINTER(C.POINTER(Step))]
    L.lora_hip_trace_clear.argtypes = [vp]
    L.lora_hip_trace_clear.restype = None
    L.lora_hip_estimate_cfo_device.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_int64), C.c_size_t, C.c_int, C.POINTER(C.c_float), vp]
    L.lora_hip_estimate_cfo_device.restype = C.c_int
    L.lora_hip_ref_ifreq_device.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_float), vp]
    L.lora_hip_ref_ifreq_device.restype = C.c_int
    if hasattr(L, "lora_hip_get_table") or not os.environ.get("LORA_HIP_LIB"):   # (a library variant of an older ABI under tools/ab.sh does without)
        L.lora_hip_get_table.argtypes = [vp, C.c_int, C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_size_t)]
        L.lora_hip_get_table.restype = C.c_int
    L.lora_hip_window_stats_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(WindowStats), vp]
    L.lora_hip_detect_preambles_device.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_uint32, C.c_float, C.POINTER(Preamble), C.c_size_t, C.POINTER(C.c_size_t), vp]
    L.lora_hip_decode_at_headers_device.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_uint32, C.POINTER(Preamble), C.c_size_t, vp]
    L.lora_hip_walker_kernel_name.argtypes = [vp]
    L.lora_hip_walker_kernel_name.restype = C.c_char_p
    L.lora_hip_mux_create.argtypes = [C.POINTER(Config), C.c_uint32, C.POINTER(vp)]
    L.lora_hip_mux_destroy.argtypes = [vp]
    L.lora_hip_mux_destroy.restype = None
    L.lora_hip_mux_work.argtypes = [vp, C.c_uint32, vp, C.c_size_t]
    L.lora_hip_mux_flush.argtypes = [vp]
    L.lora_hip_mux_set_latency.argtypes = [vp, C.c_float]
    L.lora_hip_mux_set_max_ahead.argtypes = [vp, C.c_size_t]
    L.lora_hip_mux_frames_available.argtypes = [vp]
    L.lora_hip_mux_frames_available.restype = C.c_size_t
    L.lora_hip_mux_poll_frame.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(FrameInfo)]
    L.lora_hip_mux_passes.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.lora_hip_mux_last_error.argtypes = [vp]
    L.lora_hip_mux_last_error.restype = C.c_char_p
    L.lora_hip_set_stream_latency.argtypes = [vp, C.c_float]
    L.lora_hip_stream_info.argtypes = [vp, C.POINTER(StreamInfo)]
    if hasattr(L, "lora_hip_stream_info_ex") or not os.environ.get("LORA_HIP_LIB"):   # (a library variant of an older ABI under tools/ab.sh does without)
        L.lora_hip_stream_info_ex.argtypes = [vp, C.POINTER(StreamInfo), C.c_uint32]
    L.lora_hip_check_frame.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(FrameCheck)]
    L.lora_hip_check_frame.restype = C.c_int
    L.lora_hip_channelizer_create.argtypes = [C.POINTER(ChannelizerConfig), C.POINTER(vp)]
    L.lora_hip_channelizer_destroy.argtypes = [vp]
    L.lora_hip_channelizer_destroy.restype = None
    L.lora_hip_channelizer_last_error.argtypes = [vp]
    L.lora_hip_channelizer_last_error.restype = C.c_char_p
    L.lora_hip_channelizer_taps.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lora_hip_channelizer_output_items.argtypes = [vp, C.c_size_t]
    L.lora_hip_channelizer_output_items.restype = C.c_size_t
    L.lora_hip_channelizer_run_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t), vp]
    L.lora_hip_channelizer_work.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lora_hip_channelizer_apply_cfo.argtypes = [vp, C.c_float]
    L.lora_hip_channelizer_last_kernel_ms.argtypes = [vp]
    L.lora_hip_channelizer_last_kernel_ms.restype = C.c_float
    L.lora_hip_filterbank_create.argtypes = [C.POINTER(FilterBankConfig), C.POINTER(vp)]
    L.lora_hip_filterbank_destroy.argtypes = [vp]
    L.lora_hip_filterbank_destroy.restype = None
    L.lora_hip_filterbank_last_error.argtypes = [vp]
    L.lora_hip_filterbank_last_error.restype = C.c_char_p
    L.lora_hip_filterbank_taps.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lora_hip_filterbank_output_items.argtypes = [vp, C.c_size_t]
    L.lora_hip_filterbank_output_items.restype = C.c_size_t
    L.lora_hip_filterbank_run_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t), vp]
    L.lora_hip_filterbank_work.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lora_hip_filterbank_last_kernel_ms.argtypes = [vp]
    L.lora_hip_filterbank_last_kernel_ms.restype = C.c_float
    if hasattr(L, "lora_hip_filterbank_get_plan") or not os.environ.get("LORA_HIP_LIB"):   # (as above: an older library variant does without)
        L.lora_hip_filterbank_get_plan.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_size_t)]
    L.lora_hip_filterbank_run_device_rows.argtypes = [vp, vp, C.c_size_t, C.POINTER(vp), C.c_uint32, C.c_size_t, C.POINTER(C.c_size_t), vp]
    L.lora_hip_gateway_create.argtypes = [C.POINTER(GatewayConfig), C.POINTER(vp)]
    L.lora_hip_gateway_destroy.argtypes = [vp]
    L.lora_hip_gateway_destroy.restype = None
    L.lora_hip_gateway_last_error.argtypes = [vp]
    L.lora_hip_gateway_last_error.restype = C.c_char_p
    L.lora_hip_gateway_work.argtypes = [vp, vp, C.c_size_t]
    L.lora_hip_gateway_work_device.argtypes = [vp, vp, C.c_size_t, vp]
    L.lora_hip_gateway_flush.argtypes = [vp]
    L.lora_hip_gateway_set_latency.argtypes = [vp, C.c_float]
    L.lora_hip_gateway_frames_available.argtypes = [vp]
    L.lora_hip_gateway_frames_available.restype = C.c_size_t
    L.lora_hip_gateway_poll_frame.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(GatewayFrameInfo)]
    L.lora_hip_gateway_stats.argtypes = [vp, C.POINTER(GatewayStats)]
    if hasattr(L, "lora_hip_work_raw") or not os.environ.get("LORA_HIP_LIB"):   # (as above: an older library variant does without)
        L.lora_hip_iq_item_bytes.argtypes = [C.c_int]
        L.lora_hip_iq_item_bytes.restype = C.c_size_t
        L.lora_hip_iq_unpack_device.argtypes = [C.c_int, vp, C.c_size_t, C.c_int, C.c_float, vp, vp]
        L.lora_hip_work_raw.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_float, C.POINTER(C.c_size_t)]
        L.lora_hip_channelizer_run_device_raw.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_float, vp, C.c_size_t, C.POINTER(C.c_size_t), vp]
        L.lora_hip_channelizer_work_raw.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_float, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.lora_hip_filterbank_run_device_raw.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_float, vp, C.c_size_t, C.POINTER(C.c_size_t), vp]
        L.lora_hip_filterbank_run_device_rows_raw.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_float, C.POINTER(vp), C.c_uint32, C.c_size_t, C.POINTER(C.c_size_t), vp]
        L.lora_hip_filterbank_work_raw.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_float, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.lora_hip_gateway_work_raw.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_float]
        L.lora_hip_gateway_work_device_raw.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_float, vp]
    if hasattr(L, "lora_hip_tx_create") or not os.environ.get("LORA_HIP_LIB"):   # (as above)
        L.lora_hip_tx_encode.argtypes = [C.POINTER(TxFrame), C.POINTER(C.c_uint16), C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.lora_hip_tx_frame_items.argtypes = [C.POINTER(TxFrame), C.c_float, C.POINTER(C.c_uint64)]
        L.lora_hip_tx_create.argtypes = [C.POINTER(TxConfig), C.POINTER(vp)]
        L.lora_hip_tx_destroy.argtypes = [vp]
        L.lora_hip_tx_destroy.restype = None
        L.lora_hip_tx_last_error.argtypes = [vp]
        L.lora_hip_tx_last_error.restype = C.c_char_p
        L.lora_hip_tx_add_frames.argtypes = [vp, C.POINTER(TxFrame), C.c_size_t]
        L.lora_hip_tx_generate_device.argtypes = [vp, vp, C.c_size_t, vp]
        L.lora_hip_tx_generate_device_raw.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_double, vp]
        L.lora_hip_tx_generate.argtypes = [vp, vp, C.c_size_t]
        L.lora_hip_tx_position.argtypes = [vp]
        L.lora_hip_tx_position.restype = C.c_int64
        L.lora_hip_tx_pending.argtypes = [vp]
        L.lora_hip_tx_pending.restype = C.c_size_t
        L.lora_hip_tx_last_kernel_ms.argtypes = [vp]
        L.lora_hip_tx_last_kernel_ms.restype = C.c_float
    if hasattr(L, "lora_hip_link_enable") or not os.environ.get("LORA_HIP_LIB"):   # (as above)
        L.lora_hip_link_measure_device.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_uint32, C.POINTER(LinkRequest), C.c_size_t, C.POINTER(LinkMetrics),
                                                   C.POINTER(LinkWindow), vp]
        L.lora_hip_link_combine.argtypes = [C.POINTER(LinkWindow), C.c_uint32, C.c_uint32, C.c_double, C.POINTER(LinkMetrics)]
        L.lora_hip_link_enable.argtypes = [vp, C.c_int]
        L.lora_hip_link_poll_frame.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(FrameInfo), C.POINTER(LinkMetrics)]
        L.lora_hip_link_drain_frames.argtypes = [vp, vp, C.c_size_t, C.POINTER(FrameInfo), C.POINTER(LinkMetrics), C.c_size_t, C.POINTER(C.c_size_t)]
        L.lora_hip_link_mux_enable.argtypes = [vp, C.c_int]
        L.lora_hip_link_mux_poll_frame.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(FrameInfo), C.POINTER(LinkMetrics)]
        L.lora_hip_link_gateway_enable.argtypes = [vp, C.c_int]
        L.lora_hip_link_gateway_poll_frame.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(GatewayFrameInfo), C.POINTER(LinkMetrics)]
        L.lora_hip_link_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    if hasattr(L, "lora_hip_spectrum_create") or not os.environ.get("LORA_HIP_LIB"):   # (as above)
        u64p, szp = C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)
        L.lora_hip_spectrum_create.argtypes = [C.POINTER(SpectrumConfig), C.POINTER(vp)]
        L.lora_hip_spectrum_destroy.argtypes = [vp]
        L.lora_hip_spectrum_destroy.restype = None
        L.lora_hip_spectrum_last_error.argtypes = [vp]
        L.lora_hip_spectrum_last_error.restype = C.c_char_p
        L.lora_hip_spectrum_window.argtypes = [vp, vp, C.c_size_t, szp]
        L.lora_hip_spectrum_output_rows.argtypes = [vp, C.c_size_t]
        L.lora_hip_spectrum_output_rows.restype = C.c_size_t
        L.lora_hip_spectrum_run_device.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, C.c_size_t, C.c_size_t, szp, u64p, vp]
        L.lora_hip_spectrum_run_device_raw.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_float, vp, vp, vp, C.c_size_t, C.c_size_t, szp, u64p, vp]
        L.lora_hip_spectrum_work.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, C.c_size_t, C.c_size_t, szp, u64p]
        L.lora_hip_spectrum_work_raw.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_float, vp, vp, vp, C.c_size_t, C.c_size_t, szp, u64p]
        L.lora_hip_spectrum_reset.argtypes = [vp]
        L.lora_hip_spectrum_last_kernel_ms.argtypes = [vp]
        L.lora_hip_spectrum_last_kernel_ms.restype = C.c_float
    if hasattr(L, "lora_hip_resampler_create") or not os.environ.get("LORA_HIP_LIB"):   # (as above)
        u32p, u64p, szp = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)
        L.lora_hip_resampler_create.argtypes = [C.POINTER(ResamplerConfig), C.POINTER(vp)]
        L.lora_hip_resampler_destroy.argtypes = [vp]
        L.lora_hip_resampler_destroy.restype = None
        L.lora_hip_resampler_last_error.argtypes = [vp]
        L.lora_hip_resampler_last_error.restype = C.c_char_p
        L.lora_hip_resampler_taps.argtypes = [vp, vp, C.c_size_t, szp]
        L.lora_hip_resampler_ratio.argtypes = [vp, u32p, u32p, u32p]
        L.lora_hip_resampler_delay.argtypes = [vp]
        L.lora_hip_resampler_delay.restype = C.c_double
        L.lora_hip_resampler_get_plan.argtypes = [vp, u32p, u32p, u32p, szp]
        L.lora_hip_resampler_output_items.argtypes = [vp, C.c_size_t]
        L.lora_hip_resampler_output_items.restype = C.c_size_t
        L.lora_hip_resampler_run_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, szp, u64p, vp]
        L.lora_hip_resampler_run_device_raw.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_float, vp, C.c_size_t, szp, u64p, vp]
        L.lora_hip_resampler_work.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, szp, u64p]
        L.lora_hip_resampler_work_raw.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_float, vp, C.c_size_t, szp, u64p]
        L.lora_hip_resampler_reset.argtypes = [vp]
        L.lora_hip_resampler_last_kernel_ms.argtypes = [vp]
        L.lora_hip_resampler_last_kernel_ms.restype = C.c_float
    if hasattr(L, "lora_hip_conditioner_create") or not os.environ.get("LORA_HIP_LIB"):   # (as above)
        u32p, u64p, szp = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)
        L.lora_hip_conditioner_create.argtypes = [C.POINTER(ConditionerConfig), C.POINTER(vp)]
        L.lora_hip_conditioner_destroy.argtypes = [vp]
        L.lora_hip_conditioner_destroy.restype = None
        L.lora_hip_conditioner_last_error.argtypes = [vp]
        L.lora_hip_conditioner_last_error.restype = C.c_char_p
        L.lora_hip_conditioner_output_items.argtypes = [vp, C.c_size_t]
        L.lora_hip_conditioner_output_items.restype = C.c_size_t
        L.lora_hip_conditioner_get_plan.argtypes = [vp, u32p, u32p, u32p, u32p]
        L.lora_hip_conditioner_run_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, szp, u64p, vp]
        L.lora_hip_conditioner_run_device_raw.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_float, vp, C.c_size_t, szp, u64p, vp]
        L.lora_hip_conditioner_work.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, szp, u64p]
        L.lora_hip_conditioner_work_raw.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_float, vp, C.c_size_t, szp, u64p]
        L.lora_hip_conditioner_flush_device.argtypes = [vp, vp, C.c_size_t, szp, u64p, vp]
        L.lora_hip_conditioner_flush.argtypes = [vp, vp, C.c_size_t, szp, u64p]
        L.lora_hip_conditioner_reset.argtypes = [vp]
        L.lora_hip_conditioner_set_fixed.argtypes = [vp, C.c_float, C.c_float, C.c_float, C.c_float]
        L.lora_hip_conditioner_set_adaptive.argtypes = [vp]
        L.lora_hip_conditioner_block_records.argtypes = [vp, vp, vp, C.c_size_t, szp, vp, vp]
        L.lora_hip_conditioner_last_kernel_ms.argtypes = [vp]
        L.lora_hip_conditioner_last_kernel_ms.restype = C.c_float
    if hasattr(L, "lora_hip_soft_symbols_device") or not os.environ.get("LORA_HIP_LIB"):   # (as above)
        L.lora_hip_soft_symbols_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, vp, vp, vp, vp]
        L.lora_hip_soft_decode_at_headers_device.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_uint32, C.POINTER(Preamble), C.c_size_t, C.c_uint32,
                                                             C.POINTER(SoftReport), vp]
    if hasattr(L, "lora_hip_soft_crc_repair_enable") or not os.environ.get("LORA_HIP_LIB"):   # (as above)
        L.lora_hip_soft_crc_repair_enable.argtypes = [vp, C.c_uint32]
        L.lora_hip_soft_crc_repair_results.argtypes = [vp, C.POINTER(SoftRepair), C.c_size_t]
        L.lora_hip_soft_crc_repair_codewords.argtypes = [vp, C.c_size_t, vp, vp, vp, vp, C.c_uint32, vp, C.POINTER(SoftRepair), vp]
    _lib = L
    return L


def _raw_items(raw, fmt=None):
    """(contiguous component array, format, item count) of integer IQ given flat interleaved or shaped (n, 2)."""
    from . import iqformat
    return iqformat.as_components(raw, fmt)


def unpack_device(d_raw: int, n_items: int, fmt: int, d_out: int, scale: float = 0.0, device: int = 0, stream: int = 0):
    """lora_hip_iq_unpack_device: n_items items of format fmt at device address d_raw -> complex64 at d_out (no handle)."""
    L = load()
    st = L.lora_hip_iq_unpack_device(int(device), d_raw, int(n_items), int(fmt), float(scale), d_out, stream)
    if st != 0:
        raise LoraHipError(st, "lora_hip_iq_unpack_device: %s" % L.lora_hip_strerror(st).decode())


def check_frame(blob: bytes) -> FrameCheck:
    """Header checksum and payload CRC of a published frame blob (lora_hip_check_frame: host only, no GPU needed)."""
    out = FrameCheck()
    st = load().lora_hip_check_frame(bytes(blob), len(blob), C.byref(out))
    if st != 0:
        raise LoraHipError(st, "lora_hip_check_frame: blob too short")
    return out


class Handle:
    """Thin RAII wrapper of lora_hip_decoder_t."""

    def __init__(self, samp_rate=1e6, bandwidth=125000, sf=7, implicit=False, cr=4, crc=True, reduced_rate=False,
                 disable_drift_correction=False, device=0, demod=DEMOD_FFT_COMPAT, flags=0, segment_symbols=0,
                 batch_items=0):
        self.L = load()
        cfg = Config(struct_size=C.sizeof(Config), samp_rate=float(samp_rate), bandwidth=int(bandwidth), sf=int(sf),
                     implicit=int(bool(implicit)), cr=int(cr), crc=int(bool(crc)), reduced_rate=int(bool(reduced_rate)),
                     disable_drift_correction=int(bool(disable_drift_correction)), device=int(device), demod=int(demod),
                     flags=int(flags), segment_symbols=int(segment_symbols), batch_items=int(batch_items))
        h = C.c_void_p()
        st = self.L.lora_hip_create(C.byref(cfg), C.byref(h))
        if st != 0:
            raise LoraHipError(st, "%s (%s)" % (self.L.lora_hip_strerror(st).decode(), self.L.lora_hip_last_error(None).decode()))
        self.h = h
        a, b, d = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self.L.lora_hip_get_geometry(self.h, C.byref(a), C.byref(b), C.byref(d))
        self.sps, self.nbins, self.decim = a.value, b.value, d.value
        self.device, self.batch_items = int(device), int(batch_items)
        self.reduced_rate = bool(reduced_rate)

    def close(self):
        if getattr(self, "h", None):
            self.L.lora_hip_destroy(self.h)
            self.h = None

    __del__ = close

    def _check(self, st: int):
        if st != 0:
            raise LoraHipError(st, "%s (%s)" % (self.L.lora_hip_strerror(st).decode(), self.L.lora_hip_last_error(self.h).decode()))

    # streaming (host buffers)
    def work(self, iq: np.ndarray) -> int:
        a = np.ascontiguousarray(iq, dtype=np.complex64)
        n = C.c_size_t(0)
        self._check(self.L.lora_hip_work(self.h, a.ctypes.data, a.size, C.byref(n)))
        return n.value

    def work_raw(self, raw, fmt=None, scale: float = 0.0) -> int:
        """lora_hip_work_raw: integer items (int16 / int8 / uint8, flat interleaved or (n, 2)); fmt None: from the dtype."""
        a, f, n_items = _raw_items(raw, fmt)
        n = C.c_size_t(0)
        self._check(self.L.lora_hip_work_raw(self.h, a.ctypes.data, n_items, f, float(scale), C.byref(n)))
        return n.value

    def flush(self):
        self._check(self.L.lora_hip_flush(self.h))

    def kernel_name(self) -> str:
        """lora_hip_walker_kernel_name: the state-machine kernel this handle's passes launch."""
        return self.L.lora_hip_walker_kernel_name(self.h).decode()

    def set_stream_latency(self, max_latency_ms: float):
        """lora_hip_set_stream_latency: wall-clock bound on how long a delivered sample waits for a device pass (0 = off)."""
        self._check(self.L.lora_hip_set_stream_latency(self.h, float(max_latency_ms)))

    def stream_info(self) -> StreamInfo:
        """lora_hip_stream_info_ex: with resume_pos / resume_cr, the serial decoder's state behind the last collected pass."""
        out = StreamInfo()
        if hasattr(self.L, "lora_hip_stream_info_ex"):
            self._check(self.L.lora_hip_stream_info_ex(self.h, C.byref(out), C.sizeof(StreamInfo)))
        else:
            self._check(self.L.lora_hip_stream_info(self.h, C.byref(out)))
        return out

    # batched, device-resident
    def decode_device(self, dev_ptr: int, total_items: int, offs: Sequence[int], lens: Sequence[int], stream: int = 0):
        o = np.ascontiguousarray(offs, dtype=np.uint64)
        l = np.ascontiguousarray(lens, dtype=np.uint64)
        self._check(self.L.lora_hip_decode_device(self.h, dev_ptr, total_items, o.ctypes.data, l.ctypes.data, o.size, stream))

    def decode_device_begin(self, dev_ptr: int, total_items: int, offs: Sequence[int], lens: Sequence[int], stream: int = 0, iq_ready: bool = False):
        """First half of a pass (plan + main launch); finish it with decode_device_end().  iq_ready: LORA_HIP_BEGIN_IQ_READY."""
        o = np.ascontiguousarray(offs, dtype=np.uint64)
        l = np.ascontiguousarray(lens, dtype=np.uint64)
        self._check(self.L.lora_hip_decode_device_begin(self.h, dev_ptr, total_items, o.ctypes.data, l.ctypes.data, o.size, stream, 1 if iq_ready else 0))

    def decode_device_prepass(self, dev_ptr: int, total_items: int, offs: Sequence[int], lens: Sequence[int], stream: int = 0, iq_ready: bool = False):
        """Issues the envelope pre-pass of the pass that will be begun next on this handle (lora_hip_decode_device_prepass)."""
        o = np.ascontiguousarray(offs, dtype=np.uint64)
        l = np.ascontiguousarray(lens, dtype=np.uint64)
        self._check(self.L.lora_hip_decode_device_prepass(self.h, dev_ptr, total_items, o.ctypes.data, l.ctypes.data, o.size, stream, 1 if iq_ready else 0))

    def decode_device_end(self):
        self._check(self.L.lora_hip_decode_device_end(self.h))

    def gap_starts_device(self, dev_ptr: int, total_items: int, offs: Sequence[int], lens: Sequence[int], stream: int = 0):
        """Per stream, the item positions where the envelope pre-pass sees a gap begin (lora_hip_gap_starts_device)."""
        o = np.ascontiguousarray(offs, dtype=np.uint64)
        l = np.ascontiguousarray(lens, dtype=np.uint64)
        cap = int(sum(int(x) for x in l) // 64 + 16)
        pos = np.zeros(cap, dtype=np.int64)
        cnt = np.zeros(o.size, dtype=np.uint32)
        self._check(self.L.lora_hip_gap_starts_device(self.h, dev_ptr, total_items, o.ctypes.data, l.ctypes.data, o.size, pos.ctypes.data, cap,
                                                      cnt.ctypes.data, stream))
        out, k = [], 0
        for c in cnt:
            out.append(pos[k:k + int(c)].copy()); k += int(c)
        return out

    def demod_symbols_device(self, dev_ptr: int, total_items: int, offsets: Sequence[int], demod: int, stream: int = 0) -> np.ndarray:
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        out = np.zeros(off.size, dtype=np.uint32)
        self._check(self.L.lora_hip_demod_symbols_device(self.h, dev_ptr, total_items, off.ctypes.data, off.size, demod, out.ctypes.data, stream))
        return out

    def demod_symbols_ex_device(self, dev_ptr: int, total_items: int, offsets: Sequence[int], demod: int, stream: int = 0):
        """(shifts, fine): get_shift_fft's value and d_fine_sync after the per-symbol fine_sync, per window."""
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        out = np.zeros(off.size, dtype=np.uint32)
        fine = np.zeros(off.size, dtype=np.int32)
        self._check(self.L.lora_hip_demod_symbols_ex_device(self.h, dev_ptr, total_items, off.ctypes.data, off.size, demod, out.ctypes.data,
                                                            fine.ctypes.data, stream))
        return out, fine

    def estimate_cfo_device(self, dev_ptr: int, total_items: int, offsets: Sequence[int], mode: int = 1, stream: int = 0) -> np.ndarray:
        """CFO in Hz of the windows at `offsets` (experimental_determine_cfo, decoder_impl.cc:730-738; mode 1: mean over the window)."""
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        out = np.zeros(off.size, dtype=np.float32)
        self._check(self.L.lora_hip_estimate_cfo_device(self.h, C.c_void_p(dev_ptr), total_items, off.ctypes.data_as(C.POINTER(C.c_int64)), off.size, mode,
                                                        out.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(stream)))
        return out

    def ref_ifreq_device(self, dev_ptr: int, n_items: int, stream: int = 0):
        """(atan2f of every item, instantaneous_frequency of every pair) as the strict SYNC path computes them (decoder_impl.cc:231-240)."""
        arg = np.zeros(n_items, dtype=np.float32)
        f = np.zeros(n_items - 1, dtype=np.float32)
        self._check(self.L.lora_hip_ref_ifreq_device(self.h, C.c_void_p(dev_ptr), n_items, arg.ctypes.data_as(C.POINTER(C.c_float)),
                                                     f.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(stream)))
        return arg, f

    def window_stats_device(self, dev_ptr: int, total_items: int, offsets: Sequence[int], stream: int = 0):
        """lora_hip_window_stats_device: per window (bin_down, peak_down, total_down, bin_up, peak_up, total_up)."""
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        out = (WindowStats * max(off.size, 1))()
        self._check(self.L.lora_hip_window_stats_device(self.h, dev_ptr, total_items, off.ctypes.data, off.size, out, stream))
        return [(o.bin_down, o.peak_down, o.total_down, o.bin_up, o.peak_up, o.total_up) for o in out[: off.size]]

    def detect_preambles_device(self, dev_ptr: int, total_items: int, offs: Sequence[int], lens: Sequence[int], threshold: float = 0.0, stream: int = 0, cap: int = 4096):
        """lora_hip_detect_preambles_device: FFT-domain preamble detection (acquires below 0 dB); list of dicts."""
        o = np.ascontiguousarray(offs, dtype=np.uint64)
        l = np.ascontiguousarray(lens, dtype=np.uint64)
        out = (Preamble * cap)()
        n = C.c_size_t(0)
        self._check(self.L.lora_hip_detect_preambles_device(self.h, dev_ptr, total_items, o.ctypes.data, l.ctypes.data, o.size, float(threshold), out, cap, C.byref(n), stream))
        return [dict(header_pos=p.header_pos, run_pos=p.run_pos, stream=p.stream, run_len=p.run_len, bin=p.bin, sfd_index=p.sfd_index, pmr=p.pmr,
                     cfo_bins=p.cfo_bins, cfo_hz=p.cfo_hz, delta=p.delta) for p in out[: n.value]]

    def decode_at_headers_device(self, dev_ptr: int, total_items: int, offs: Sequence[int], lens: Sequence[int], preambles, stream: int = 0):
        """lora_hip_decode_at_headers_device: decodes the packets at the detector's header positions (dicts of detect_preambles_device, or
        (stream, header_pos) pairs); frames go to the handle's queue."""
        o = np.ascontiguousarray(offs, dtype=np.uint64)
        l = np.ascontiguousarray(lens, dtype=np.uint64)
        arr = (Preamble * max(len(preambles), 1))()
        for i, p in enumerate(preambles):
            st, hp = (p["stream"], p["header_pos"]) if isinstance(p, dict) else p
            arr[i].stream, arr[i].header_pos = int(st), int(hp)
        self._check(self.L.lora_hip_decode_at_headers_device(self.h, dev_ptr, total_items, o.ctypes.data, l.ctypes.data, o.size, arr, len(preambles), stream))

    def soft_symbols_device(self, dev_ptr: int, total_items: int, offsets: Sequence[int], reduced=None, stream: int = 0):
        """lora_hip_soft_symbols_device: (list of per-window LLR arrays - sf - 2 floats where reduced[i], else sf -, arg-max indices k, peak
        magnitudes).  reduced None: the handle's reduced_rate for every window."""
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        red = None if reduced is None else np.ascontiguousarray(np.asarray(reduced) != 0, dtype=np.uint8)
        if red is not None and red.size != off.size:
            raise ValueError("one reduced flag per window")
        llr = np.zeros(max(off.size, 1) * 12, dtype=np.float32)
        k = np.zeros(max(off.size, 1), dtype=np.int32)
        peak = np.zeros(max(off.size, 1), dtype=np.float32)
        self._check(self.L.lora_hip_soft_symbols_device(self.h, dev_ptr, total_items, off.ctypes.data, off.size, None if red is None else red.ctypes.data,
                                                        llr.ctypes.data, k.ctypes.data, peak.ctypes.data, stream))
        sf = int(self.nbins).bit_length() - 1
        out, at = [], 0
        for i in range(off.size):
            ppm = sf - 2 if (self.reduced_rate if red is None else red[i]) else sf
            out.append(llr[at:at + ppm].copy())
            at += ppm
        return out, k[: off.size], peak[: off.size]

    def soft_decode_at_headers_device(self, dev_ptr: int, total_items: int, offs: Sequence[int], lens: Sequence[int], preambles, flags: int = 0, stream: int = 0):
        """lora_hip_soft_decode_at_headers_device: decode_at_headers_device with soft decisions; frames go to the handle's queue (drain them as
        before), the per-entry reports come back as dicts."""
        o = np.ascontiguousarray(offs, dtype=np.uint64)
        l = np.ascontiguousarray(lens, dtype=np.uint64)
        arr = (Preamble * max(len(preambles), 1))()
        for i, p in enumerate(preambles):
            st, hp = (p["stream"], p["header_pos"]) if isinstance(p, dict) else p
            arr[i].stream, arr[i].header_pos = int(st), int(hp)
        rep = (SoftReport * max(len(preambles), 1))()
        self._check(self.L.lora_hip_soft_decode_at_headers_device(self.h, dev_ptr, total_items, o.ctypes.data, l.ctypes.data, o.size, arr, len(preambles), int(flags),
                                                                  rep, stream))
        self._soft_entries = len(preambles)
        return [r.as_dict() for r in rep[: len(preambles)]]

    def soft_crc_repair_enable(self, candidates: int):
        """lora_hip_soft_crc_repair_enable: 0 off (the default), 1 .. 8: CRC-aided repair with that many candidates in later soft_decode_at_headers_device calls"""
        if not 0 <= int(candidates) <= SOFT_REPAIR_MAX_CANDIDATES:
            raise ValueError("crc repair candidates: 0 .. %d, not %r" % (SOFT_REPAIR_MAX_CANDIDATES, candidates))
        self._check(self.L.lora_hip_soft_crc_repair_enable(self.h, int(candidates)))

    def soft_crc_repair_results(self) -> List[dict]:
        """lora_hip_soft_crc_repair_results: the repair records of the last soft_decode_at_headers_device call, one dict per entry"""
        n = getattr(self, "_soft_entries", 0)
        rec = (SoftRepair * max(n, 1))()
        self._check(self.L.lora_hip_soft_crc_repair_results(self.h, rec, n))
        return [r.as_dict() for r in rec[:n]]

    def soft_crc_repair_codewords(self, lengths: Sequence[int], nibbles, seconds, margins, candidates: int, stream: int = 0):
        """lora_hip_soft_crc_repair_codewords: the repair kernel alone.  lengths[f]: payload bytes in front of the CRC bytes; nibbles / seconds /
        margins: the 2 * (lengths[f] + 2) body codewords of every frame, back to back -> (list of repaired bodies, list of record dicts)"""
        ln = np.ascontiguousarray(lengths, dtype=np.uint32)
        nib, sec = np.ascontiguousarray(nibbles, dtype=np.uint8), np.ascontiguousarray(seconds, dtype=np.uint8)
        mar = np.ascontiguousarray(margins, dtype=np.float32)
        n_cw = int(2 * (ln.astype(np.int64) + 2).sum())
        if not (nib.size == sec.size == mar.size == n_cw):
            raise ValueError("2 * (length + 2) codewords per frame: %d expected" % n_cw)
        out = np.zeros(max(n_cw // 2, 1), dtype=np.uint8)
        rec = (SoftRepair * max(ln.size, 1))()
        self._check(self.L.lora_hip_soft_crc_repair_codewords(self.h, ln.size, ln.ctypes.data, nib.ctypes.data, sec.ctypes.data, mar.ctypes.data, int(candidates),
                                                              out.ctypes.data, rec, stream))
        bodies, at = [], 0
        for v in ln:
            bodies.append(bytes(out[at:at + int(v) + 2]))
            at += int(v) + 2
        return bodies, [r.as_dict() for r in rec[: ln.size]]

    def frames_available(self) -> int:
        return self.L.lora_hip_frames_available(self.h)

    def poll_frame(self) -> Optional[Tuple[bytes, FrameInfo]]:
        buf = (C.c_uint8 * 320)()
        n = C.c_size_t(0)
        info = FrameInfo()
        self._check(self.L.lora_hip_poll_frame(self.h, buf, 320, C.byref(n), C.byref(info)))
        if n.value == 0:
            return None
        return bytes(buf[: n.value]), info

    def drain(self) -> List[Tuple[bytes, FrameInfo]]:
        """All queued frames, through the bulk call (one ABI crossing per 1024 frames)."""
        out = []
        while True:
            n_avail = self.frames_available()
            if n_avail == 0:
                return out
            k = min(n_avail, 4096)
            buf = (C.c_uint8 * (k * 280))()
            infos = (FrameInfo * k)()
            n = C.c_size_t(0)
            self._check(self.L.lora_hip_drain_frames(self.h, buf, k * 280, infos, k, C.byref(n)))
            raw = bytes(buf)
            off = 0
            for i in range(n.value):
                ln = infos[i].length
                inf = FrameInfo(infos[i].stream, ln, infos[i].header_pos, infos[i].end_pos)
                out.append((raw[off:off + ln], inf))
                off += ln
            if n.value == 0:
                return out

    def enable_link(self, on: bool = True):
        """lora_hip_link_enable: every frame published from now on carries link metrics (drain_link)."""
        self._check(self.L.lora_hip_link_enable(self.h, int(bool(on))))

    def drain_link(self) -> List[Tuple[bytes, FrameInfo, "LinkMetrics"]]:
        """All queued frames with their link metrics (flags == 0: published while link metrics were off)."""
        out = []
        while True:
            k = min(self.frames_available(), 4096)
            if k == 0:
                return out
            buf = (C.c_uint8 * (k * 280))()
            infos, mets = (FrameInfo * k)(), (LinkMetrics * k)()
            n = C.c_size_t(0)
            self._check(self.L.lora_hip_link_drain_frames(self.h, buf, k * 280, infos, mets, k, C.byref(n)))
            raw, off = bytes(buf), 0
            for i in range(n.value):
                ln = infos[i].length
                out.append((raw[off:off + ln], FrameInfo(infos[i].stream, ln, infos[i].header_pos, infos[i].end_pos), LinkMetrics.from_buffer_copy(mets[i])))
                off += ln
            if n.value == 0:
                return out

    def poll_frame_link(self):
        buf = (C.c_uint8 * 320)()
        n, info, met = C.c_size_t(0), FrameInfo(), LinkMetrics()
        self._check(self.L.lora_hip_link_poll_frame(self.h, buf, 320, C.byref(n), C.byref(info), C.byref(met)))
        return None if n.value == 0 else (bytes(buf[: n.value]), info, met)

    def measure_link_device(self, dev_ptr: int, total_items: int, offs: Sequence[int], lens: Sequence[int], requests, stream: int = 0, windows: bool = False):
        """lora_hip_link_measure_device: requests = (stream, header_pos) pairs -> list of LinkMetrics (and, with windows, the
        6 * n LinkWindow records)."""
        o = np.ascontiguousarray(offs, dtype=np.uint64)
        l = np.ascontiguousarray(lens, dtype=np.uint64)
        n = len(requests)
        arr = (LinkRequest * max(n, 1))()
        for i, (st, hp) in enumerate(requests):
            arr[i].stream, arr[i].header_pos = int(st), int(hp)
        mets = (LinkMetrics * max(n, 1))()
        wins = (LinkWindow * max(6 * n, 1))() if windows else None
        self._check(self.L.lora_hip_link_measure_device(self.h, dev_ptr, total_items, o.ctypes.data, l.ctypes.data, o.size, arr, n, mets, wins, stream))
        m = [LinkMetrics.from_buffer_copy(mets[i]) for i in range(n)]
        return (m, [LinkWindow.from_buffer_copy(wins[i]) for i in range(6 * n)]) if windows else m

    def link_stats(self) -> dict:
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_double(0.0)
        self._check(self.L.lora_hip_link_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"launches": int(a.value), "frames": int(b.value), "kernel_ms": float(c.value)}

    INFO_DTYPE = np.dtype([("stream", "<u4"), ("length", "<u4"), ("header_pos", "<i8"), ("end_pos", "<i8")])

    def drain_raw(self):
        """All queued frames without per-frame Python objects: (blob bytes back to back as uint8[], infos as a
        structured array with fields stream / length / header_pos / end_pos)."""
        bufs, infos = [], []
        while True:
            n_avail = self.frames_available()
            if n_avail == 0:
                break
            k = min(n_avail, 8192)
            buf = np.empty(k * 280, dtype=np.uint8)
            inf = np.empty(k, dtype=self.INFO_DTYPE)
            n = C.c_size_t(0)
            self._check(self.L.lora_hip_drain_frames(self.h, buf.ctypes.data, buf.size, C.cast(inf.ctypes.data, C.POINTER(FrameInfo)), k, C.byref(n)))
            if n.value == 0:
                break
            inf = inf[: n.value]
            bufs.append(buf[: int(inf["length"].sum())])
            infos.append(inf)
        if not bufs:
            return np.empty(0, dtype=np.uint8), np.empty(0, dtype=self.INFO_DTYPE)
        return np.concatenate(bufs), np.concatenate(infos)

    def drain_slots(self, slot_bytes: int) -> np.ndarray:
        """All queued frames as fixed-size slots uint8[n, slot_bytes]: u32 stream | u32 length | i64 header_pos | blob | zeros."""
        n_avail = self.frames_available()
        out = np.empty((max(n_avail, 1), slot_bytes), dtype=np.uint8)
        n = C.c_size_t(0)
        self._check(self.L.lora_hip_drain_slots(self.h, out.ctypes.data, slot_bytes, n_avail, C.byref(n)))
        return out[: n.value]

    def timing(self) -> Timing:
        t = Timing()
        self._check(self.L.lora_hip_last_timing(self.h, C.byref(t)))
        return t

    def plan(self):
        """(burst_aware, segments) of the last pass: lora_hip_last_plan."""
        b, n = C.c_uint32(0), C.c_uint32(0)
        self._check(self.L.lora_hip_last_plan(self.h, C.byref(b), C.byref(n)))
        return bool(b.value), int(n.value)

    def sync_stops(self):
        """(tail_probes, at_sync) of the last pass's main launch: lora_hip_last_sync_stops."""
        t, s = C.c_uint32(0), C.c_uint32(0)
        self._check(self.L.lora_hip_last_sync_stops(self.h, C.byref(t), C.byref(s)))
        return int(t.value), int(s.value)

    def table(self, which: int) -> np.ndarray:
        """The handle's ideal-chirp table `which` (0 downchirp, 1 upchirp, 2 downchirp ifreq, 3 upchirp ifreq, 4 d_upchirp_ifreq_v + guard) as float32: lora_hip_get_table."""
        n = C.c_size_t()
        self._check(self.L.lora_hip_get_table(self.h, which, None, 0, C.byref(n)))
        out = np.empty(n.value, np.float32)
        self._check(self.L.lora_hip_get_table(self.h, which, out.ctypes.data_as(C.POINTER(C.c_float)), n.value, C.byref(n)))
        return out

    def payload_pass(self):
        """dict(packets, moved, rerun, rounds, symbols, ms) of the last pass's payload pass (all zero unless it ran decoupled): lora_hip_last_payload_pass."""
        a, mv, b, r, c, m = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_float(0)
        self._check(self.L.lora_hip_last_payload_pass(self.h, C.byref(a), C.byref(mv), C.byref(b), C.byref(r), C.byref(c), C.byref(m)))
        return dict(packets=int(a.value), moved=int(mv.value), rerun=int(b.value), rounds=int(r.value), symbols=int(c.value), ms=float(m.value))

    def trace(self):
        p = C.POINTER(Step)()
        n = self.L.lora_hip_trace(self.h, C.byref(p))
        return [(p[i].state, p[i].pos, p[i].consumed, p[i].bin, p[i].fine, p[i].value, p[i].stream, p[i].cycles) for i in range(n)]

    def trace_clear(self):
        self.L.lora_hip_trace_clear(self.h)


class Mux:
    """lora_hip_mux_*: n_channels independent decoders fed in any order, decoded by ONE device pass per chunk (the gateway flowgraph)."""

    def __init__(self, n_channels, samp_rate=1e6, bandwidth=125000, sf=7, implicit=False, cr=4, crc=True, reduced_rate=False,
                 disable_drift_correction=False, device=0, demod=DEMOD_FFT_COMPAT, flags=0, segment_symbols=0, batch_items=0):
        self.L = load()
        cfg = Config(struct_size=C.sizeof(Config), samp_rate=float(samp_rate), bandwidth=int(bandwidth), sf=int(sf), implicit=int(bool(implicit)), cr=int(cr),
                     crc=int(bool(crc)), reduced_rate=int(bool(reduced_rate)), disable_drift_correction=int(bool(disable_drift_correction)), device=int(device),
                     demod=int(demod), flags=int(flags), segment_symbols=int(segment_symbols), batch_items=int(batch_items))
        self.h = C.c_void_p()
        st = self.L.lora_hip_mux_create(C.byref(cfg), int(n_channels), C.byref(self.h))
        if st != 0:
            raise LoraHipError(st, "%s (%s)" % (self.L.lora_hip_strerror(st).decode(), self.L.lora_hip_last_error(None).decode()))
        self.n_channels = int(n_channels)

    def _check(self, st):
        if st != 0:
            raise LoraHipError(st, "%s (%s)" % (self.L.lora_hip_strerror(st).decode(), (self.L.lora_hip_mux_last_error(self.h) or b"").decode()))

    def work(self, channel: int, iq: np.ndarray):
        a = np.ascontiguousarray(iq, dtype=np.complex64)
        self._check(self.L.lora_hip_mux_work(self.h, int(channel), a.ctypes.data, a.size))

    def flush(self):
        self._check(self.L.lora_hip_mux_flush(self.h))

    def set_latency(self, ms: float):
        self._check(self.L.lora_hip_mux_set_latency(self.h, float(ms)))

    def set_max_ahead(self, items: int):
        self._check(self.L.lora_hip_mux_set_max_ahead(self.h, int(items)))

    def passes(self):
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(self.L.lora_hip_mux_passes(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def drain(self) -> List[Tuple[bytes, FrameInfo]]:
        out = []
        buf = (C.c_uint8 * 320)()
        while self.L.lora_hip_mux_frames_available(self.h):
            n = C.c_size_t(0)
            info = FrameInfo()
            self._check(self.L.lora_hip_mux_poll_frame(self.h, buf, 320, C.byref(n), C.byref(info)))
            out.append((bytes(buf[: n.value]), info))
        return out

    def enable_link(self, on: bool = True):
        self._check(self.L.lora_hip_link_mux_enable(self.h, int(bool(on))))

    def drain_link(self) -> List[Tuple[bytes, FrameInfo, "LinkMetrics"]]:
        out = []
        buf = (C.c_uint8 * 320)()
        while self.L.lora_hip_mux_frames_available(self.h):
            n, info, met = C.c_size_t(0), FrameInfo(), LinkMetrics()
            self._check(self.L.lora_hip_link_mux_poll_frame(self.h, buf, 320, C.byref(n), C.byref(info), C.byref(met)))
            out.append((bytes(buf[: n.value]), info, met))
        return out

    def close(self):
        if getattr(self, "h", None):
            self.L.lora_hip_mux_destroy(self.h)
            self.h = None

    __del__ = close


class Channelizer:
    """lora_hip_channelizer_* (include/lora_hip_channelizer.h): the frequency-translating FIR in front of the decoder."""

    def __init__(self, samp_rate, center_freq, channel_list, bandwidth, decimation=1, device=0, cutoff_hz=0.0, transition_hz=0.0, flags=0):
        self.L = load()
        self.n_channels = len(channel_list)
        self._chan = (C.c_float * self.n_channels)(*[float(c) for c in channel_list])
        cfg = ChannelizerConfig(struct_size=C.sizeof(ChannelizerConfig), samp_rate=float(samp_rate), center_freq=float(center_freq),
                                channel_list=self._chan, n_channels=self.n_channels, bandwidth=int(bandwidth), decimation=int(decimation), device=int(device),
                                cutoff_hz=float(cutoff_hz), transition_hz=float(transition_hz), flags=int(flags))
        self.h = C.c_void_p()
        st = self.L.lora_hip_channelizer_create(C.byref(cfg), C.byref(self.h))
        if st != 0:
            raise LoraHipError(st, self.L.lora_hip_strerror(st).decode())

    def _check(self, st):
        if st != 0:
            raise LoraHipError(st, (self.L.lora_hip_channelizer_last_error(self.h) or b"").decode() or self.L.lora_hip_strerror(st).decode())

    def taps(self) -> np.ndarray:
        n = C.c_size_t(0)
        self._check(self.L.lora_hip_channelizer_taps(self.h, None, 0, C.byref(n)))
        t = np.zeros(n.value, dtype=np.float32)
        self._check(self.L.lora_hip_channelizer_taps(self.h, t.ctypes.data, t.size, C.byref(n)))
        return t

    def output_items(self, n_in: int) -> int:
        return int(self.L.lora_hip_channelizer_output_items(self.h, n_in))

    def work(self, x) -> np.ndarray:
        """Host buffers in and out: complex64[n_in] -> complex64[n_channels, n_out]."""
        a = np.ascontiguousarray(x, dtype=np.complex64)
        no = self.output_items(a.size)
        out = np.zeros((self.n_channels, max(no, 1)), dtype=np.complex64)
        n = C.c_size_t(0)
        self._check(self.L.lora_hip_channelizer_work(self.h, a.ctypes.data, a.size, out.ctypes.data, out.shape[1], C.byref(n)))
        return out[:, : n.value]

    def run_device(self, d_in: int, n_in: int, d_out: int, out_stride: int, stream: int = 0) -> int:
        n = C.c_size_t(0)
        self._check(self.L.lora_hip_channelizer_run_device(self.h, d_in, n_in, d_out, out_stride, C.byref(n), stream))
        return int(n.value)

    def work_raw(self, raw, fmt=None, scale: float = 0.0) -> np.ndarray:
        """Integer items in (flat interleaved or (n, 2); fmt None: from the dtype), complex64[n_channels, n_out] out."""
        a, f, n_items = _raw_items(raw, fmt)
        no = self.output_items(n_items)
        out = np.zeros((self.n_channels, max(no, 1)), dtype=np.complex64)
        n = C.c_size_t(0)
        self._check(self.L.lora_hip_channelizer_work_raw(self.h, a.ctypes.data, n_items, f, float(scale), out.ctypes.data, out.shape[1], C.byref(n)))
        return out[:, : n.value]

    def run_device_raw(self, d_in: int, n_in: int, fmt: int, d_out: int, out_stride: int, scale: float = 0.0, stream: int = 0) -> int:
        n = C.c_size_t(0)
        self._check(self.L.lora_hip_channelizer_run_device_raw(self.h, d_in, n_in, int(fmt), float(scale), d_out, out_stride, C.byref(n), stream))
        return int(n.value)

    def apply_cfo(self, cfo: float):
        self._check(self.L.lora_hip_channelizer_apply_cfo(self.h, float(cfo)))

    def kernel_ms(self) -> float:
        return float(self.L.lora_hip_channelizer_last_kernel_ms(self.h))

    def close(self):
        if self.h:
            self.L.lora_hip_channelizer_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FilterBank:
    """lora_hip_filterbank_* (include/lora_hip_filterbank.h): the polyphase DFT channeliser for channels on a uniform grid.
    Row c is the channeliser's output at grid_offset + channels[c] * samp_rate / n_grid (Hz from the capture's centre)."""

    def __init__(self, samp_rate, grid_offset, n_grid, channels, bandwidth, decimation=1, device=0, cutoff_hz=0.0, transition_hz=0.0, flags=0):
        self.L = load()
        self.channels = [int(k) for k in channels]
        self.n_channels = len(self.channels)
        self._chan = (C.c_int32 * max(self.n_channels, 1))(*self.channels)
        cfg = FilterBankConfig(struct_size=C.sizeof(FilterBankConfig), samp_rate=float(samp_rate), grid_offset_hz=float(grid_offset), n_grid=int(n_grid),
                               channels=self._chan, n_channels=self.n_channels, bandwidth=int(bandwidth), decimation=int(decimation), device=int(device),
                               cutoff_hz=float(cutoff_hz), transition_hz=float(transition_hz), flags=int(flags))
        self.h = C.c_void_p()
        st = self.L.lora_hip_filterbank_create(C.byref(cfg), C.byref(self.h))
        if st != 0:
            raise LoraHipError(st, self.L.lora_hip_strerror(st).decode())

    def _check(self, st):
        if st != 0:
            raise LoraHipError(st, (self.L.lora_hip_filterbank_last_error(self.h) or b"").decode() or self.L.lora_hip_strerror(st).decode())

    def taps(self) -> np.ndarray:
        n = C.c_size_t(0)
        self._check(self.L.lora_hip_filterbank_taps(self.h, None, 0, C.byref(n)))
        t = np.zeros(n.value, dtype=np.float32)
        self._check(self.L.lora_hip_filterbank_taps(self.h, t.ctypes.data, t.size, C.byref(n)))
        return t

    def output_items(self, n_in: int) -> int:
        return int(self.L.lora_hip_filterbank_output_items(self.h, n_in))

    def work(self, x) -> np.ndarray:
        """Host buffers in and out: complex64[n_in] -> complex64[n_channels, n_out]."""
        a = np.ascontiguousarray(x, dtype=np.complex64)
        no = self.output_items(a.size)
        out = np.zeros((self.n_channels, max(no, 1)), dtype=np.complex64)
        n = C.c_size_t(0)
        self._check(self.L.lora_hip_filterbank_work(self.h, a.ctypes.data, a.size, out.ctypes.data, out.shape[1], C.byref(n)))
        return out[:, : n.value]

    def run_device(self, d_in: int, n_in: int, d_out: int, out_stride: int, stream: int = 0) -> int:
        n = C.c_size_t(0)
        self._check(self.L.lora_hip_filterbank_run_device(self.h, d_in, n_in, d_out, out_stride, C.byref(n), stream))
        return int(n.value)

    def run_device_rows(self, d_in: int, n_in: int, row_ptrs: Sequence[int], n_dst: int, max_out: int, stream: int = 0) -> int:
        """row_ptrs[dst * n_channels + c]: device address of row c's first new item for destination dst."""
        ptrs = (C.c_void_p * max(len(row_ptrs), 1))(*[int(p) for p in row_ptrs])
        n = C.c_size_t(0)
        self._check(self.L.lora_hip_filterbank_run_device_rows(self.h, d_in, n_in, ptrs, int(n_dst), int(max_out), C.byref(n), stream))
        return int(n.value)

    def work_raw(self, raw, fmt=None, scale: float = 0.0) -> np.ndarray:
        """Integer items in (flat interleaved or (n, 2); fmt None: from the dtype), complex64[n_channels, n_out] out."""
        a, f, n_items = _raw_items(raw, fmt)
        no = self.output_items(n_items)
        out = np.zeros((self.n_channels, max(no, 1)), dtype=np.complex64)
        n = C.c_size_t(0)
        self._check(self.L.lora_hip_filterbank_work_raw(self.h, a.ctypes.data, n_items, f, float(scale), out.ctypes.data, out.shape[1], C.byref(n)))
        return out[:, : n.value]

    def run_device_raw(self, d_in: int, n_in: int, fmt: int, d_out: int, out_stride: int, scale: float = 0.0, stream: int = 0) -> int:
        n = C.c_size_t(0)
        self._check(self.L.lora_hip_filterbank_run_device_raw(self.h, d_in, n_in, int(fmt), float(scale), d_out, out_stride, C.byref(n), stream))
        return int(n.value)

    def run_device_rows_raw(self, d_in: int, n_in: int, fmt: int, row_ptrs: Sequence[int], n_dst: int, max_out: int, scale: float = 0.0, stream: int = 0) -> int:
        ptrs = (C.c_void_p * max(len(row_ptrs), 1))(*[int(p) for p in row_ptrs])
        n = C.c_size_t(0)
        self._check(self.L.lora_hip_filterbank_run_device_rows_raw(self.h, d_in, n_in, int(fmt), float(scale), ptrs, int(n_dst), int(max_out), C.byref(n), stream))
        return int(n.value)

    def plan(self) -> dict:
        """The tile shape the handle planned (lora_hip_filterbank_get_plan): cw, g, nc, q, lds_bytes."""
        cw, g, nc, q, lds = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_size_t(0)
        self._check(self.L.lora_hip_filterbank_get_plan(self.h, C.byref(cw), C.byref(g), C.byref(nc), C.byref(q), C.byref(lds)))
        return dict(cw=int(cw.value), g=int(g.value), nc=int(nc.value), q=int(q.value), lds_bytes=int(lds.value))

    def kernel_ms(self) -> float:
        return float(self.L.lora_hip_filterbank_last_kernel_ms(self.h))

    def close(self):
        if self.h:
            self.L.lora_hip_filterbank_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Spectrum:
    """lora_hip_spectrum_* (include/lora_hip_spectrum.h): Welch power-spectrum rows and band powers of a wide-band capture.
    bands: (first_bin, n_bins) pairs in centred indices (gr_lora_amd.spectrum.band_bins / grid_bands make them)."""

    def __init__(self, samp_rate, nfft=1024, hop=512, n_avg=16, window=SPECTRUM_WINDOW_HANN, peak=False, bands=(), device=0):
        self.L = load()
        self.nfft, self.hop, self.n_avg = int(nfft), int(hop), int(n_avg)
        self.bands = [(int(a), int(b)) for a, b in bands]
        self.n_bands = len(self.bands)
        self.peak = bool(peak)
        self._bands = (C.c_uint32 * max(2 * self.n_bands, 1))(*[v for b in self.bands for v in b])
        cfg = SpectrumConfig(struct_size=C.sizeof(SpectrumConfig), samp_rate=float(samp_rate), nfft=self.nfft, hop=self.hop, n_avg=self.n_avg,
                             window=int(window), flags=SPECTRUM_FLAG_PEAK if peak else 0,
                             bands=self._bands, n_bands=self.n_bands, device=int(device))
        self.h = C.c_void_p()
        st = self.L.lora_hip_spectrum_create(C.byref(cfg), C.byref(self.h))
        if st != 0:
            raise LoraHipError(st, self.L.lora_hip_strerror(st).decode())

    def _check(self, st):
        if st != 0:
            raise LoraHipError(st, (self.L.lora_hip_spectrum_last_error(self.h) or b"").decode() or self.L.lora_hip_strerror(st).decode())

    def window(self) -> np.ndarray:
        n = C.c_size_t(0)
        self._check(self.L.lora_hip_spectrum_window(self.h, None, 0, C.byref(n)))
        w = np.zeros(n.value, dtype=np.float32)
        self._check(self.L.lora_hip_spectrum_window(self.h, w.ctypes.data, w.size, C.byref(n)))
        return w

    def output_rows(self, n_in: int) -> int:
        return int(self.L.lora_hip_spectrum_output_rows(self.h, int(n_in)))

    def _host_out(self, rows):
        r = max(rows, 1)
        psd = np.zeros((r, self.nfft), dtype=np.float32)
        peak = np.zeros((r, self.nfft), dtype=np.float32) if self.peak else None
        band = np.zeros((r, self.n_bands), dtype=np.float32) if self.n_bands else None
        return psd, peak, band

    @staticmethod
    def _cut(psd, peak, band, n, first):
        return psd[:n], (None if peak is None else peak[:n]), (None if band is None else band[:n]), int(first)

    def work(self, x, max_rows=None):
        """Host buffers: complex64[n_in] -> (psd[rows, nfft], peak or None, band[rows, n_bands] or None, first_row), float32."""
        a = np.ascontiguousarray(x, dtype=np.complex64)
        rows = self.output_rows(a.size) if max_rows is None else int(max_rows)
        psd, peak, band = self._host_out(rows)
        n, first = C.c_size_t(0), C.c_uint64(0)
        self._check(self.L.lora_hip_spectrum_work(self.h, a.ctypes.data, a.size, psd.ctypes.data, None if peak is None else peak.ctypes.data,
                                                  None if band is None else band.ctypes.data, self.nfft, rows, C.byref(n), C.byref(first)))
        return self._cut(psd, peak, band, n.value, first.value)

    def work_raw(self, raw, fmt=None, scale: float = 0.0, max_rows=None):
        """Integer items in (flat interleaved or (n, 2); fmt None: from the dtype); output as work()."""
        a, f, n_items = _raw_items(raw, fmt)
        rows = self.output_rows(n_items) if max_rows is None else int(max_rows)
        psd, peak, band = self._host_out(rows)
        n, first = C.c_size_t(0), C.c_uint64(0)
        self._check(self.L.lora_hip_spectrum_work_raw(self.h, a.ctypes.data, n_items, f, float(scale), psd.ctypes.data,
                                                      None if peak is None else peak.ctypes.data, None if band is None else band.ctypes.data,
                                                      self.nfft, rows, C.byref(n), C.byref(first)))
        return self._cut(psd, peak, band, n.value, first.value)

    def run_device(self, d_in: int, n_in: int, d_psd: int, d_peak, d_band, row_stride: int, max_rows: int, stream: int = 0):
        """-> (rows written, absolute index of the first of them); d_peak / d_band None where the handle has none."""
        n, first = C.c_size_t(0), C.c_uint64(0)
        self._check(self.L.lora_hip_spectrum_run_device(self.h, d_in, int(n_in), d_psd, d_peak, d_band, int(row_stride), int(max_rows), C.byref(n),
                                                        C.byref(first), stream))
        return int(n.value), int(first.value)

    def run_device_raw(self, d_in: int, n_in: int, fmt: int, d_psd: int, d_peak, d_band, row_stride: int, max_rows: int, scale: float = 0.0, stream: int = 0):
        n, first = C.c_size_t(0), C.c_uint64(0)
        self._check(self.L.lora_hip_spectrum_run_device_raw(self.h, d_in, int(n_in), int(fmt), float(scale), d_psd, d_peak, d_band, int(row_stride),
                                                            int(max_rows), C.byref(n), C.byref(first), stream))
        return int(n.value), int(first.value)

    def reset(self):
        self._check(self.L.lora_hip_spectrum_reset(self.h))

    def kernel_ms(self) -> float:
        return float(self.L.lora_hip_spectrum_last_kernel_ms(self.h))

    def close(self):
        if self.h:
            self.L.lora_hip_spectrum_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Resampler:
    """lora_hip_resampler_* (include/lora_hip_resampler.h): the stream at rate fs -> the stream at rate fs * interpolation / decimation.
    gr_lora_amd.resampler.resample is the definition."""

    def __init__(self, interpolation, decimation, zero_crossings=16, beta=8.0, cutoff=0.8, device=0):
        self.L = load()
        cfg = ResamplerConfig(struct_size=C.sizeof(ResamplerConfig), interpolation=int(interpolation), decimation=int(decimation),
                              zero_crossings=int(zero_crossings), beta=float(beta), cutoff=float(cutoff), device=int(device), flags=0)
        self.h = C.c_void_p()
        st = self.L.lora_hip_resampler_create(C.byref(cfg), C.byref(self.h))
        if st != 0:
            raise LoraHipError(st, self.L.lora_hip_strerror(st).decode())

    def _check(self, st):
        if st != 0:
            raise LoraHipError(st, (self.L.lora_hip_resampler_last_error(self.h) or b"").decode() or self.L.lora_hip_strerror(st).decode())

    def taps(self) -> np.ndarray:
        n = C.c_size_t(0)
        self._check(self.L.lora_hip_resampler_taps(self.h, None, 0, C.byref(n)))
        t = np.zeros(n.value, dtype=np.float32)
        self._check(self.L.lora_hip_resampler_taps(self.h, t.ctypes.data, t.size, C.byref(n)))
        return t

    def ratio(self) -> Tuple[int, int, int]:
        """The reduced (interpolation, decimation) and the taps per output Q."""
        l, m, q = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self._check(self.L.lora_hip_resampler_ratio(self.h, C.byref(l), C.byref(m), C.byref(q)))
        return int(l.value), int(m.value), int(q.value)

    def delay(self) -> float:
        return float(self.L.lora_hip_resampler_delay(self.h))

    def plan(self) -> Tuple[int, int, int, int]:
        """The launch plan (lora_hip_resampler_get_plan): tile, tiles_per_group, row_stride, lds_bytes."""
        t, g, s, lds = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_size_t(0)
        self._check(self.L.lora_hip_resampler_get_plan(self.h, C.byref(t), C.byref(g), C.byref(s), C.byref(lds)))
        return int(t.value), int(g.value), int(s.value), int(lds.value)

    def output_items(self, n_in: int) -> int:
        return int(self.L.lora_hip_resampler_output_items(self.h, int(n_in)))

    def work(self, x, max_out=None):
        """Host buffers: complex64[n_in] -> (complex64[n_out], absolute index of the first output)."""
        a = np.ascontiguousarray(x, dtype=np.complex64)
        cap = self.output_items(a.size) if max_out is None else int(max_out)
        y = np.zeros(max(cap, 1), dtype=np.complex64)
        n, first = C.c_size_t(0), C.c_uint64(0)
        self._check(self.L.lora_hip_resampler_work(self.h, a.ctypes.data, a.size, y.ctypes.data, cap, C.byref(n), C.byref(first)))
        return y[:n.value], int(first.value)

    def work_raw(self, raw, fmt=None, scale: float = 0.0, max_out=None):
        """Integer items in (flat interleaved or (n, 2); fmt None: from the dtype); output as work()."""
        a, f, n_items = _raw_items(raw, fmt)
        cap = self.output_items(n_items) if max_out is None else int(max_out)
        y = np.zeros(max(cap, 1), dtype=np.complex64)
        n, first = C.c_size_t(0), C.c_uint64(0)
        self._check(self.L.lora_hip_resampler_work_raw(self.h, a.ctypes.data, n_items, f, float(scale), y.ctypes.data, cap, C.byref(n), C.byref(first)))
        return y[:n.value], int(first.value)

    def run_device(self, d_in: int, n_in: int, d_out: int, max_out: int, stream: int = 0):
        """-> (outputs written, absolute index of the first of them)."""
        n, first = C.c_size_t(0), C.c_uint64(0)
        self._check(self.L.lora_hip_resampler_run_device(self.h, d_in, int(n_in), d_out, int(max_out), C.byref(n), C.byref(first), stream))
        return int(n.value), int(first.value)

    def run_device_raw(self, d_in: int, n_in: int, fmt: int, d_out: int, max_out: int, scale: float = 0.0, stream: int = 0):
        n, first = C.c_size_t(0), C.c_uint64(0)
        self._check(self.L.lora_hip_resampler_run_device_raw(self.h, d_in, int(n_in), int(fmt), float(scale), d_out, int(max_out), C.byref(n),
                                                             C.byref(first), stream))
        return int(n.value), int(first.value)

    def reset(self):
        self._check(self.L.lora_hip_resampler_reset(self.h))

    def kernel_ms(self) -> float:
        return float(self.L.lora_hip_resampler_last_kernel_ms(self.h))

    def close(self):
        if self.h:
            self.L.lora_hip_resampler_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Gateway:
    """lora_hip_gateway_* (include/lora_hip_gateway.h): one filter bank over a wide-band capture, one decoder per spreading factor
    on every row, fed on the device.  decoders: one dict of Config fields per spreading factor (sf, cr, crc, implicit,
    reduced_rate, demod, ...); samp_rate, bandwidth and device follow the filter bank."""

    def __init__(self, samp_rate, grid_offset, n_grid, channels, bandwidth, decoders, decimation=1, device=0, cutoff_hz=0.0, transition_hz=0.0, flags=0):
        self.L = load()
        self.channels = [int(k) for k in channels]
        self._chan = (C.c_int32 * max(len(self.channels), 1))(*self.channels)
        fb = FilterBankConfig(struct_size=C.sizeof(FilterBankConfig), samp_rate=float(samp_rate), grid_offset_hz=float(grid_offset), n_grid=int(n_grid),
                              channels=self._chan, n_channels=len(self.channels), bandwidth=int(bandwidth), decimation=int(decimation), device=int(device),
                              cutoff_hz=float(cutoff_hz), transition_hz=float(transition_hz), flags=0)
        rate = float(np.float32(float(samp_rate) / int(decimation)))
        self.sfs = [int(d["sf"]) for d in decoders]
        self._dec = (Config * max(len(decoders), 1))()
        for i, d in enumerate(decoders):
            kw = dict(samp_rate=rate, bandwidth=int(bandwidth), device=int(device), cr=4, crc=1, demod=DEMOD_FFT_COMPAT)
            kw.update(d)
            for k in ("implicit", "crc", "reduced_rate", "disable_drift_correction"):
                if k in kw:
                    kw[k] = int(bool(kw[k]))
            self._dec[i] = Config(struct_size=C.sizeof(Config), **kw)
        cfg = GatewayConfig(struct_size=C.sizeof(GatewayConfig), filterbank=fb, decoders=self._dec, n_decoders=len(decoders), flags=int(flags))
        self.h = C.c_void_p()
        st = self.L.lora_hip_gateway_create(C.byref(cfg), C.byref(self.h))
        if st != 0:
            raise LoraHipError(st, "%s (%s)" % (self.L.lora_hip_strerror(st).decode(), self.L.lora_hip_last_error(None).decode()))

    def _check(self, st):
        if st != 0:
            raise LoraHipError(st, "%s (%s)" % (self.L.lora_hip_strerror(st).decode(), (self.L.lora_hip_gateway_last_error(self.h) or b"").decode()))

    def work(self, iq: np.ndarray):
        """complex64 wide-band items from host memory."""
        a = np.ascontiguousarray(iq, dtype=np.complex64)
        self._check(self.L.lora_hip_gateway_work(self.h, a.ctypes.data, a.size))

    def work_device(self, ptr: int, n: int, stream: int = 0):
        """n complex64 items at device address ptr, read after the work queued on stream."""
        self._check(self.L.lora_hip_gateway_work_device(self.h, ptr, int(n), stream))

    def work_raw(self, raw, fmt=None, scale: float = 0.0):
        """Integer wide-band items from host memory (flat interleaved or (n, 2); fmt None: from the dtype)."""
        a, f, n_items = _raw_items(raw, fmt)
        self._check(self.L.lora_hip_gateway_work_raw(self.h, a.ctypes.data, n_items, f, float(scale)))

    def work_device_raw(self, ptr: int, n: int, fmt: int, scale: float = 0.0, stream: int = 0):
        """n items of format fmt at device address ptr, read after the work queued on stream."""
        self._check(self.L.lora_hip_gateway_work_device_raw(self.h, ptr, int(n), int(fmt), float(scale), stream))

    def flush(self):
        self._check(self.L.lora_hip_gateway_flush(self.h))

    def set_latency(self, ms: float):
        self._check(self.L.lora_hip_gateway_set_latency(self.h, float(ms)))

    def drain(self) -> List[Tuple[bytes, GatewayFrameInfo]]:
        out = []
        buf = (C.c_uint8 * 320)()
        while self.L.lora_hip_gateway_frames_available(self.h):
            n = C.c_size_t(0)
            info = GatewayFrameInfo()
            self._check(self.L.lora_hip_gateway_poll_frame(self.h, buf, 320, C.byref(n), C.byref(info)))
            out.append((bytes(buf[: n.value]), info))
        return out

    def enable_link(self, on: bool = True):
        self._check(self.L.lora_hip_link_gateway_enable(self.h, int(bool(on))))

    def drain_link(self) -> List[Tuple[bytes, GatewayFrameInfo, "LinkMetrics"]]:
        out = []
        buf = (C.c_uint8 * 320)()
        while self.L.lora_hip_gateway_frames_available(self.h):
            n, info, met = C.c_size_t(0), GatewayFrameInfo(), LinkMetrics()
            self._check(self.L.lora_hip_link_gateway_poll_frame(self.h, buf, 320, C.byref(n), C.byref(info), C.byref(met)))
            out.append((bytes(buf[: n.value]), info, met))
        return out

    def stats(self) -> dict:
        s = GatewayStats(struct_size=C.sizeof(GatewayStats))
        self._check(self.L.lora_hip_gateway_stats(self.h, C.byref(s)))
        nd = s.n_decoders
        return {"passes": {self.sfs[i]: int(s.passes[i]) for i in range(nd)},
                "passes_by_latency": {self.sfs[i]: int(s.passes_by_latency[i]) for i in range(nd)},
                "filterbank_calls": int(s.filterbank_calls), "filterbank_ms": float(s.filterbank_ms), "items_in": int(s.items_in),
                "step_outputs": int(s.step_outputs)}

    def close(self):
        if getattr(self, "h", None):
            self.L.lora_hip_gateway_destroy(self.h)
            self.h = None

    __del__ = close


def tx_frame(payload, sf, cr, bandwidth, start=0, freq_hz=0.0, amplitude=1.0, crc=True, implicit=False, reduced_rate=False, preamble_len=0,
             sync_shifts=None, hdr_nibbles=None, crc_bytes=None) -> TxFrame:
    """A lora_hip_tx_frame_t.  hdr_nibbles / crc_bytes None: the valid header checksum / payload CRC.  The payload's bytes are
    kept alive by the returned struct."""
    pl = bytes(payload)
    buf = (C.c_uint8 * max(len(pl), 1))(*pl)
    s0, s1 = (-1, -1) if sync_shifts is None else (int(sync_shifts[0]), int(sync_shifts[1]))
    f = TxFrame(struct_size=C.sizeof(TxFrame), bandwidth=int(bandwidth), sf=int(sf), implicit=int(bool(implicit)), cr=int(cr), crc=int(bool(crc)),
                reduced_rate=int(bool(reduced_rate)), preamble_len=int(preamble_len), sync_shifts=(C.c_int32 * 2)(s0, s1), start=int(start),
                freq_hz=float(freq_hz), amplitude=float(amplitude), length=len(pl), payload=C.cast(buf, C.POINTER(C.c_uint8)))
    f._payload = buf
    if hdr_nibbles is not None:
        f.flags |= TX_FRAME_HDR_NIBBLES
        f.hdr_nibbles = (C.c_uint8 * 2)(int(hdr_nibbles[0]), int(hdr_nibbles[1]))
    if crc_bytes is not None:
        f.flags |= TX_FRAME_CRC_BYTES
        f.crc_bytes = (C.c_uint8 * 2)(*bytes(crc_bytes)[:2])
    return f


def _tx_status(L, st: int, what: str):
    if st != 0:
        raise LoraHipError(st, "%s: %s" % (what, L.lora_hip_strerror(st).decode()))


def tx_encode(frame: TxFrame) -> Tuple[List[int], List[int]]:
    """lora_hip_tx_encode (host only): (header_shifts[8], payload_shifts) as synth.encode_shifts."""
    L = load()
    out = (C.c_uint16 * TX_MAX_SHIFTS)()
    nh, npay = C.c_uint32(0), C.c_uint32(0)
    _tx_status(L, L.lora_hip_tx_encode(C.byref(frame), out, TX_MAX_SHIFTS, C.byref(nh), C.byref(npay)), "lora_hip_tx_encode")
    return list(out[: nh.value]), list(out[nh.value: nh.value + npay.value])


def tx_frame_items(frame: TxFrame, samp_rate: float) -> int:
    """lora_hip_tx_frame_items (host only): items of the frame's waveform at samp_rate."""
    L = load()
    n = C.c_uint64(0)
    _tx_status(L, L.lora_hip_tx_frame_items(C.byref(frame), float(samp_rate), C.byref(n)), "lora_hip_tx_frame_items")
    return int(n.value)


class Tx:
    """lora_hip_tx_* (include/lora_hip_tx.h): the traffic synthesiser's stream; frames in, a wide-band capture out on the device."""

    def __init__(self, samp_rate, device=0, noise_sigma=0.0, seed=0, flags=0):
        self.L = load()
        cfg = TxConfig(struct_size=C.sizeof(TxConfig), device=int(device), samp_rate=float(samp_rate), noise_sigma=float(noise_sigma),
                       seed=int(seed) & 0xFFFFFFFFFFFFFFFF, flags=int(flags))
        self.h = C.c_void_p()
        st = self.L.lora_hip_tx_create(C.byref(cfg), C.byref(self.h))
        if st != 0:
            self.h = None
            raise LoraHipError(st, self.L.lora_hip_strerror(st).decode())
        self.samp_rate, self.device = float(samp_rate), int(device)

    def _check(self, st):
        if st != 0:
            raise LoraHipError(st, "%s (%s)" % (self.L.lora_hip_strerror(st).decode(), (self.L.lora_hip_tx_last_error(self.h) or b"").decode()))

    def add_frames(self, frames: Sequence[TxFrame]):
        arr = (TxFrame * max(len(frames), 1))(*frames)
        self._check(self.L.lora_hip_tx_add_frames(self.h, arr, len(frames)))

    def generate_device(self, d_out: int, n: int, stream: int = 0):
        self._check(self.L.lora_hip_tx_generate_device(self.h, d_out, int(n), stream))

    def generate_device_raw(self, d_out: int, n: int, fmt: int, full_scale: float, stream: int = 0):
        self._check(self.L.lora_hip_tx_generate_device_raw(self.h, d_out, int(n), int(fmt), float(full_scale), stream))

    def generate(self, n: int) -> np.ndarray:
        out = np.empty(int(n), dtype=np.complex64)
        self._check(self.L.lora_hip_tx_generate(self.h, out.ctypes.data, int(n)))
        return out

    @property
    def position(self) -> int:
        return int(self.L.lora_hip_tx_position(self.h))

    @property
    def pending(self) -> int:
        return int(self.L.lora_hip_tx_pending(self.h))

    def kernel_ms(self) -> float:
        return float(self.L.lora_hip_tx_last_kernel_ms(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.L.lora_hip_tx_destroy(self.h)
            self.h = None

    __del__ = close


class Conditioner:
    """lora_hip_conditioner_* (include/lora_hip_conditioner.h): DC-offset removal and IQ-imbalance correction, cf32 out at the
    input's rate.  gr_lora_amd.conditioner.condition is the definition."""

    def __init__(self, block=4096, window=16, dc=True, iq=True, device=0):
        self.L = load()
        flags = (CONDITIONER_FLAG_DC if dc else 0) | (CONDITIONER_FLAG_IQ if iq else 0)
        cfg = ConditionerConfig(struct_size=C.sizeof(ConditionerConfig), block=int(block), window=int(window), flags=flags, device=int(device))
        self.h = C.c_void_p()
        st = self.L.lora_hip_conditioner_create(C.byref(cfg), C.byref(self.h))
        if st != 0:
            raise LoraHipError(st, self.L.lora_hip_strerror(st).decode())
        self._held = 0                                 # items waiting for their block: what went in less what came out

    def _check(self, st):
        if st != 0:
            raise LoraHipError(st, (self.L.lora_hip_conditioner_last_error(self.h) or b"").decode() or self.L.lora_hip_strerror(st).decode())

    def plan(self) -> Tuple[int, int, int, int]:
        """The launch plan (lora_hip_conditioner_get_plan): block, window, blocks_per_group, items_per_group."""
        b, w, g, i = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self._check(self.L.lora_hip_conditioner_get_plan(self.h, C.byref(b), C.byref(w), C.byref(g), C.byref(i)))
        return int(b.value), int(w.value), int(g.value), int(i.value)

    def output_items(self, n_in: int) -> int:
        return int(self.L.lora_hip_conditioner_output_items(self.h, int(n_in)))

    def work(self, x, max_out=None):
        """Host buffers: complex64[n_in] -> (complex64[n_out], absolute index of the first output)."""
        a = np.ascontiguousarray(x, dtype=np.complex64)
        cap = self.output_items(a.size) if max_out is None else int(max_out)
        y = np.zeros(max(cap, 1), dtype=np.complex64)
        n, first = C.c_size_t(0), C.c_uint64(0)
        self._check(self.L.lora_hip_conditioner_work(self.h, a.ctypes.data, a.size, y.ctypes.data, cap, C.byref(n), C.byref(first)))
        self._held += a.size - n.value
        return y[:n.value], int(first.value)

    def work_raw(self, raw, fmt=None, scale: float = 0.0, max_out=None):
        """Integer items in (flat interleaved or (n, 2); fmt None: from the dtype); output as work()."""
        a, f, n_items = _raw_items(raw, fmt)
        cap = self.output_items(n_items) if max_out is None else int(max_out)
        y = np.zeros(max(cap, 1), dtype=np.complex64)
        n, first = C.c_size_t(0), C.c_uint64(0)
        self._check(self.L.lora_hip_conditioner_work_raw(self.h, a.ctypes.data, n_items, f, float(scale), y.ctypes.data, cap, C.byref(n), C.byref(first)))
        self._held += n_items - n.value
        return y[:n.value], int(first.value)

    def run_device(self, d_in: int, n_in: int, d_out: int, max_out: int, stream: int = 0):
        """-> (outputs written, absolute index of the first of them)."""
        n, first = C.c_size_t(0), C.c_uint64(0)
        self._check(self.L.lora_hip_conditioner_run_device(self.h, d_in, int(n_in), d_out, int(max_out), C.byref(n), C.byref(first), stream))
        self._held += int(n_in) - n.value
        return int(n.value), int(first.value)

    def run_device_raw(self, d_in: int, n_in: int, fmt: int, d_out: int, max_out: int, scale: float = 0.0, stream: int = 0):
        n, first = C.c_size_t(0), C.c_uint64(0)
        self._check(self.L.lora_hip_conditioner_run_device_raw(self.h, d_in, int(n_in), int(fmt), float(scale), d_out, int(max_out), C.byref(n),
                                                               C.byref(first), stream))
        self._held += int(n_in) - n.value
        return int(n.value), int(first.value)

    def held_items(self) -> int:
        """Items held back for the next block (what flush would emit)."""
        return self._held

    def flush(self):
        """-> (the held items, corrected with the newest parameters; absolute index of the first of them)."""
        cap = self.held_items()
        y = np.zeros(max(cap, 1), dtype=np.complex64)
        n, first = C.c_size_t(0), C.c_uint64(0)
        self._check(self.L.lora_hip_conditioner_flush(self.h, y.ctypes.data, cap, C.byref(n), C.byref(first)))
        self._held -= n.value
        return y[:n.value], int(first.value)

    def flush_device(self, d_out: int, max_out: int, stream: int = 0):
        n, first = C.c_size_t(0), C.c_uint64(0)
        self._check(self.L.lora_hip_conditioner_flush_device(self.h, d_out, int(max_out), C.byref(n), C.byref(first), stream))
        self._held -= n.value
        return int(n.value), int(first.value)

    def block_records(self):
        """-> (moments float64[n, 5], params float32[n, 4]) of the blocks the last run call completed."""
        n = C.c_size_t(0)
        self._check(self.L.lora_hip_conditioner_block_records(self.h, None, None, 0, C.byref(n), None, None))
        mom, par = np.zeros((n.value, 5), dtype=np.float64), np.zeros((n.value, 4), dtype=np.float32)
        if n.value:
            self._check(self.L.lora_hip_conditioner_block_records(self.h, mom.ctypes.data, par.ctypes.data, n.value, C.byref(n), None, None))
        return mom, par

    def newest(self):
        """-> (params float32[4]: dI, dQ, a, b; estimates float64[4]: mI, mQ, r, q) of the newest complete block."""
        n = C.c_size_t(0)
        par, est = np.zeros(4, dtype=np.float32), np.zeros(4, dtype=np.float64)
        self._check(self.L.lora_hip_conditioner_block_records(self.h, None, None, 0, C.byref(n), par.ctypes.data, est.ctypes.data))
        return par, est

    def set_fixed(self, d_i, d_q, a, b):
        self._check(self.L.lora_hip_conditioner_set_fixed(self.h, float(d_i), float(d_q), float(a), float(b)))

    def set_adaptive(self):
        self._check(self.L.lora_hip_conditioner_set_adaptive(self.h))

    def reset(self):
        self._check(self.L.lora_hip_conditioner_reset(self.h))
        self._held = 0

    def kernel_ms(self) -> float:
        return float(self.L.lora_hip_conditioner_last_kernel_ms(self.h))

    def close(self):
        if self.h:
            self.L.lora_hip_conditioner_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
