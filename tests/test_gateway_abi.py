"""CPU: the C ABI of the multi-SF gateway (include/lora_hip_gateway.h) and the filter bank's many-destination entry
(lora_hip_filterbank_run_device_rows) - exports, struct layouts against the C compiler's, argument checks before any device
call, and no CPU fallback."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_BAD_SF, ERR_BAD_CONFIG, ERR_NO_DEVICE, ERR_ARG = -1, -2, -3, -6


@pytest.fixture(scope="module")
def lib():
    from gr_lora_amd import build, capi
    build.build_library()
    return capi.load()


def _exported(prefix):
    from gr_lora_amd import capi
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    return set(re.findall(r" T (%s[a-z_]+)" % prefix, out))


def test_every_declared_symbol_is_listed_and_exported(lib):
    from gr_lora_amd import capi
    hdr = open(os.path.join(ROOT, "include", "lora_hip_gateway.h")).read()
    declared = set(re.findall(r"\b(lora_hip_gateway_[a-z_]+)\s*\(", hdr))
    assert declared == set(capi.EXPORTS_GATEWAY)
    assert declared <= _exported("lora_hip_gateway_")
    for name in declared:
        assert getattr(lib, name) is not None
    others = set(capi.EXPORTS + capi.EXPORTS_CHANNELIZER + capi.EXPORTS_FILTERBANK)
    assert not set(capi.EXPORTS_GATEWAY) & others
    # the mux's device-fed path is internal: nothing of it is exported
    out = subprocess.check_output(["nm", "-D", "--defined-only", "-C", capi.LIB_PATH]).decode()
    assert "lora_mux_dev" not in out


def test_run_device_rows_is_declared_and_exported(lib):
    from gr_lora_amd import capi
    hdr = open(os.path.join(ROOT, "include", "lora_hip_filterbank.h")).read()
    assert re.search(r"\blora_hip_filterbank_run_device_rows\s*\(", hdr)
    assert "lora_hip_filterbank_run_device_rows" in capi.EXPORTS_FILTERBANK
    assert "lora_hip_filterbank_run_device_rows" in _exported("lora_hip_filterbank_")
    assert re.search(r"#define LORA_HIP_FILTERBANK_MAX_DST %du" % capi.FILTERBANK_MAX_DST, hdr)
    gw_hdr = open(os.path.join(ROOT, "include", "lora_hip_gateway.h")).read()
    assert re.search(r"#define LORA_HIP_GATEWAY_MAX_DECODERS %du" % capi.GATEWAY_MAX_DECODERS, gw_hdr)
    assert re.search(r"#define LORA_HIP_GATEWAY_STEP_OUTPUTS %du" % capi.GATEWAY_STEP_OUTPUTS, gw_hdr)


def test_structs_match_the_c_layout(tmp_path):
    """sizeof and offsetof of every member, from the C compiler on the header, against the ctypes structs."""
    from gr_lora_amd import capi
    structs = [("lora_hip_gateway_config_t", capi.GatewayConfig), ("lora_hip_gateway_frame_info_t", capi.GatewayFrameInfo),
               ("lora_hip_gateway_stats_t", capi.GatewayStats)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lora_hip_gateway.h"', "int main(void) {"]
    for cname, cls in structs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, cls in structs:
        assert int(got[cname]) == C.sizeof(cls), cname
        for f in cls._fields_:
            assert int(got["%s.%s" % (cname, f[0])]) == getattr(cls, f[0]).offset, (cname, f[0])


def _cfg(sfs=(7, 8, 9, 10, 11, 12), fs=2e6, D=2, M=10, channels=(-4, -3, -2, -1, 0, 1, 2, 3), dec_change=None, **kw):
    from gr_lora_amd import capi
    chans = (C.c_int32 * max(len(channels), 1))(*channels)
    fb = capi.FilterBankConfig(struct_size=C.sizeof(capi.FilterBankConfig), samp_rate=fs, grid_offset_hz=100e3, n_grid=M, channels=chans,
                               n_channels=len(channels), bandwidth=125000, decimation=D, device=0)
    decs = (capi.Config * max(len(sfs), 1))()
    for i, sf in enumerate(sfs):
        decs[i] = capi.Config(struct_size=C.sizeof(capi.Config), samp_rate=fs / max(D, 1), bandwidth=125000, sf=sf, cr=4, crc=1,
                              reduced_rate=int(sf >= 11), device=0, demod=capi.DEMOD_FFT_COMPAT)
    if dec_change:
        for k, v in dec_change.items():
            setattr(decs[len(sfs) - 1], k, v)
    cfg = capi.GatewayConfig(struct_size=C.sizeof(capi.GatewayConfig), filterbank=fb, decoders=decs, n_decoders=len(sfs), flags=0)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg, (chans, decs)


def _create(lib, cfg):
    h = C.c_void_p()
    st = lib.lora_hip_gateway_create(C.byref(cfg), C.byref(h))
    if st == 0:
        lib.lora_hip_gateway_destroy(h)
    return st, h


@pytest.mark.parametrize("change,status", [
    (dict(sfs=()), ERR_BAD_CONFIG),                                    # n_decoders 0
    (dict(sfs=(6, 7, 8, 9, 10, 11, 12), n_decoders=8), ERR_BAD_CONFIG),  # above the limit
    (dict(flags=1), ERR_BAD_CONFIG),
    (dict(sfs=(7, 8, 7)), ERR_BAD_CONFIG),                             # one SF twice
    (dict(dec_change=dict(samp_rate=1e6 + 1)), ERR_BAD_CONFIG),        # not fs / D
    (dict(fs=2e6, D=3, dec_change=dict(samp_rate=2e6 / 3 + 1)), ERR_BAD_CONFIG),
    (dict(dec_change=dict(bandwidth=250000)), ERR_BAD_CONFIG),
    (dict(dec_change=dict(device=1)), ERR_BAD_CONFIG),
    (dict(dec_change=dict(cr=5)), ERR_BAD_CONFIG),
    (dict(dec_change=dict(demod=3)), ERR_BAD_CONFIG),
    (dict(dec_change=dict(sf=13)), ERR_BAD_SF),
    (dict(dec_change=dict(sf=5)), ERR_BAD_SF),
    (dict(dec_change=dict(struct_size=8)), ERR_ARG),
    (dict(D=0, dec_change=dict(samp_rate=2e6)), ERR_BAD_CONFIG),
    (dict(M=0, channels=(0,)), ERR_BAD_CONFIG),                        # the filter bank's own limits
    (dict(channels=(1, 2, 1)), ERR_BAD_CONFIG),
    (dict(struct_size=8), ERR_ARG),
    (dict(dec_change=dict(batch_items=(1 << 18) + 4096)), ERR_BAD_CONFIG),  # a batch that is no whole number of steps
    (dict(dec_change=dict(batch_items=1000)), ERR_BAD_CONFIG),
])
def test_bad_config_fails_before_any_device_call(lib, change, status):
    cfg, keep = _cfg(**change)
    st, h = _create(lib, cfg)
    assert st == status and not h.value


def test_null_arguments(lib):
    from gr_lora_amd import capi
    h = C.c_void_p()
    assert lib.lora_hip_gateway_create(None, C.byref(h)) == ERR_ARG
    cfg, keep = _cfg()
    assert lib.lora_hip_gateway_create(C.byref(cfg), None) == ERR_ARG
    cfg.decoders = C.cast(None, C.POINTER(capi.Config))
    assert lib.lora_hip_gateway_create(C.byref(cfg), C.byref(h)) == ERR_ARG
    cfg2, keep2 = _cfg()
    cfg2.filterbank.channels = C.cast(None, C.POINTER(C.c_int32))
    assert lib.lora_hip_gateway_create(C.byref(cfg2), C.byref(h)) == ERR_ARG
    assert lib.lora_hip_gateway_last_error(None) == b"null handle"
    assert lib.lora_hip_gateway_frames_available(None) == 0
    n = C.c_size_t(0)
    assert lib.lora_hip_gateway_work(None, None, 0) == ERR_ARG
    assert lib.lora_hip_gateway_work_device(None, None, 0, None) == ERR_ARG
    assert lib.lora_hip_gateway_flush(None) == ERR_ARG
    assert lib.lora_hip_gateway_set_latency(None, 1.0) == ERR_ARG
    assert lib.lora_hip_gateway_poll_frame(None, None, 0, C.byref(n), None) == ERR_ARG
    assert lib.lora_hip_gateway_stats(None, None) == ERR_ARG
    ptrs = (C.c_void_p * 1)(None)
    assert lib.lora_hip_filterbank_run_device_rows(None, None, 0, ptrs, 1, 0, C.byref(n), None) == ERR_ARG


def test_valid_config_creates_only_with_a_device(lib):
    """No CPU fallback: a valid config gives LORA_HIP_ERR_NO_DEVICE without a GPU, a handle with one."""
    import torch
    from gr_lora_amd import capi
    gpu = torch.cuda.is_available()
    for kw in (dict(), dict(sfs=(7,)), dict(fs=2e6, D=3), dict(sfs=(6, 7, 8, 9, 10, 11, 12)), dict(dec_change=dict(batch_items=3 << 16))):
        cfg, keep = _cfg(**kw)
        st, h = _create(lib, cfg)
        assert st == (0 if gpu else ERR_NO_DEVICE) and bool(h.value) == gpu, kw
    if not gpu:
        with pytest.raises(capi.LoraHipError):
            capi.Gateway(2e6, 100e3, 10, [0, 1], 125000, [dict(sf=7), dict(sf=12, reduced_rate=True)], decimation=2)


def test_lorawan_reduced_rate_rule():
    from gr_lora_amd import lora
    assert [sf for sf in range(6, 13) if lora.lorawan_reduced_rate(sf, 125000)] == [11, 12]
    assert [sf for sf in range(6, 13) if lora.lorawan_reduced_rate(sf, 250000)] == [12]
    assert not any(lora.lorawan_reduced_rate(sf, 500000) for sf in range(6, 13))


class _FakeDeviceTensor:
    """What multi_sf_gateway_receiver.work reads of a torch CUDA tensor, without a GPU."""

    def __init__(self, dtype, numel, index):
        import types
        self.is_cuda, self.dtype, self._n, self.device = True, dtype, numel, types.SimpleNamespace(index=index)

    def contiguous(self):
        return self

    def numel(self):
        return self._n


def test_receiver_refuses_odd_float32_and_foreign_device_tensors():
    """Checked before the gateway is called: an odd float32 length (no whole I/Q pair) and a tensor on another device."""
    import torch
    from gr_lora_amd import lora
    rx = object.__new__(lora.multi_sf_gateway_receiver)   # (no device here: the checks run before any gateway call)
    rx.device = 0
    with pytest.raises(ValueError, match="interleaved"):
        rx.work(_FakeDeviceTensor(torch.float32, 8193, 0))
    with pytest.raises(ValueError, match="cuda:0"):
        rx.work(_FakeDeviceTensor(torch.complex64, 4096, 1))
    with pytest.raises(TypeError):
        rx.work(_FakeDeviceTensor(torch.float64, 4096, 0))
