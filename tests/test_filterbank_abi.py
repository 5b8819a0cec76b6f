"""CPU: the C ABI of the polyphase filter bank (include/lora_hip_filterbank.h) - exports, argument checks before any device
call, and no CPU fallback."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_BAD_CONFIG, ERR_NO_DEVICE, ERR_ARG = -2, -3, -6


@pytest.fixture(scope="module")
def lib():
    from gr_lora_amd import build, capi
    build.build_library()
    return capi.load()


def _cfg(M=10, channels=(-4, -3, -2, -1, 0, 1, 2, 3), D=2, fs=2e6, f0=100e3, **kw):
    from gr_lora_amd import capi
    arr = (C.c_int32 * max(len(channels), 1))(*channels)
    cfg = capi.FilterBankConfig(struct_size=C.sizeof(capi.FilterBankConfig), samp_rate=fs, grid_offset_hz=f0, n_grid=M, channels=arr,
                                n_channels=len(channels), bandwidth=125000, decimation=D, device=0, **kw)
    return cfg, arr


def _create(lib, cfg):
    h = C.c_void_p()
    st = lib.lora_hip_filterbank_create(C.byref(cfg), C.byref(h))
    if st == 0:
        lib.lora_hip_filterbank_destroy(h)
    return st, h


def test_every_declared_symbol_is_listed_and_exported(lib):
    from gr_lora_amd import capi
    hdr = open(os.path.join(ROOT, "include", "lora_hip_filterbank.h")).read()
    declared = set(re.findall(r"\b(lora_hip_filterbank_[a-z_]+)\s*\(", hdr))
    assert declared == set(capi.EXPORTS_FILTERBANK)
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (lora_hip_filterbank_[a-z_]+)", out))
    assert declared <= exported
    for name in declared:
        assert getattr(lib, name) is not None
    assert not set(capi.EXPORTS_FILTERBANK) & set(capi.EXPORTS + capi.EXPORTS_CHANNELIZER)


def test_config_struct_matches_the_header():
    """FilterBankConfig's fields in the header's order (the ctypes layout is the C layout of the same member list)."""
    from gr_lora_amd import capi
    hdr = open(os.path.join(ROOT, "include", "lora_hip_filterbank.h")).read()
    body = hdr[hdr.index("typedef struct lora_hip_filterbank_config {"):hdr.index("} lora_hip_filterbank_config_t;")]
    names = re.findall(r"\*?(\w+);", body)
    assert names == [f[0] for f in capi.FilterBankConfig._fields_]


@pytest.mark.parametrize("change,status", [
    (dict(M=0, channels=(0,)), ERR_BAD_CONFIG),
    (dict(M=257, channels=(0,)), ERR_BAD_CONFIG),
    (dict(channels=(-4, 5)), ERR_BAD_CONFIG),          # 5 > ceil(10 / 2) - 1
    (dict(channels=(-6, 0)), ERR_BAD_CONFIG),          # -6 < -floor(10 / 2)
    (dict(channels=(1, 2, 1)), ERR_BAD_CONFIG),        # duplicate
    (dict(channels=()), ERR_BAD_CONFIG),
    (dict(D=0), ERR_BAD_CONFIG),
    (dict(D=1025), ERR_BAD_CONFIG),
    (dict(fs=0.0), ERR_BAD_CONFIG),
    (dict(f0=float("nan")), ERR_BAD_CONFIG),
    (dict(flags=1), ERR_BAD_CONFIG),
    (dict(transition_hz=10.0), ERR_BAD_CONFIG),        # 53 fs / (22 tw) taps: far above the limit
    (dict(transition_hz=2.6e6), ERR_BAD_CONFIG),       # 53 fs / (22 tw) = 1.85: one tap, its Hamming window 0 / 0
])
def test_bad_arguments_fail_before_any_device_call(lib, change, status):
    cfg, keep = _cfg(**change)
    st, h = _create(lib, cfg)
    assert st == status and not h.value


def test_null_and_short_struct(lib):
    from gr_lora_amd import capi
    h = C.c_void_p()
    assert lib.lora_hip_filterbank_create(None, C.byref(h)) == ERR_ARG
    cfg, keep = _cfg()
    assert lib.lora_hip_filterbank_create(C.byref(cfg), None) == ERR_ARG
    cfg.struct_size = 8
    assert lib.lora_hip_filterbank_create(C.byref(cfg), C.byref(h)) == ERR_ARG
    cfg2, keep2 = _cfg()
    cfg2.channels = C.cast(None, C.POINTER(C.c_int32))
    assert lib.lora_hip_filterbank_create(C.byref(cfg2), C.byref(h)) == ERR_ARG
    assert lib.lora_hip_filterbank_output_items(None, 100) == 0
    assert lib.lora_hip_filterbank_last_error(None) == b"null handle"
    n = C.c_size_t(0)
    assert lib.lora_hip_filterbank_run_device(None, None, 0, None, 0, C.byref(n), None) == ERR_ARG
    assert lib.lora_hip_filterbank_get_plan(None, None, None, None, None, C.byref(n)) == ERR_ARG
    assert capi.FilterBankConfig.samp_rate.size == 8 and capi.FilterBankConfig.grid_offset_hz.size == 8


def test_valid_arguments_create_only_with_a_device(lib):
    """No CPU fallback: valid arguments give LORA_HIP_ERR_NO_DEVICE without a GPU, a handle with one."""
    import torch
    from gr_lora_amd import capi
    gpu = torch.cuda.is_available()
    for kw in (dict(), dict(M=80, channels=tuple(range(-32, 32)), D=16, fs=16e6), dict(M=1, channels=(0,), D=1024, f0=0.0)):
        cfg, keep = _cfg(**kw)
        st, h = _create(lib, cfg)
        assert st == (0 if gpu else ERR_NO_DEVICE) and bool(h.value) == gpu
    if not gpu:
        with pytest.raises(capi.LoraHipError):
            capi.FilterBank(2e6, 100e3, 10, [0, 1], 125000, 2)
