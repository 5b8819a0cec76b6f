"""CPU: the C ABI of the spectral scan (include/lora_hip_spectrum.h) - exports, argument checks before any device call, the row
arithmetic of the definition, and no CPU fallback."""
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


def _cfg(nfft=1024, hop=512, n_avg=16, window=0, flags=0, bands=((100, 64), (0, 1024)), fs=2e6, device=0):
    from gr_lora_amd import capi
    flat = [v for b in bands for v in b]
    arr = (C.c_uint32 * max(len(flat), 1))(*flat)
    cfg = capi.SpectrumConfig(struct_size=C.sizeof(capi.SpectrumConfig), samp_rate=fs, nfft=nfft, hop=hop, n_avg=n_avg, window=window, flags=flags,
                              bands=arr, n_bands=len(bands), device=device)
    return cfg, arr


def _create(lib, cfg):
    h = C.c_void_p()
    st = lib.lora_hip_spectrum_create(C.byref(cfg), C.byref(h))
    if st == 0:
        lib.lora_hip_spectrum_destroy(h)
    return st, h


def test_every_declared_symbol_is_listed_and_exported(lib):
    from gr_lora_amd import capi
    hdr = open(os.path.join(ROOT, "include", "lora_hip_spectrum.h")).read()
    declared = set(re.findall(r"\b(lora_hip_spectrum_[a-z_]+)\s*\(", hdr))
    assert declared == set(capi.EXPORTS_SPECTRUM) and len(capi.EXPORTS_SPECTRUM) == len(set(capi.EXPORTS_SPECTRUM))
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (lora_hip_spectrum_[a-z_]+)", out))
    assert declared <= exported
    for name in declared:
        assert getattr(lib, name) is not None
    others = set(capi.EXPORTS + capi.EXPORTS_CHANNELIZER + capi.EXPORTS_FILTERBANK + capi.EXPORTS_GATEWAY + capi.EXPORTS_TX + capi.EXPORTS_LINK)
    assert not set(capi.EXPORTS_SPECTRUM) & others


def test_config_struct_matches_the_header():
    """SpectrumConfig's fields in the header's order (the ctypes layout is the C layout of the same member list)."""
    from gr_lora_amd import capi, spectrum
    hdr = open(os.path.join(ROOT, "include", "lora_hip_spectrum.h")).read()
    body = hdr[hdr.index("typedef struct lora_hip_spectrum_config {"):hdr.index("} lora_hip_spectrum_config_t;")]
    names = re.findall(r"\*?(\w+);", body)
    assert names == [f[0] for f in capi.SpectrumConfig._fields_]
    assert capi.SpectrumConfig.samp_rate.size == 8
    limits = dict(re.findall(r"#define LORA_HIP_SPECTRUM_(\w+) (\d+)u", hdr))
    assert (int(limits["MIN_NFFT"]), int(limits["MAX_NFFT"]), int(limits["MAX_AVG"]), int(limits["MAX_BANDS"])) == \
        (spectrum.MIN_NFFT, spectrum.MAX_NFFT, spectrum.MAX_AVG, spectrum.MAX_BANDS)
    assert (int(limits["WINDOW_HANN"]), int(limits["WINDOW_RECT"]), int(limits["FLAG_PEAK"])) == \
        (capi.SPECTRUM_WINDOW_HANN, capi.SPECTRUM_WINDOW_RECT, capi.SPECTRUM_FLAG_PEAK) == (spectrum.HANN, spectrum.RECT, 1)


@pytest.mark.parametrize("change", [
    dict(nfft=32), dict(nfft=8192), dict(nfft=1000), dict(nfft=0),          # a power of two, 64 .. 4096
    dict(hop=0), dict(hop=1025),                                            # 1 <= hop <= nfft
    dict(n_avg=0), dict(n_avg=1025),                                        # 1 .. 1024
    dict(window=2),                                                         # HANN or RECT
    dict(flags=2), dict(flags=0x80000001),                                  # an unknown flag bit
    dict(bands=((0, 1),) * 257),                                            # 0 .. 256 bands
    dict(bands=((1024, 1),)), dict(bands=((1000, 25),)), dict(bands=((5, 0),)), dict(bands=((0, 1025),)),   # inside [0, nfft), not empty
    dict(bands=((0xffffffff, 2),)),                                         # (first + n wraps in 32 bits)
    dict(fs=0.0), dict(fs=float("nan")),
])
def test_bad_config_fails_before_any_device_call(lib, change):
    cfg, keep = _cfg(**change)
    st, h = _create(lib, cfg)
    assert st == ERR_BAD_CONFIG and not h.value


def test_null_and_short_struct(lib):
    from gr_lora_amd import capi
    h = C.c_void_p()
    assert lib.lora_hip_spectrum_create(None, C.byref(h)) == ERR_ARG
    cfg, keep = _cfg()
    assert lib.lora_hip_spectrum_create(C.byref(cfg), None) == ERR_ARG
    cfg.struct_size = C.sizeof(capi.SpectrumConfig) - 1
    assert lib.lora_hip_spectrum_create(C.byref(cfg), C.byref(h)) == ERR_ARG and not h.value
    cfg2, keep2 = _cfg()
    cfg2.bands = C.cast(None, C.POINTER(C.c_uint32))
    assert lib.lora_hip_spectrum_create(C.byref(cfg2), C.byref(h)) == ERR_ARG                 # n_bands > 0 without bands
    assert lib.lora_hip_spectrum_output_rows(None, 100000) == 0
    assert lib.lora_hip_spectrum_last_error(None) == b"null handle"
    assert lib.lora_hip_spectrum_last_kernel_ms(None) == 0.0
    assert lib.lora_hip_spectrum_reset(None) == ERR_ARG
    n, first = C.c_size_t(0), C.c_uint64(0)
    assert lib.lora_hip_spectrum_window(None, None, 0, C.byref(n)) == ERR_ARG
    assert lib.lora_hip_spectrum_run_device(None, None, 0, None, None, None, 0, 0, C.byref(n), C.byref(first), None) == ERR_ARG
    assert lib.lora_hip_spectrum_run_device_raw(None, None, 0, 1, 0.0, None, None, None, 0, 0, C.byref(n), C.byref(first), None) == ERR_ARG
    assert lib.lora_hip_spectrum_work(None, None, 0, None, None, None, 0, 0, C.byref(n), C.byref(first)) == ERR_ARG
    assert lib.lora_hip_spectrum_work_raw(None, None, 0, 1, 0.0, None, None, None, 0, 0, C.byref(n), C.byref(first)) == ERR_ARG
    lib.lora_hip_spectrum_destroy(None)


def test_a_larger_struct_size_is_accepted(lib):
    """struct_size is a lower bound (ABI growth): a caller built against a longer struct gets the same answer as the exact one."""
    import torch
    want = 0 if torch.cuda.is_available() else ERR_NO_DEVICE
    cfg, keep = _cfg()
    cfg.struct_size = C.sizeof(type(cfg)) + 16
    st, h = _create(lib, cfg)
    assert st == want


def test_valid_arguments_create_only_with_a_device(lib):
    """No CPU fallback: valid arguments give LORA_HIP_ERR_NO_DEVICE without a GPU, a handle with one."""
    import torch
    from gr_lora_amd import capi
    gpu = torch.cuda.is_available()
    for kw in (dict(), dict(nfft=64, hop=1, n_avg=1, bands=()), dict(nfft=4096, hop=4096, n_avg=1024, window=1, flags=1, bands=((0, 4096),) * 256)):
        cfg, keep = _cfg(**kw)
        st, h = _create(lib, cfg)
        assert st == (0 if gpu else ERR_NO_DEVICE) and bool(h.value) == gpu
    cfg, keep = _cfg(device=-1)
    assert _create(lib, cfg)[0] == ERR_NO_DEVICE
    if not gpu:
        with pytest.raises(capi.LoraHipError):
            capi.Spectrum(2e6)


@pytest.mark.parametrize("nfft,hop,n_avg,chunks", [
    (64, 64, 1, [63, 1, 64, 0, 200]),
    (64, 32, 3, [127, 1, 95, 1, 1000, 5]),
    (256, 129, 16, [1] * 5 + [2190, 1, 2063, 1, 40000]),
    (4096, 2049, 5, [4095, 8196, 1, 12000, 7919, 100000]),
])
def test_output_rows_arithmetic(nfft, hop, n_avg, chunks):
    """The definition's row count: row r is complete once (r n_avg + n_avg - 1) hop + nfft items have arrived; a chunk emits the
    rows completed by its items.  (The handle's lora_hip_spectrum_output_rows is held to the same sequence on the device:
    tests/test_gpu_spectrum.py.)"""
    from gr_lora_amd import spectrum
    total, seen = 0, 0
    for c in chunks:
        total += c
        rows = spectrum.output_rows(total, nfft, hop, n_avg)
        brute = 0
        while (brute * n_avg + n_avg - 1) * hop + nfft <= total:
            brute += 1
        assert rows == brute
        assert rows - seen >= 0
        seen = rows
    assert seen == spectrum.output_rows(sum(chunks), nfft, hop, n_avg)
