"""CPU: the C ABI of the rational resampler (include/lora_hip_resampler.h) - exports, argument checks before any device call, the
limits of the header against those of the float64 definition, and no CPU fallback."""
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


def _cfg(L=5, M=6, Z=16, beta=8.0, cutoff=0.8, device=0, flags=0):
    from gr_lora_amd import capi
    return capi.ResamplerConfig(struct_size=C.sizeof(capi.ResamplerConfig), interpolation=L, decimation=M, zero_crossings=Z, beta=beta, cutoff=cutoff,
                                device=device, flags=flags)


def _create(lib, cfg):
    h = C.c_void_p()
    st = lib.lora_hip_resampler_create(C.byref(cfg), C.byref(h))
    if st == 0:
        lib.lora_hip_resampler_destroy(h)
    return st, h


def test_every_declared_symbol_is_listed_and_exported(lib):
    from gr_lora_amd import capi
    hdr = open(os.path.join(ROOT, "include", "lora_hip_resampler.h")).read()
    declared = set(re.findall(r"\b(lora_hip_resampler_[a-z_]+)\s*\(", hdr))
    assert declared == set(capi.EXPORTS_RESAMPLER) and len(capi.EXPORTS_RESAMPLER) == len(set(capi.EXPORTS_RESAMPLER))
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (lora_hip_resampler_[a-z_]+)", out))
    assert declared <= exported
    for name in declared:
        assert getattr(lib, name) is not None
    others = set(capi.EXPORTS + capi.EXPORTS_CHANNELIZER + capi.EXPORTS_FILTERBANK + capi.EXPORTS_GATEWAY + capi.EXPORTS_TX + capi.EXPORTS_LINK +
                 capi.EXPORTS_SPECTRUM)
    assert not set(capi.EXPORTS_RESAMPLER) & others
    for want in ("create", "destroy", "last_error", "taps", "ratio", "delay", "output_items", "run_device", "run_device_raw", "work", "work_raw", "reset",
                 "last_kernel_ms", "get_plan"):
        assert "lora_hip_resampler_" + want in declared


def test_config_struct_and_limits_match_the_header():
    """ResamplerConfig's fields in the header's order (the ctypes layout is the C layout of the same member list), and the
    header's limits are those of gr_lora_amd/resampler.py."""
    from gr_lora_amd import capi, resampler
    hdr = open(os.path.join(ROOT, "include", "lora_hip_resampler.h")).read()
    body = hdr[hdr.index("typedef struct lora_hip_resampler_config {"):hdr.index("} lora_hip_resampler_config_t;")]
    names = re.findall(r"\*?(\w+);", body)
    assert names == [f[0] for f in capi.ResamplerConfig._fields_]
    assert names == ["struct_size", "interpolation", "decimation", "zero_crossings", "beta", "cutoff", "device", "flags"]
    assert capi.ResamplerConfig.beta.size == 8 and capi.ResamplerConfig.cutoff.size == 8
    limits = {k: int(v) for k, v in re.findall(r"#define LORA_HIP_RESAMPLER_(\w+) (\d+)u", hdr)}
    assert limits == dict(MAX_RATIO=resampler.MAX_RATIO, MIN_ZERO_CROSSINGS=resampler.MIN_ZERO_CROSSINGS, MAX_ZERO_CROSSINGS=resampler.MAX_ZERO_CROSSINGS,
                          MAX_BETA=resampler.MAX_BETA, MAX_TAPS=resampler.MAX_TAPS, MAX_Q=resampler.MAX_Q)
    assert limits == dict(MAX_RATIO=512, MIN_ZERO_CROSSINGS=2, MAX_ZERO_CROSSINGS=32, MAX_BETA=20, MAX_TAPS=16385, MAX_Q=1024)


@pytest.mark.parametrize("change", [
    dict(L=0), dict(M=0), dict(L=513), dict(M=513), dict(L=1026, M=1024),   # 1 .. 512, as given
    dict(Z=1), dict(Z=33),                                                  # 2 .. 32
    dict(beta=-0.5), dict(beta=float("nan")), dict(beta=20.5),              # 0 .. 20
    dict(cutoff=0.0), dict(cutoff=1.5), dict(cutoff=-0.8), dict(cutoff=float("nan")),   # (0, 1]
    dict(L=1, M=40),                                                        # Q = 1281 > 1024
    dict(L=1, M=256, Z=2),                                                  # Q = 1025
    dict(L=511, M=512, Z=32),                                               # ntaps = 32769 > 16385
    dict(L=512, M=511, Z=17),                                               # ntaps = 17409
    dict(flags=1), dict(flags=0x80000000),                                  # reserved
])
def test_bad_config_fails_before_any_device_call(lib, change):
    from gr_lora_amd import resampler
    st, h = _create(lib, _cfg(**change))
    assert st == ERR_BAD_CONFIG and not h.value
    if "flags" not in change:                                               # the float64 definition refuses the same designs
        kw = dict(L=5, M=6, Z=16, beta=8.0, cutoff=0.8)
        kw.update(change)
        with pytest.raises(ValueError):
            resampler.design(kw["L"], kw["M"], kw["Z"], kw["beta"], kw["cutoff"])


def test_null_and_short_struct(lib):
    from gr_lora_amd import capi
    h = C.c_void_p()
    assert lib.lora_hip_resampler_create(None, C.byref(h)) == ERR_ARG
    cfg = _cfg()
    assert lib.lora_hip_resampler_create(C.byref(cfg), None) == ERR_ARG
    cfg.struct_size = C.sizeof(capi.ResamplerConfig) - 1
    assert lib.lora_hip_resampler_create(C.byref(cfg), C.byref(h)) == ERR_ARG and not h.value


def test_every_entry_point_on_a_null_handle(lib):
    n, first = C.c_size_t(0), C.c_uint64(0)
    a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    assert lib.lora_hip_resampler_output_items(None, 100000) == 0
    assert lib.lora_hip_resampler_last_error(None) == b"null handle"
    assert lib.lora_hip_resampler_last_kernel_ms(None) == 0.0
    assert lib.lora_hip_resampler_delay(None) == 0.0
    assert lib.lora_hip_resampler_reset(None) == ERR_ARG
    assert lib.lora_hip_resampler_taps(None, None, 0, C.byref(n)) == ERR_ARG
    assert lib.lora_hip_resampler_ratio(None, C.byref(a), C.byref(b), C.byref(c)) == ERR_ARG
    assert lib.lora_hip_resampler_get_plan(None, C.byref(a), C.byref(b), C.byref(c), C.byref(n)) == ERR_ARG
    assert lib.lora_hip_resampler_run_device(None, None, 0, None, 0, C.byref(n), C.byref(first), None) == ERR_ARG
    assert lib.lora_hip_resampler_run_device_raw(None, None, 0, 1, 0.0, None, 0, C.byref(n), C.byref(first), None) == ERR_ARG
    assert lib.lora_hip_resampler_work(None, None, 0, None, 0, C.byref(n), C.byref(first)) == ERR_ARG
    assert lib.lora_hip_resampler_work_raw(None, None, 0, 1, 0.0, None, 0, C.byref(n), C.byref(first)) == ERR_ARG
    lib.lora_hip_resampler_destroy(None)


def test_a_larger_struct_size_is_accepted(lib):
    """struct_size is a lower bound (ABI growth): a caller built against a longer struct gets the same answer as the exact one."""
    import torch
    want = 0 if torch.cuda.is_available() else ERR_NO_DEVICE
    cfg = _cfg()
    cfg.struct_size = C.sizeof(type(cfg)) + 16
    st, h = _create(lib, cfg)
    assert st == want


def test_valid_arguments_create_only_with_a_device(lib):
    """No CPU fallback: valid arguments give LORA_HIP_ERR_NO_DEVICE without a GPU, a handle with one.  Zero for zero_crossings or
    beta asks for the default; the largest table, the longest chain and an unreduced ratio are inside the limits."""
    import torch
    from gr_lora_amd import capi
    gpu = torch.cuda.is_available()
    for kw in (dict(), dict(Z=0, beta=0.0), dict(L=512, M=511), dict(L=1, M=31), dict(L=1, M=255, Z=2), dict(L=500, M=512, Z=32, beta=20.0, cutoff=1.0),
               dict(L=1, M=1, Z=2), dict(L=512, M=1)):
        st, h = _create(lib, _cfg(**kw))
        assert st == (0 if gpu else ERR_NO_DEVICE) and bool(h.value) == gpu, kw
    assert _create(lib, _cfg(device=-1))[0] == ERR_NO_DEVICE
    if not gpu:
        with pytest.raises(capi.LoraHipError):
            capi.Resampler(5, 6)
