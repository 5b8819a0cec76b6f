"""CPU: the C ABI of the channeliser (include/lora_hip_channelizer.h) - exports, struct layout, argument checks before any device
call (among them the design's size: tap count and staged tile), and no CPU fallback."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_BAD_CONFIG, ERR_NO_DEVICE, ERR_ARG = -2, -3, -6
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    from gr_lora_amd import build, capi
    build.build_library()
    return capi.load()


def _cfg(channels=(868.1e6,), fs=1e6, D=1, **kw):
    from gr_lora_amd import capi
    arr = (C.c_float * max(len(channels), 1))(*channels)
    cfg = capi.ChannelizerConfig(struct_size=C.sizeof(capi.ChannelizerConfig), samp_rate=fs, center_freq=868.0e6, channel_list=arr,
                                 n_channels=len(channels), bandwidth=125000, decimation=D, device=0, **kw)
    return cfg, arr


def _create(lib, cfg):
    h = C.c_void_p()
    st = lib.lora_hip_channelizer_create(C.byref(cfg), C.byref(h))
    if st == 0:
        lib.lora_hip_channelizer_destroy(h)
    return st, h


def test_every_declared_symbol_is_listed_and_exported(lib):
    from gr_lora_amd import capi
    hdr = open(os.path.join(ROOT, "include", "lora_hip_channelizer.h")).read()
    declared = set(re.findall(r"\b(lora_hip_channelizer_[a-z_]+)\s*\(", hdr))
    assert declared == set(capi.EXPORTS_CHANNELIZER)
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (lora_hip_channelizer_[a-z_]+)", out))
    assert declared <= exported
    for name in declared:
        assert getattr(lib, name) is not None
    assert not set(capi.EXPORTS_CHANNELIZER) & set(capi.EXPORTS + capi.EXPORTS_FILTERBANK)


def test_config_struct_matches_the_header():
    """ChannelizerConfig's fields in the header's order (the ctypes layout is the C layout of the same member list)."""
    from gr_lora_amd import capi
    hdr = open(os.path.join(ROOT, "include", "lora_hip_channelizer.h")).read()
    body = hdr[hdr.index("typedef struct lora_hip_channelizer_config {"):hdr.index("} lora_hip_channelizer_config_t;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\*?(\w+);", body)
    assert names == [f[0] for f in capi.ChannelizerConfig._fields_]
    assert capi.ChannelizerConfig.samp_rate.size == 4 and capi.ChannelizerConfig.cutoff_hz.size == 4
    assert capi.CHANNELIZER_FLAG_UINT32_OFFSET == int(re.search(r"#define LORA_HIP_CHANNELIZER_FLAG_UINT32_OFFSET (\d+)u", hdr).group(1))


@pytest.mark.parametrize("change", [
    dict(channels=()),
    dict(D=0),
    dict(D=65),
    dict(fs=0.0),
    dict(fs=-1e6),
    dict(fs=NAN),
    dict(fs=INF),
    dict(cutoff_hz=-1.0),
    dict(cutoff_hz=NAN),
    dict(cutoff_hz=INF),
    dict(transition_hz=-1.0),
    dict(transition_hz=NAN),
    dict(transition_hz=INF),
    dict(flags=2),
    dict(flags=0x80000001),
    dict(transition_hz=1e-3),                # 53 fs / (22 tw) = 2.4e9 taps: does not fit an int
    dict(transition_hz=100.0),               # 24 090 taps: above LORA_HIP_CHANNELIZER_MAX_TAPS
    dict(transition_hz=1.3e6),               # 53 fs / (22 tw) = 1.85: one tap, its Hamming window 0 / 0
    dict(transition_hz=2.5e6),               # ... = 0.96: no tap at all
    dict(D=64, transition_hz=500.0),         # 4 819 taps, tile of 16 384: (21 215 + 1 325 + 1) * 8 = 180 328 bytes of LDS
    dict(D=64, transition_hz=800.0),         # 3 011 taps: 164 960 bytes
    dict(D=1, transition_hz=150.0),          # 16 061 taps, tile of 4 096: 171 352 bytes
])
def test_bad_arguments_fail_before_any_device_call(lib, change):
    cfg, keep = _cfg(**change)
    st, h = _create(lib, cfg)
    assert st == ERR_BAD_CONFIG and not h.value


def test_null_and_short_struct(lib):
    from gr_lora_amd import capi
    h = C.c_void_p()
    assert lib.lora_hip_channelizer_create(None, C.byref(h)) == ERR_ARG
    cfg, keep = _cfg()
    assert lib.lora_hip_channelizer_create(C.byref(cfg), None) == ERR_ARG
    cfg.struct_size = capi.ChannelizerConfig.cutoff_hz.offset - 1
    assert lib.lora_hip_channelizer_create(C.byref(cfg), C.byref(h)) == ERR_ARG and not h.value
    cfg2, keep2 = _cfg()
    cfg2.channel_list = C.cast(None, C.POINTER(C.c_float))
    assert lib.lora_hip_channelizer_create(C.byref(cfg2), C.byref(h)) == ERR_BAD_CONFIG and not h.value
    # an old-layout caller: the fields from cutoff_hz on are not read, whatever they hold
    cfg3, keep3 = _cfg(cutoff_hz=NAN, transition_hz=-1.0, flags=0xFFFFFFFF)
    cfg3.struct_size = capi.ChannelizerConfig.cutoff_hz.offset
    st, h3 = _create(lib, cfg3)
    assert st in (0, ERR_NO_DEVICE)
    # the handle-less calls
    n = C.c_size_t(0)
    assert lib.lora_hip_channelizer_output_items(None, 100) == 0
    assert lib.lora_hip_channelizer_last_error(None) == b"null handle"
    assert lib.lora_hip_channelizer_last_kernel_ms(None) == 0.0
    assert lib.lora_hip_channelizer_taps(None, None, 0, C.byref(n)) == ERR_ARG
    assert lib.lora_hip_channelizer_run_device(None, None, 0, None, 0, C.byref(n), None) == ERR_ARG
    assert lib.lora_hip_channelizer_work(None, None, 0, None, 0, C.byref(n)) == ERR_ARG
    assert lib.lora_hip_channelizer_apply_cfo(None, 1.0) == ERR_ARG
    lib.lora_hip_channelizer_destroy(None)


def test_valid_arguments_create_only_with_a_device(lib):
    """No CPU fallback: valid arguments give LORA_HIP_ERR_NO_DEVICE without a GPU, a handle with one.  Among them the designs
    just inside each limit of test_bad_arguments_fail_before_any_device_call."""
    import torch
    from gr_lora_amd import capi
    gpu = torch.cuda.is_available()
    for kw in (dict(), dict(channels=(867.9e6, 868.1e6, 868.3e6), D=64), dict(cutoff_hz=200e3, transition_hz=100e3),
               dict(flags=capi.CHANNELIZER_FLAG_UINT32_OFFSET),
               dict(transition_hz=1.2e6),              # 53 fs / (22 tw) = 2.008: 3 taps
               dict(D=64, transition_hz=1000.0),       # 2 409 taps: 159 792 bytes of LDS
               dict(D=1, transition_hz=160.0)):        # 15 057 taps: 162 920 bytes
        cfg, keep = _cfg(**kw)
        st, h = _create(lib, cfg)
        assert st == (0 if gpu else ERR_NO_DEVICE) and bool(h.value) == gpu, kw
    if not gpu:
        with pytest.raises(capi.LoraHipError):
            capi.Channelizer(1e6, 868.0e6, [868.1e6], 125000, 1)
