"""CPU: the C ABI of the IQ conditioner (include/lora_hip_conditioner.h) - exports, argument checks before any device call, the
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


def _cfg(block=4096, window=16, flags=3, device=0):
    from gr_lora_amd import capi
    return capi.ConditionerConfig(struct_size=C.sizeof(capi.ConditionerConfig), block=block, window=window, flags=flags, device=device)


def _create(lib, cfg):
    h = C.c_void_p()
    st = lib.lora_hip_conditioner_create(C.byref(cfg), C.byref(h))
    if st == 0:
        lib.lora_hip_conditioner_destroy(h)
    return st, h


def test_every_declared_symbol_is_listed_and_exported(lib):
    from gr_lora_amd import capi
    hdr = open(os.path.join(ROOT, "include", "lora_hip_conditioner.h")).read()
    declared = set(re.findall(r"\b(lora_hip_conditioner_[a-z_]+)\s*\(", hdr))
    assert declared == set(capi.EXPORTS_CONDITIONER) and len(capi.EXPORTS_CONDITIONER) == len(set(capi.EXPORTS_CONDITIONER))
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (lora_hip_conditioner_[a-z_]+)", out))
    assert declared <= exported
    for name in declared:
        assert getattr(lib, name) is not None
    others = set(capi.EXPORTS + capi.EXPORTS_CHANNELIZER + capi.EXPORTS_FILTERBANK + capi.EXPORTS_GATEWAY + capi.EXPORTS_TX + capi.EXPORTS_LINK +
                 capi.EXPORTS_SPECTRUM + capi.EXPORTS_RESAMPLER)
    assert not set(capi.EXPORTS_CONDITIONER) & others
    for want in ("create", "destroy", "last_error", "output_items", "run_device", "run_device_raw", "work", "work_raw", "flush_device", "flush", "reset",
                 "set_fixed", "set_adaptive", "block_records", "get_plan", "last_kernel_ms"):
        assert "lora_hip_conditioner_" + want in declared


def test_config_struct_and_limits_match_the_header():
    """ConditionerConfig's fields in the header's order, and the header's limits are those of gr_lora_amd/conditioner.py."""
    from gr_lora_amd import capi, conditioner
    hdr = open(os.path.join(ROOT, "include", "lora_hip_conditioner.h")).read()
    body = hdr[hdr.index("typedef struct lora_hip_conditioner_config {"):hdr.index("} lora_hip_conditioner_config_t;")]
    names = re.findall(r"\*?(\w+);", body)
    assert names == [f[0] for f in capi.ConditionerConfig._fields_] == ["struct_size", "block", "window", "flags", "device"]
    defs = {k: int(v) for k, v in re.findall(r"#define LORA_HIP_CONDITIONER_(\w+) (\d+)u", hdr)}
    assert defs == dict(MIN_BLOCK=conditioner.MIN_BLOCK, MAX_BLOCK=conditioner.MAX_BLOCK, MAX_WINDOW=conditioner.MAX_WINDOW,
                        FLAG_DC=capi.CONDITIONER_FLAG_DC, FLAG_IQ=capi.CONDITIONER_FLAG_IQ)
    assert defs == dict(MIN_BLOCK=256, MAX_BLOCK=65536, MAX_WINDOW=256, FLAG_DC=1, FLAG_IQ=2)
    assert (conditioner.DEFAULT_BLOCK, conditioner.DEFAULT_WINDOW) == (4096, 16)


@pytest.mark.parametrize("change", [
    dict(block=128), dict(block=255), dict(block=257), dict(block=3000), dict(block=65537), dict(block=131072), dict(block=1 << 31),   # a power of two, 256 .. 65536
    dict(window=257), dict(window=0xffffffff),                                                                                       # 1 .. 256
    dict(flags=4), dict(flags=0x80000003),                                                                                           # unknown bits
])
def test_bad_config_fails_before_any_device_call(lib, change):
    from gr_lora_amd import conditioner
    st, h = _create(lib, _cfg(**change))
    assert st == ERR_BAD_CONFIG and not h.value
    if "flags" not in change:                                               # the float64 definition refuses the same
        kw = dict(block=4096, window=16)
        kw.update(change)
        with pytest.raises(ValueError):
            conditioner.check(**kw)


def test_null_and_short_struct(lib):
    from gr_lora_amd import capi
    h = C.c_void_p()
    assert lib.lora_hip_conditioner_create(None, C.byref(h)) == ERR_ARG
    cfg = _cfg()
    assert lib.lora_hip_conditioner_create(C.byref(cfg), None) == ERR_ARG
    cfg.struct_size = C.sizeof(capi.ConditionerConfig) - 1
    assert lib.lora_hip_conditioner_create(C.byref(cfg), C.byref(h)) == ERR_ARG and not h.value


def test_every_entry_point_on_a_null_handle(lib):
    n, first = C.c_size_t(0), C.c_uint64(0)
    a, b, c, d = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    assert lib.lora_hip_conditioner_output_items(None, 100000) == 0
    assert lib.lora_hip_conditioner_last_error(None) == b"null handle"
    assert lib.lora_hip_conditioner_last_kernel_ms(None) == 0.0
    assert lib.lora_hip_conditioner_reset(None) == ERR_ARG
    assert lib.lora_hip_conditioner_set_fixed(None, 0.0, 0.0, 0.0, 1.0) == ERR_ARG
    assert lib.lora_hip_conditioner_set_adaptive(None) == ERR_ARG
    assert lib.lora_hip_conditioner_get_plan(None, C.byref(a), C.byref(b), C.byref(c), C.byref(d)) == ERR_ARG
    assert lib.lora_hip_conditioner_block_records(None, None, None, 0, C.byref(n), None, None) == ERR_ARG
    assert lib.lora_hip_conditioner_run_device(None, None, 0, None, 0, C.byref(n), C.byref(first), None) == ERR_ARG
    assert lib.lora_hip_conditioner_run_device_raw(None, None, 0, 1, 0.0, None, 0, C.byref(n), C.byref(first), None) == ERR_ARG
    assert lib.lora_hip_conditioner_work(None, None, 0, None, 0, C.byref(n), C.byref(first)) == ERR_ARG
    assert lib.lora_hip_conditioner_work_raw(None, None, 0, 1, 0.0, None, 0, C.byref(n), C.byref(first)) == ERR_ARG
    assert lib.lora_hip_conditioner_flush_device(None, None, 0, C.byref(n), C.byref(first), None) == ERR_ARG
    assert lib.lora_hip_conditioner_flush(None, None, 0, C.byref(n), C.byref(first)) == ERR_ARG
    lib.lora_hip_conditioner_destroy(None)


def test_a_larger_struct_size_is_accepted(lib):
    """struct_size is a lower bound (ABI growth): a caller built against a longer struct gets the same answer as the exact one."""
    import torch
    want = 0 if torch.cuda.is_available() else ERR_NO_DEVICE
    cfg = _cfg()
    cfg.struct_size = C.sizeof(type(cfg)) + 16
    st, h = _create(lib, cfg)
    assert st == want


def test_valid_arguments_create_only_with_a_device(lib):
    """No CPU fallback: valid arguments give LORA_HIP_ERR_NO_DEVICE without a GPU, a handle with one.  Zero for block or window asks
    for the default; both ends of both ranges and every combination of the two flags are inside the limits."""
    import torch
    from gr_lora_amd import capi
    gpu = torch.cuda.is_available()
    for kw in (dict(), dict(block=0, window=0), dict(block=256, window=1), dict(block=65536, window=256), dict(flags=0), dict(flags=1), dict(flags=2)):
        st, h = _create(lib, _cfg(**kw))
        assert st == (0 if gpu else ERR_NO_DEVICE) and bool(h.value) == gpu, kw
    assert _create(lib, _cfg(device=-1))[0] == ERR_NO_DEVICE
    if not gpu:
        with pytest.raises(capi.LoraHipError):
            capi.Conditioner()
