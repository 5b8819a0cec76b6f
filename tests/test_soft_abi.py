"""CPU: the C ABI of the soft-decision decoder (include/lora_hip_soft.h) - exports, struct layout against the C compiler's, argument checks
before any device call - and what it must leave alone: the older public headers and their ABI version."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -6


@pytest.fixture(scope="module")
def lib():
    from gr_lora_amd import build, capi
    build.build_library()
    return capi.load()


def test_every_declared_symbol_is_listed_and_exported(lib):
    from gr_lora_amd import capi
    hdr = open(os.path.join(ROOT, "include", "lora_hip_soft.h")).read()
    declared = set(re.findall(r"\b(lora_hip_soft_[a-z_]+)\s*\(", hdr))
    assert declared == set(capi.EXPORTS_SOFT) and len(capi.EXPORTS_SOFT) == len(set(capi.EXPORTS_SOFT))
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (lora_hip_soft_[a-z_]+)", out))
    assert declared == exported
    for name in declared:
        assert getattr(lib, name) is not None
    others = set(capi.EXPORTS + capi.EXPORTS_CHANNELIZER + capi.EXPORTS_FILTERBANK + capi.EXPORTS_GATEWAY + capi.EXPORTS_TX + capi.EXPORTS_LINK +
                 capi.EXPORTS_SPECTRUM + capi.EXPORTS_RESAMPLER + capi.EXPORTS_CONDITIONER)
    assert not set(capi.EXPORTS_SOFT) & others
    # the kernels' launch interface is internal: no C symbol of it
    assert not re.findall(r" T (launch_soft[a-z_]*)", out)


def test_older_headers_name_nothing_of_it(lib):
    from gr_lora_amd import capi, softdecode
    for name in os.listdir(os.path.join(ROOT, "include")):
        if name != "lora_hip_soft.h":
            assert "lora_hip_soft" not in open(os.path.join(ROOT, "include", name)).read().lower(), name
    assert lib.lora_hip_abi_version() == 4
    hdr = open(os.path.join(ROOT, "include", "lora_hip_soft.h")).read()
    assert re.search(r"#define LORA_HIP_SOFT_REQUIRE_HEADER_CHECKSUM %du" % capi.SOFT_REQUIRE_HEADER_CHECKSUM, hdr)
    for name, v, m in (("FRAME", capi.SOFT_FRAME, softdecode.STATUS_FRAME), ("HEADER_REJECTED", capi.SOFT_HEADER_REJECTED, softdecode.STATUS_HEADER_REJECTED),
                       ("CR_ZERO", capi.SOFT_CR_ZERO, softdecode.STATUS_CR_ZERO), ("TRUNCATED", capi.SOFT_TRUNCATED, softdecode.STATUS_TRUNCATED)):
        assert re.search(r"#define LORA_HIP_SOFT_%s %du" % (name, v), hdr) and v == m


def test_struct_matches_the_c_layout(tmp_path):
    from gr_lora_amd import capi
    cname, cls = "lora_hip_soft_report_t", capi.SoftReport
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lora_hip_soft.h"', "int main(void) {", 'printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    for f in cls._fields_:
        lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got[cname]) == C.sizeof(cls) == 36
    for f in cls._fields_:
        assert int(got["%s.%s" % (cname, f[0])]) == getattr(cls, f[0]).offset, f[0]


def test_argument_errors_come_before_any_device_call(lib):
    from gr_lora_amd import capi
    off, ln = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(1 << 20)
    pre, rep = (capi.Preamble * 1)(), (capi.SoftReport * 1)()
    woff = (C.c_int64 * 1)(0)
    llr = (C.c_float * 12)()
    rep[0].status = 77
    p = C.c_void_p(4096)
    assert lib.lora_hip_soft_decode_at_headers_device(None, p, 1 << 20, off, ln, 1, pre, 1, 0, rep, None) == ERR_ARG
    assert lib.lora_hip_soft_symbols_device(None, p, 1 << 20, woff, 1, None, llr, None, None, None) == ERR_ARG
    assert rep[0].status == 77 and llr[0] == 0.0


def test_sf_range_is_stated_and_checked_before_a_handle_is_made():
    """SF 7 .. 12: the header says so, and the receiver refuses SF6 before it asks for a device (the C call's own check needs a handle: tests/test_gpu_soft.py)."""
    from gr_lora_amd import lora
    hdr = open(os.path.join(ROOT, "include", "lora_hip_soft.h")).read()
    assert re.search(r"SF 7\.\.12 only.*SF6.*ERR_BAD_CONFIG before any device call", hdr, re.S)
    for sf in (6, 13):
        with pytest.raises(ValueError):
            lora.weak_signal_receiver(1e6, 125000, sf, 4, True)


def test_receiver_needs_a_device():
    """No CPU fallback: the Python class of the low-SNR receive path cannot be made without a GPU."""
    import torch
    from gr_lora_amd import capi, lora
    if not torch.cuda.is_available():
        with pytest.raises(capi.LoraHipError):
            lora.weak_signal_receiver(1e6, 125000, 7, 4, True)
