"""CPU: the C ABI of the link metrics (include/lora_hip_link.h) - exports, struct layouts against the C compiler's, argument
checks before any device call - and what it must leave alone: the two older public headers and their ABI version."""
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
    hdr = open(os.path.join(ROOT, "include", "lora_hip_link.h")).read()
    declared = set(re.findall(r"\b(lora_hip_link_[a-z_]+)\s*\(", hdr))
    assert declared == set(capi.EXPORTS_LINK) and len(capi.EXPORTS_LINK) == len(set(capi.EXPORTS_LINK))
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (lora_hip_link_[a-z_]+)", out))
    assert declared == exported
    for name in declared:
        assert getattr(lib, name) is not None
    others = set(capi.EXPORTS + capi.EXPORTS_CHANNELIZER + capi.EXPORTS_FILTERBANK + capi.EXPORTS_GATEWAY + capi.EXPORTS_TX)
    assert not set(capi.EXPORTS_LINK) & others
    # the kernel's launch interface is internal: no C symbol of it
    assert not re.findall(r" T (launch_link[a-z_]*)", out)


def test_older_headers_name_nothing_of_it(lib):
    for name in ("lora_hip.h", "lora_hip_gateway.h", "lora_hip_filterbank.h", "lora_hip_channelizer.h", "lora_hip_tx.h"):
        assert "lora_hip_link" not in open(os.path.join(ROOT, "include", name)).read(), name
    assert lib.lora_hip_abi_version() == 4
    hdr = open(os.path.join(ROOT, "include", "lora_hip_link.h")).read()
    from gr_lora_amd import capi, linkmetrics
    assert re.search(r"#define LORA_HIP_LINK_WINDOWS %du" % linkmetrics.WINDOWS, hdr)
    assert re.search(r"#define LORA_HIP_LINK_LOBE %d\b" % linkmetrics.LOBE, hdr)
    for name, v in (("PREAMBLE", capi.LINK_FLAG_PREAMBLE), ("SYNC", capi.LINK_FLAG_SYNC), ("SFD", capi.LINK_FLAG_SFD)):
        assert re.search(r"#define LORA_HIP_LINK_FLAG_%s %du" % (name, v), hdr)
    assert (capi.LINK_FLAG_PREAMBLE, capi.LINK_FLAG_SYNC, capi.LINK_FLAG_SFD) == (linkmetrics.FLAG_PREAMBLE, linkmetrics.FLAG_SYNC, linkmetrics.FLAG_SFD)


def test_structs_match_the_c_layout(tmp_path):
    from gr_lora_amd import capi
    structs = [("lora_hip_link_window_t", capi.LinkWindow), ("lora_hip_link_metrics_t", capi.LinkMetrics), ("lora_hip_link_request_t", capi.LinkRequest)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lora_hip_link.h"', "int main(void) {"]
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
    assert C.sizeof(capi.LinkWindow) == 24


def test_null_arguments(lib):
    from gr_lora_amd import capi
    n = C.c_size_t(7)
    met, info, ginfo = capi.LinkMetrics(), capi.FrameInfo(), capi.GatewayFrameInfo()
    off, ln = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(4096)
    req = (capi.LinkRequest * 1)()
    buf = (C.c_uint8 * 320)()
    assert lib.lora_hip_link_measure_device(None, C.c_void_p(4096), 4096, off, ln, 1, req, 1, C.byref(met), None, None) == ERR_ARG
    assert lib.lora_hip_link_enable(None, 1) == ERR_ARG
    assert lib.lora_hip_link_poll_frame(None, buf, 320, C.byref(n), C.byref(info), C.byref(met)) == ERR_ARG
    assert lib.lora_hip_link_drain_frames(None, buf, 320, C.byref(info), C.byref(met), 1, C.byref(n)) == ERR_ARG
    assert lib.lora_hip_link_mux_enable(None, 1) == ERR_ARG
    assert lib.lora_hip_link_mux_poll_frame(None, buf, 320, C.byref(n), C.byref(info), C.byref(met)) == ERR_ARG
    assert lib.lora_hip_link_gateway_enable(None, 1) == ERR_ARG
    assert lib.lora_hip_link_gateway_poll_frame(None, buf, 320, C.byref(n), C.byref(ginfo), C.byref(met)) == ERR_ARG
    assert lib.lora_hip_link_stats(None, None, None, None) == ERR_ARG
    assert n.value == 7


def test_combine_argument_checks(lib):
    from gr_lora_amd import capi
    w, out = (capi.LinkWindow * 6)(), capi.LinkMetrics()
    assert lib.lora_hip_link_combine(None, 1024, 128, 125000.0, C.byref(out)) == ERR_ARG
    assert lib.lora_hip_link_combine(w, 1024, 128, 125000.0, None) == ERR_ARG
    for sps, N in ((1000, 128), (1024, 100), (64, 128), (1024, 8), (0, 0)):
        assert lib.lora_hip_link_combine(w, sps, N, 125000.0, C.byref(out)) == ERR_ARG, (sps, N)
    assert lib.lora_hip_link_combine(w, 1024, 128, 125000.0, C.byref(out)) == 0
    assert out.flags == 0 and out.rssi_dbfs == -200.0


def test_handle_wrappers_need_a_device():
    """No CPU fallback: the Python classes that would turn link metrics on cannot be made without a GPU."""
    import torch
    from gr_lora_amd import capi, lora
    if not torch.cuda.is_available():
        with pytest.raises(capi.LoraHipError):
            lora.decoder(1e6, 125000, 7, False, 4, True, verbose=False, link_metrics=True)
