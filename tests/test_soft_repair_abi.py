"""CPU: the C ABI of the CRC-aided repair (include/lora_hip_soft.h) - exports, the record's layout against the C compiler's, argument errors
before any device call or any look at the handle - and that the ABI version and the report struct are what they were."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -6
NEW = ["lora_hip_soft_crc_repair_enable", "lora_hip_soft_crc_repair_results", "lora_hip_soft_crc_repair_codewords"]


@pytest.fixture(scope="module")
def lib():
    from gr_lora_amd import build, capi
    build.build_library()
    return capi.load()


def test_exports(lib):
    from gr_lora_amd import capi
    hdr = open(os.path.join(ROOT, "include", "lora_hip_soft.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    for name in NEW:
        assert name in capi.EXPORTS_SOFT and re.search(r"lora_hip_status %s\(" % name, hdr) and re.search(r" T %s\n" % name, out)
        assert getattr(lib, name).argtypes is not None and not re.search(r"\d", name)
    assert not re.findall(r" T (launch_soft[a-z_]*)", out) and "soft_repair_kernel" not in re.findall(r" T (\S+)", out)
    assert lib.lora_hip_abi_version() == 4


def test_constants_agree():
    from gr_lora_amd import capi, softdecode as SD
    hdr = open(os.path.join(ROOT, "include", "lora_hip_soft.h")).read()
    for name, v, m in (("NOT_ATTEMPTED", capi.SOFT_REPAIR_NOT_ATTEMPTED, SD.REPAIR_NOT_ATTEMPTED), ("CRC_HELD", capi.SOFT_REPAIR_CRC_HELD, SD.REPAIR_CRC_HELD),
                       ("REPAIRED", capi.SOFT_REPAIR_REPAIRED, SD.REPAIR_REPAIRED), ("FAILED", capi.SOFT_REPAIR_FAILED, SD.REPAIR_FAILED),
                       ("MAX_CANDIDATES", capi.SOFT_REPAIR_MAX_CANDIDATES, SD.REPAIR_MAX_CANDIDATES)):
        assert re.search(r"#define LORA_HIP_SOFT_REPAIR_%s %du" % (name, v), hdr) and v == m, name


def _layout(tmp_path, cname, cls):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lora_hip_soft.h"', "int main(void) {", 'printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    for f in cls._fields_:
        lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    lines.append("return 0; }")
    src = tmp_path / ("%s.c" % cname)
    src.write_text("\n".join(lines))
    exe = tmp_path / cname
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    return dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())


def test_record_matches_the_c_layout(tmp_path):
    from gr_lora_amd import capi
    got = _layout(tmp_path, "lora_hip_soft_repair_t", capi.SoftRepair)
    assert int(got["lora_hip_soft_repair_t"]) == C.sizeof(capi.SoftRepair) == 40
    for f in capi.SoftRepair._fields_:
        assert int(got["lora_hip_soft_repair_t.%s" % f[0]]) == getattr(capi.SoftRepair, f[0]).offset, f[0]
    assert [f[0] for f in capi.SoftRepair._fields_] == ["status", "candidates", "pattern", "changed", "syndrome", "reserved", "penalty", "codeword"]
    assert capi.SoftRepair.codeword.size == 16 and capi.SoftRepair.penalty.offset == 20
    # the report struct is what it was
    got = _layout(tmp_path, "lora_hip_soft_report_t", capi.SoftReport)
    assert int(got["lora_hip_soft_report_t"]) == C.sizeof(capi.SoftReport) == 36


def test_record_as_dict_has_the_models_keys():
    from gr_lora_amd import capi, softdecode as SD
    r = capi.SoftRepair()
    r.status, r.candidates, r.pattern, r.changed, r.syndrome, r.penalty = 2, 3, 5, 2, 0xbeef, 0.75
    r.codeword[0], r.codeword[1], r.codeword[2] = 9, 4, 513
    d = r.as_dict()
    assert set(d) == set(SD.no_repair()) and d["codewords"] == [9, 4, 513] and d["syndrome"] == 0xbeef and d["penalty"] == 0.75
    assert capi.SoftRepair().as_dict() == SD.no_repair(dtype=__import__("numpy").float32)


def test_argument_errors_come_before_any_device_call(lib):
    """with a handle that is no handle: every one of these is refused before the handle is looked at"""
    from gr_lora_amd import capi
    h = C.c_void_p(4096)
    rec = (capi.SoftRepair * 2)()
    rec[0].status = 77
    assert lib.lora_hip_soft_crc_repair_enable(None, 8) == ERR_ARG
    assert lib.lora_hip_soft_crc_repair_enable(h, 9) == ERR_ARG
    assert lib.lora_hip_soft_crc_repair_enable(h, 0xffffffff) == ERR_ARG
    assert lib.lora_hip_soft_crc_repair_results(None, rec, 0) == ERR_ARG
    assert lib.lora_hip_soft_crc_repair_results(h, None, 1) == ERR_ARG          # a null out
    ln = (C.c_uint32 * 1)(1)
    nib, sec = (C.c_uint8 * 6)(), (C.c_uint8 * 6)(*([1] * 6))
    mar = (C.c_float * 6)()
    out = (C.c_uint8 * 3)(9, 9, 9)
    args = lambda **kw: [kw.get("h", h), 1, kw.get("ln", ln), kw.get("nib", nib), kw.get("sec", sec), kw.get("mar", mar), kw.get("cand", 8), kw.get("out", out),
                         kw.get("rec", rec), None]
    for bad in (dict(h=None), dict(cand=9), dict(cand=0), dict(ln=None), dict(nib=None), dict(sec=None), dict(mar=None), dict(out=None), dict(rec=None)):
        assert lib.lora_hip_soft_crc_repair_codewords(*args(**bad)) == ERR_ARG, bad
    assert rec[0].status == 77 and bytes(out) == b"\x09\x09\x09"
