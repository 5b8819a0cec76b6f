"""CPU: the C ABI of the transmit side (include/lora_hip_tx.h) - exports, struct layouts against the C compiler's, argument checks
before any device call, no CPU fallback - and the host-only frame encoder against the numpy transmit model (synth.encode_shifts)."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_BAD_SF, ERR_BAD_CONFIG, ERR_NO_DEVICE, ERR_ARG, ERR_OVERFLOW = 0, -1, -2, -3, -6, -7


@pytest.fixture(scope="module")
def lib():
    from gr_lora_amd import build, capi
    build.build_library()
    return capi.load()


def test_every_declared_symbol_is_listed_and_exported(lib):
    from gr_lora_amd import capi
    hdr = open(os.path.join(ROOT, "include", "lora_hip_tx.h")).read()
    declared = set(re.findall(r"\b(lora_hip_tx_[a-z_]+)\s*\(", hdr))
    assert declared == set(capi.EXPORTS_TX) and len(capi.EXPORTS_TX) == len(set(capi.EXPORTS_TX))
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    assert declared <= set(re.findall(r" T (lora_hip_tx_[a-z_]+)", out))
    for name in declared:
        assert getattr(lib, name) is not None
    others = set(capi.EXPORTS + capi.EXPORTS_CHANNELIZER + capi.EXPORTS_FILTERBANK + capi.EXPORTS_GATEWAY)
    assert not set(capi.EXPORTS_TX) & others
    assert re.search(r"#define LORA_HIP_TX_MAX_SHIFTS %du" % capi.TX_MAX_SHIFTS, hdr)
    assert re.search(r"#define LORA_HIP_TX_FRAME_HDR_NIBBLES %du" % capi.TX_FRAME_HDR_NIBBLES, hdr)
    assert re.search(r"#define LORA_HIP_TX_FRAME_CRC_BYTES %du" % capi.TX_FRAME_CRC_BYTES, hdr)


def test_the_receive_header_is_as_it_was(lib):
    """The transmit side has a header of its own: nothing of it in lora_hip.h, whose version stays."""
    hdr = open(os.path.join(ROOT, "include", "lora_hip.h")).read()
    assert "lora_hip_tx" not in hdr
    assert lib.lora_hip_abi_version() == 4


def test_structs_match_the_c_layout(tmp_path):
    """sizeof and offsetof of every member, from the C compiler on the header, against the ctypes structs."""
    from gr_lora_amd import capi
    structs = [("lora_hip_tx_frame_t", capi.TxFrame), ("lora_hip_tx_config_t", capi.TxConfig)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lora_hip_tx.h"', "int main(void) {"]
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


def _encode(lib, f, cap=None):
    from gr_lora_amd import capi
    cap = capi.TX_MAX_SHIFTS if cap is None else cap
    out = (C.c_uint16 * max(cap, 1))()
    nh, npay = C.c_uint32(0), C.c_uint32(0)
    st = lib.lora_hip_tx_encode(C.byref(f), out, cap, C.byref(nh), C.byref(npay))
    return st, nh.value, npay.value


@pytest.mark.parametrize("change,status", [
    (dict(sf=5), ERR_BAD_SF),
    (dict(sf=13), ERR_BAD_SF),
    (dict(cr=0), ERR_BAD_CONFIG),
    (dict(cr=5), ERR_BAD_CONFIG),
    (dict(sf=6), ERR_BAD_CONFIG),              # SF6 with an explicit header
    (dict(length=256), ERR_BAD_CONFIG),
    (dict(flags=4), ERR_BAD_CONFIG),
    (dict(flags=1, hdr_nibbles=(C.c_uint8 * 2)(16, 0)), ERR_BAD_CONFIG),
    (dict(struct_size=8), ERR_ARG),
    (dict(payload=C.cast(None, C.POINTER(C.c_uint8))), ERR_ARG),
])
def test_encoder_argument_checks(lib, change, status):
    from gr_lora_amd import capi
    f = capi.tx_frame(b"abcd", 7, 4, 125000)
    for k, v in change.items():
        setattr(f, k, v)
    assert _encode(lib, f)[0] == status
    n = C.c_uint64(0)
    assert lib.lora_hip_tx_frame_items(C.byref(f), 1e6, C.byref(n)) == status


def test_encoder_null_and_overflow(lib):
    from gr_lora_amd import capi
    f = capi.tx_frame(b"abcd", 7, 4, 125000)
    nh, npay = C.c_uint32(0), C.c_uint32(0)
    assert lib.lora_hip_tx_encode(None, None, 0, C.byref(nh), C.byref(npay)) == ERR_ARG
    assert lib.lora_hip_tx_encode(C.byref(f), None, 0, None, C.byref(npay)) == ERR_ARG
    assert lib.lora_hip_tx_encode(C.byref(f), None, 0, C.byref(nh), C.byref(npay)) == OK and nh.value == 8 and npay.value > 0
    st, nh2, np2 = _encode(lib, f, cap=8 + npay.value - 1)
    assert st == ERR_OVERFLOW and (nh2, np2) == (8, npay.value)
    assert lib.lora_hip_tx_frame_items(C.byref(f), 1e6, None) == ERR_ARG
    assert lib.lora_hip_tx_frame_items(None, 1e6, C.byref(C.c_uint64(0))) == ERR_ARG


@pytest.mark.parametrize("fs,change", [
    (1e6 + 1, dict()),                       # fs / bw no integer
    (100e3, dict()),                         # below 1
    (125000.0 * 1025, dict()),               # above the limit
    (1e6, dict(bandwidth=0)),
    (1e6, dict(preamble_len=1025)),
])
def test_frame_items_refuses_rates_the_kernel_does_not_take(lib, fs, change):
    from gr_lora_amd import capi
    f = capi.tx_frame(b"abcd", 7, 4, 125000)
    for k, v in change.items():
        setattr(f, k, v)
    assert lib.lora_hip_tx_frame_items(C.byref(f), fs, C.byref(C.c_uint64(0))) == ERR_BAD_CONFIG


def test_frame_items_takes_the_largest_symbol(lib):
    """Decimation 1024 at SF12: 2^22 items per symbol, the limit."""
    from gr_lora_amd import capi
    f = capi.tx_frame(b"abcd", 12, 4, 125000)
    n_pay = len(capi.tx_encode(f)[1])
    assert capi.tx_frame_items(f, 125000.0 * 1024) == (8 + 4 + 8 + n_pay) * (1 << 22) + (1 << 20)


def _cfg(**kw):
    from gr_lora_amd import capi
    cfg = capi.TxConfig(struct_size=C.sizeof(capi.TxConfig), device=0, samp_rate=2e6, noise_sigma=0.0, seed=1, flags=0)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


@pytest.mark.parametrize("change,status", [
    (dict(struct_size=8), ERR_ARG),
    (dict(device=-1), ERR_ARG),
    (dict(samp_rate=0.0), ERR_BAD_CONFIG),
    (dict(samp_rate=-1e6), ERR_BAD_CONFIG),
    (dict(samp_rate=float("nan")), ERR_BAD_CONFIG),
    (dict(samp_rate=float("inf")), ERR_BAD_CONFIG),
    (dict(noise_sigma=-1.0), ERR_BAD_CONFIG),
    (dict(noise_sigma=float("nan")), ERR_BAD_CONFIG),
    (dict(flags=1), ERR_BAD_CONFIG),
])
def test_bad_config_fails_before_any_device_call(lib, change, status):
    h = C.c_void_p()
    assert lib.lora_hip_tx_create(C.byref(_cfg(**change)), C.byref(h)) == status and not h.value


def test_null_arguments(lib):
    h = C.c_void_p()
    assert lib.lora_hip_tx_create(None, C.byref(h)) == ERR_ARG
    assert lib.lora_hip_tx_create(C.byref(_cfg()), None) == ERR_ARG
    assert lib.lora_hip_tx_last_error(None) == b"null handle"
    assert lib.lora_hip_tx_add_frames(None, None, 0) == ERR_ARG
    assert lib.lora_hip_tx_generate_device(None, None, 0, None) == ERR_ARG
    assert lib.lora_hip_tx_generate_device_raw(None, None, 0, 1, 1.0, None) == ERR_ARG
    assert lib.lora_hip_tx_generate(None, None, 0) == ERR_ARG
    assert lib.lora_hip_tx_position(None) == 0 and lib.lora_hip_tx_pending(None) == 0 and lib.lora_hip_tx_last_kernel_ms(None) == 0.0
    lib.lora_hip_tx_destroy(None)


def test_valid_config_creates_only_with_a_device(lib):
    """No CPU fallback: a valid config gives LORA_HIP_ERR_NO_DEVICE without a GPU, a handle with one."""
    import torch
    from gr_lora_amd import capi, lora
    gpu = torch.cuda.is_available()
    for kw in (dict(), dict(noise_sigma=0.5, seed=2 ** 63 + 5), dict(samp_rate=375e3)):
        h = C.c_void_p()
        st = lib.lora_hip_tx_create(C.byref(_cfg(**kw)), C.byref(h))
        assert st == (OK if gpu else ERR_NO_DEVICE) and bool(h.value) == gpu, kw
        if h.value:
            lib.lora_hip_tx_destroy(h)
    if not gpu:
        with pytest.raises(capi.LoraHipError):
            lora.traffic_synthesizer(2e6)
        with pytest.raises(capi.LoraHipError):
            lora.modulator(1e6, 125000, 7, False, 4, True)


# ---- the encoder against the numpy model -------------------------------------------------------------------------------

LENGTHS = (1, 2, 17, 64, 255)


def _payload(length, seed):
    return bytes(np.random.default_rng(seed).integers(0, 256, length, dtype=np.uint8))


@pytest.mark.parametrize("sf", range(6, 13))
def test_encoder_equals_the_numpy_model(lib, sf):
    """SF x CR 1..4 x crc x implicit x reduced_rate x lengths, default (valid) checksum and CRC and overridden ones; the frame's
    item count at a rate whose decimation is no power of two; ERR_BAD_CONFIG exactly where the model raises."""
    from gr_lora_amd import capi, synth
    for cr, crc, implicit, rr, length in itertools.product(range(1, 5), (False, True), (False, True), (False, True), LENGTHS):
        pl = _payload(length, 1000 * sf + length)
        over = (cr + length) % 2 == 0                       # every other case with the README's free nibbles and CRC bytes
        nib = (0, 4) if over else synth.valid_hdr_nibbles(length, cr, crc)
        cb = b"\x70\x0d" if over else synth.valid_crc_bytes(pl)
        cfg = synth.TxConfig(sf=sf, cr=cr, bw=125000, samp_rate=375e3, crc=crc, implicit=implicit, reduced_rate=rr, hdr_nibbles=nib)
        f = capi.tx_frame(pl, sf, cr, 125000, crc=crc, implicit=implicit, reduced_rate=rr, hdr_nibbles=nib if over else None,
                          crc_bytes=cb if over else None)
        try:
            want = synth.encode_shifts(pl, cfg, cb)
        except ValueError:
            assert sf == 6 and not implicit
            assert _encode(lib, f)[0] == ERR_BAD_CONFIG
            continue
        got = capi.tx_encode(f)
        assert got == (list(want[0]), list(want[1])), (sf, cr, crc, implicit, rr, length)
        if length <= 17:                                    # (the closed form below for all, the modulated frame itself for the short ones)
            assert capi.tx_frame_items(f, 375e3) == len(synth.modulate_frame(want[0], want[1], cfg))
        assert capi.tx_frame_items(f, 375e3) == (cfg.preamble_len + 4 + 8 + len(want[1])) * cfg.sps + cfg.sps // 4


def test_readme_vector_and_default_checks(lib):
    """049040deadbeef700d: payload deadbeef, SF7, CR4, CRC on, free nibbles (0, 4), CRC bytes 70 0d -> the model's shifts, which
    the golden capture tests/golden/sf7_cr4_deadbeef_x2.cf32 carries.  Without overrides the frame passes lora_hip_check_frame."""
    from gr_lora_amd import capi, synth
    pl = bytes.fromhex("deadbeef")
    cfg = synth.TxConfig(sf=7, cr=4)
    want = synth.encode_shifts(pl, cfg)
    assert synth.expected_frame_tail(pl, cfg).hex() == "049040deadbeef700d"
    assert capi.tx_encode(capi.tx_frame(pl, 7, 4, 125000, hdr_nibbles=(0, 4), crc_bytes=b"\x70\x0d")) == (list(want[0]), list(want[1]))
    for length in (0, 1, 2, 3, 17, 255):
        p = _payload(length, length)
        for cr in (1, 4):
            cfg = synth.TxConfig(sf=8, cr=cr, hdr_nibbles=synth.valid_hdr_nibbles(length, cr, True))
            w = synth.encode_shifts(p, cfg, synth.valid_crc_bytes(p))
            assert capi.tx_encode(capi.tx_frame(p, 8, cr, 125000)) == (list(w[0]), list(w[1]))
            chk = capi.check_frame(bytes(15) + synth.expected_frame_tail(p, cfg, synth.valid_crc_bytes(p)))
            assert chk.has_header and chk.header_checksum_ok and chk.crc_ok


def test_preamble_and_custom_sync_only_change_the_item_count(lib):
    from gr_lora_amd import capi
    a = capi.tx_frame(b"abcd", 9, 2, 125000)
    b = capi.tx_frame(b"abcd", 9, 2, 125000, preamble_len=12, sync_shifts=(8, 16))
    assert capi.tx_encode(a) == capi.tx_encode(b)
    assert capi.tx_frame_items(b, 1e6) - capi.tx_frame_items(a, 1e6) == 4 * 8 * 512
