"""CPU: the Semtech UDP packet-forwarder egress (gr_lora_amd/forwarder.py, lora.packet_forwarder_sink): the rxpk object of a frame
and its link metrics, the PUSH_DATA datagram, over a loopback socket."""
import base64
import json
import socket

import pytest

from gr_lora_amd import forwarder, lora, synth

EUI = "AA:55:5A:00:00:00:01:02"


def _blob(payload, cr=4, valid=True):
    """A published frame: 15-byte loratap header, 3-byte PHY header, payload, the two CRC bytes (as the decoder leaves them)."""
    cfg = synth.TxConfig(sf=7, cr=cr, hdr_nibbles=synth.valid_hdr_nibbles(len(payload), cr, True))
    crc = synth.valid_crc_bytes(payload)
    if not valid:
        crc = bytes([crc[0] ^ 0x40, crc[1]])
    return bytes(15) + synth.expected_frame_tail(payload, cfg, crc)


def _link(**kw):
    d = dict(flags=7, signal_power=1e-3, noise_power=1e-4, rssi_dbfs=-30.4, snr_db=9.96, cfo_bins=0.1, cfo_hz=97.6, timing_samples=0.2,
             sync_shift=[24, 32], header_pos=12345678, end_pos=12400000)
    d.update(kw)
    return d


def test_rxpk_fields():
    payload = b"\x40\x11\x22\x33\x44hello"
    pk = forwarder.rxpk(_blob(payload), _link(), freq_hz=868.1e6, sf=7, bandwidth=125000, row_rate=1e6, rssi_offset_db=-107.0)
    assert pk["tmst"] == 12345678 and pk["freq"] == 868.1 and pk["datr"] == "SF7BW125" and pk["codr"] == "4/8" and pk["modu"] == "LORA"
    assert pk["stat"] == 1 and pk["rssi"] == -137 and pk["lsnr"] == 10.0 and pk["size"] == len(payload)
    assert base64.b64decode(pk["data"]) == payload
    # a corrupted CRC, another rate, a time stamp past 2^32 us, a row rate that is not 1 MHz
    pk = forwarder.rxpk(_blob(payload, cr=1, valid=False), _link(header_pos=3 * (1 << 31), snr_db=-7.26), freq_hz=867.5e6, sf=12, bandwidth=125000,
                        row_rate=250e3)
    assert pk["stat"] == -1 and pk["codr"] == "4/5" and pk["datr"] == "SF12BW125" and pk["lsnr"] == -7.3
    assert pk["tmst"] == (3 * (1 << 31) * 4) % (1 << 32) and pk["freq"] == 867.5 and pk["rssi"] == -30
    # no CRC in the frame: stat 0, nothing cut off the payload
    cfg = synth.TxConfig(sf=7, cr=4, crc=False, hdr_nibbles=synth.valid_hdr_nibbles(len(payload), 4, False))
    pk = forwarder.rxpk(bytes(15) + synth.expected_frame_tail(payload, cfg), _link(), freq_hz=868.1e6, sf=7, bandwidth=125000, row_rate=1e6)
    assert pk["stat"] == 0 and base64.b64decode(pk["data"]) == payload
    with pytest.raises(ValueError):
        forwarder.rxpk(bytes(16), _link(), freq_hz=868.1e6, sf=7, bandwidth=125000, row_rate=1e6)


def test_push_data_header():
    d = forwarder.push_data(EUI, [{"a": 1}], token=b"\x12\x34")
    assert d[:12] == bytes([2, 0x12, 0x34, 0x00]) + bytes.fromhex("AA555A0000000102")
    assert json.loads(d[12:]) == {"rxpk": [{"a": 1}]}
    assert forwarder.eui_bytes(0xAA555A0000000102) == forwarder.eui_bytes(EUI) == forwarder.eui_bytes(bytes.fromhex("AA555A0000000102"))
    with pytest.raises(ValueError):
        forwarder.eui_bytes("AA55")
    with pytest.raises(ValueError):
        forwarder.push_data(EUI, [], token=b"\x01")


def test_sink_sends_one_datagram_per_link_message():
    srv = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    srv.bind(("127.0.0.1", 0))
    srv.settimeout(5.0)
    sink = lora.packet_forwarder_sink("127.0.0.1", srv.getsockname()[1], EUI, rssi_offset_db=-100.0)
    src = lora._MsgBlock()
    src.message_port_register_out("link")
    lora.msg_connect(src, "link", sink, "link")
    payloads = [b"first frame", b"second"]
    for i, p in enumerate(payloads):
        src.message_port_pub("link", _link(blob=_blob(p, valid=i == 0), header_pos=1000 * (i + 1), sf=9, bandwidth=125000, row_rate=1e6, freq_hz=868.3e6,
                                           row=i, grid_index=i - 1))
    assert sink.sent == 2
    for i, p in enumerate(payloads):
        d = srv.recv(4096)
        assert d[0] == 2 and d[3] == 0 and d[4:12] == bytes.fromhex("AA555A0000000102")
        (pk,) = json.loads(d[12:])["rxpk"]
        assert base64.b64decode(pk["data"]) == p and pk["size"] == len(p) and pk["tmst"] == 1000 * (i + 1)
        assert pk["stat"] == (1 if i == 0 else -1) and pk["datr"] == "SF9BW125" and pk["freq"] == 868.3 and pk["rssi"] == -130 and pk["chan"] == i
    sink.close()
    srv.close()
