"""Semtech UDP packet-forwarder egress: a decoded frame and its link metrics as an `rxpk` object, and the PUSH_DATA datagram
that carries it to a network server (protocol version 2).  Host only: no device, no torch.

    PUSH_DATA = 0x02 | two token bytes | 0x00 | the gateway's 8-byte EUI | JSON {"rxpk": [...]}
"""
from __future__ import annotations

import base64
import json
import os
from typing import Mapping, Sequence

from . import capi

PROTOCOL_VERSION = 2
PUSH_DATA = 0x00
LORATAP_LEN, LORAPHY_LEN = 15, 3


def eui_bytes(eui) -> bytes:
    """A gateway EUI given as 8 bytes, an int, or 16 hex digits (separators allowed)."""
    if isinstance(eui, (bytes, bytearray)):
        b = bytes(eui)
    elif isinstance(eui, int):
        b = eui.to_bytes(8, "big")
    else:
        b = bytes.fromhex("".join(c for c in str(eui) if c not in ":-. "))
    if len(b) != 8:
        raise ValueError("a gateway EUI is 8 bytes, not %d" % len(b))
    return b


def _field(link, name):
    return link[name] if isinstance(link, Mapping) else getattr(link, name)


def rxpk(blob: bytes, link, *, freq_hz: float, sf: int, bandwidth: int, row_rate: float, rssi_offset_db: float = 0.0) -> dict:
    """One frame as the packet forwarder reports it.  blob: the published frame (loratap header, PHY header, payload, CRC bytes);
    link: its metrics (a "link" message or a capi.LinkMetrics, with header_pos); row_rate: sample rate of the stream header_pos counts in."""
    blob = bytes(blob)
    phy = blob[LORATAP_LEN:LORATAP_LEN + LORAPHY_LEN]
    if len(phy) < LORAPHY_LEN:
        raise ValueError("frame blob too short for a PHY header")
    chk = capi.check_frame(blob)
    has_crc = bool(chk.has_crc)
    payload = blob[LORATAP_LEN + LORAPHY_LEN:len(blob) - (2 if has_crc else 0)]
    cr = (phy[1] >> 5) & 7
    return {
        "tmst": int(round(int(_field(link, "header_pos")) * 1e6 / float(row_rate))) % (1 << 32),
        "freq": round(float(freq_hz) / 1e6, 6),
        "chan": int(link.get("row", 0)) if isinstance(link, Mapping) else 0,
        "rfch": 0,
        "stat": (1 if chk.crc_ok else -1) if has_crc else 0,
        "modu": "LORA",
        "datr": "SF%dBW%d" % (int(sf), int(bandwidth) // 1000),
        "codr": "4/%d" % (4 + cr) if 1 <= cr <= 4 else "OFF",
        "rssi": int(round(float(_field(link, "rssi_dbfs")) + float(rssi_offset_db))),
        "lsnr": round(float(_field(link, "snr_db")), 1),
        "size": len(payload),
        "data": base64.b64encode(payload).decode("ascii"),
    }


def push_data(gateway_eui, rxpks: Sequence[dict], token: bytes = None) -> bytes:
    """The PUSH_DATA datagram for a list of rxpk objects (token: two bytes, random if not given)."""
    token = os.urandom(2) if token is None else bytes(token)
    if len(token) != 2:
        raise ValueError("the token is two bytes")
    body = json.dumps({"rxpk": list(rxpks)}, separators=(",", ":")).encode("ascii")
    return bytes([PROTOCOL_VERSION]) + token + bytes([PUSH_DATA]) + eui_bytes(gateway_eui) + body
