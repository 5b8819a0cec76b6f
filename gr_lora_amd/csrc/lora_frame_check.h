// lora_frame_check.h -- the PHY header checksum, the payload CRC-16 and the payload whitening byte as a LoRa transmitter
// computes them: shared by lora_hip_check_frame (lora_frame_check.cpp), which verifies a decoded frame, and the frame encoder
// (lora_tx.hip), which makes frames that pass it.  Host only.
#ifndef LORA_FRAME_CHECK_H
#define LORA_FRAME_CHECK_H

#include <cstdint>

namespace lora_frame {

// 5-bit header checksum c4..c0 over a0..a7 = length (MSB first), a8..a10 = cr (MSB first), a11 = has_crc
// (include/lora/utilities.h:398-402 in its own bit numbering)
inline uint32_t header_checksum(uint32_t length, uint32_t cr, uint32_t has_crc)
{
    const uint32_t a = (length << 4) | (cr << 1) | has_crc; // a0 is bit 11
    auto bit = [&](int i) { return (a >> (11 - i)) & 1u; };
    const uint32_t c4 = bit(0) ^ bit(1) ^ bit(2) ^ bit(3), c3 = bit(0) ^ bit(4) ^ bit(5) ^ bit(6) ^ bit(11),
                   c2 = bit(1) ^ bit(4) ^ bit(7) ^ bit(8) ^ bit(10), c1 = bit(2) ^ bit(5) ^ bit(7) ^ bit(9) ^ bit(10) ^ bit(11),
                   c0 = bit(3) ^ bit(6) ^ bit(8) ^ bit(9) ^ bit(10) ^ bit(11);
    return (c4 << 4) | (c3 << 3) | (c2 << 2) | (c1 << 1) | c0;
}

// byte idx of the payload whitening sequence
inline uint8_t whiten_at(uint32_t idx)
{
    uint8_t r = 0xff;
    for (uint32_t i = 0; i < idx; i++) r = (uint8_t)((r << 1) | (((r >> 7) ^ (r >> 5) ^ (r >> 4) ^ (r >> 3)) & 1u));
    return r;
}

// CRC-16 of a payload of `length` bytes: CCITT over all but the last two, which are XORed in
inline uint16_t payload_crc16(const uint8_t *pl, uint32_t length)
{
    uint16_t crc = 0;
    for (uint32_t i = 0; i + 2u < length; i++) {
        crc ^= (uint16_t)(pl[i] << 8);
        for (int k = 0; k < 8; k++) crc = (crc & 0x8000u) ? (uint16_t)((crc << 1) ^ 0x1021u) : (uint16_t)(crc << 1);
    }
    if (length >= 1u) crc ^= pl[length - 1u];
    if (length >= 2u) crc ^= (uint16_t)(pl[length - 2u] << 8);
    return crc;
}

} // namespace lora_frame

#endif // LORA_FRAME_CHECK_H
