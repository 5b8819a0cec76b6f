// lora_frame_check.cpp -- frame validity (beyond the reference): the PHY header checksum and the payload
// CRC of a published frame blob.  Host only, no device work, no handle; see include/lora_hip.h for the contract and the
// reference lines (README.md:12, include/lora/utilities.h:396-404, lib/decoder_impl.cc:643,839).
#include <cstdint>
#include <cstring>

#include "../../include/lora_hip.h"
#include "lora_frame_check.h"

namespace {
constexpr int kLoratapLen = 15; // sizeof(loratap_header_t), include/lora/loratap.h:35-55
}

extern "C" {

lora_hip_status lora_hip_check_frame(const uint8_t *blob, size_t len, lora_hip_frame_check_t *out)
{
    if (!blob || !out) return LORA_HIP_ERR_ARG;
    std::memset(out, 0, sizeof *out);
    if (len < (size_t)kLoratapLen + 3u) return LORA_HIP_ERR_ARG;
    const uint8_t *ph = blob + kLoratapLen, *pl = ph + 3;
    const uint32_t length = ph[0], cr = ph[1] >> 5, has_crc = (ph[1] >> 4) & 1u;
    out->has_crc = (uint8_t)has_crc;
    out->has_header = len == (size_t)kLoratapLen + 3u + length + 2u * has_crc;
    out->header_checksum_calc = (uint8_t)lora_frame::header_checksum(length, cr, has_crc);
    out->header_checksum_rx = (uint8_t)((((uint32_t)ph[1] << 4) & 0x10u) | (ph[2] >> 4)); // d_phy_crc (:839), 5 bits
    out->header_checksum_ok = out->header_checksum_calc == out->header_checksum_rx;
    if (!out->has_header || !has_crc) return LORA_HIP_OK;
    using lora_frame::whiten_at;
    out->crc_calc = lora_frame::payload_crc16(pl, length);
    out->crc_rx = (uint16_t)((pl[length] ^ whiten_at(length)) | ((pl[length + 1u] ^ whiten_at(length + 1u)) << 8));
    out->crc_ok = out->crc_calc == out->crc_rx;
    return LORA_HIP_OK;
}


} // extern "C"
