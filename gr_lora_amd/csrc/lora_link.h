// lora_link.h -- launch interface of the link-metrics window kernel (lora_link.hip), shared with the host runtime.
#pragma once
#include <stdint.h>

#include "lora_device.h"

namespace lora_hip {

struct LinkWindowDesc {   // one window (host-written)
    int64_t  offset;      // first item of the window inside the IQ buffer; not looked at when valid == 0
    uint32_t valid;       // 0: the window lies outside its stream - its workgroup returns before forming any address
    uint32_t conj;        // 1: the spectrum of the window's complex conjugate (SFD windows)
};
struct LinkWindowRec {    // mirrors lora_hip_link_window_t
    int32_t  peak_bin;
    float    frac, lobe_power, total_power, peak_power;
    uint32_t valid;
};
constexpr int kLinkLobe = 3; // LORA_HIP_LINK_LOBE

// One 256-thread workgroup per window; d_out[n] must be zeroed by the caller (invalid windows write nothing).  hann: sps floats.
int launch_link_windows(const DevParams &p, const float *d_hann, const float2 *iq, const LinkWindowDesc *d_wins, uint32_t n, LinkWindowRec *d_out, void *stream);

} // namespace lora_hip
