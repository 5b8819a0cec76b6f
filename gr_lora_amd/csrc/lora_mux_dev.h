// lora_mux_dev.h -- internal: the mux's device-fed path (lora_runtime.cpp), next to lora_hip_mux_work's host uploads.
// A writer on the device (the gateway's filter bank, lora_gateway.cpp) stores the next n items of every channel straight into
// the current chunks of the mux's pipeline (the chunk pipeline of lora_hip_work, with n channels); the mux then
// runs the same pass loop and latency check as after lora_hip_mux_work.  Per step:
//     collect_if_done -> room -> rows -> before_write(st) -> the writer on st -> event on st -> commit(n, event)
// Row pointers stay valid until the next commit or collect_if_done (a rotation or a grown tail area moves them).
// Not exported (hidden visibility): the C ABI is include/lora_hip.h and include/lora_hip_gateway.h.
#ifndef LORA_MUX_DEV_H
#define LORA_MUX_DEV_H

#include <hip/hip_runtime.h>

#include <stddef.h>

#include "../../include/lora_hip.h"

namespace lora_mux_dev {

#define LORA_MUX_DEV_API __attribute__((visibility("hidden")))

// publishes the pass in flight if its device work is done (what lora_hip_mux_work does first)
LORA_MUX_DEV_API lora_hip_status collect_if_done(lora_hip_mux_t *m);
// items per channel in a full chunk (a pass starts when every chunk is full)
LORA_MUX_DEV_API size_t batch(const lora_hip_mux_t *m);
// items that every channel's current chunk can still take
LORA_MUX_DEV_API size_t room(const lora_hip_mux_t *m);
// n_channels device pointers (float2 *): where each channel's next item goes in the current chunk
LORA_MUX_DEV_API void rows(const lora_hip_mux_t *m, void **out);
// st waits for every copy of the mux that still reads the current chunk area (short channels' moves, the last collect's tails)
LORA_MUX_DEV_API lora_hip_status before_write(lora_hip_mux_t *m, hipStream_t st);
// n items written on every channel once `written` has completed: fill += n, then the pass loop and the latency check
LORA_MUX_DEV_API lora_hip_status commit(lora_hip_mux_t *m, size_t n, hipEvent_t written);

} // namespace lora_mux_dev

#endif
