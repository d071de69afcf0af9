// What csrc/split.hip offers the other translation units.
#ifndef MBPE_SPLIT_H
#define MBPE_SPLIT_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mbpe {

// adds the chunk ends of an end mask over n_bytes text bytes (bit i of byte i >> 3; the mask is 4-byte aligned and, as
// everywhere, 2 * ceil(n_bytes / 16) + 16 bytes long with nothing set at or beyond n_bytes) to *count_out on the device
void launch_mask_popcount(hipStream_t stream, const uint8_t *mask, uint64_t n_bytes, unsigned long long *count_out);

}  // namespace mbpe

#endif
