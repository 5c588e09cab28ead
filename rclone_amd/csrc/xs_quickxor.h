// Launcher of the QuickXorHash kernel (xs_quickxor.hip).  Declared here and not in xs_internal.h for
// the reason xs_sha1.h gives: that header is one of the crypt kernels' sources
// (build.KERNEL_SOURCES), and the hardware counters committed under profiles/ are tied to its bytes.
#pragma once
#include "xs_internal.h"

namespace xs {

// Bytes of a stream one workgroup takes per step: 320 lanes x 16 bytes x 4 loads.  A multiple of
// 160, so every slice starts at ring position 0 and a lane's 16-byte chunk keeps its place in the
// 160-byte row.  The tests take their lengths around it (xs_quickxor_slice()).
constexpr uint64_t kQuickXorSlice = 320u * 16u * 4u;

// QuickXorHash of n streams (xs_md5_desc, as launch_md5): 20 bytes per stream at digest + 20 i
// (4-byte aligned), ok[i] = 0 and a zero digest for an invalid descriptor (ok may be nullptr).
// max_len is a hint, an upper bound of the longest stream in bytes (src_len will do): it sets how
// many workgroups share one stream.  The digest buffer is zeroed on `stream` before the kernel.
hipError_t launch_quickxor(const xs_md5_desc* d, uint64_t n, const uint8_t* src, uint64_t src_len, uint8_t* digest,
                           uint8_t* ok, uint64_t max_len, hipStream_t stream);

}  // namespace xs
