// Launcher of the SHA-1 kernel (xs_sha1.hip), launch_md5's twin.  It is declared here and not beside
// launch_md5 in xs_internal.h because that header is one of the crypt kernels' sources
// (build.KERNEL_SOURCES): the hardware counters committed under profiles/ are tied to its bytes.
#pragma once
#include "xs_internal.h"

namespace xs {

// SHA-1 of n streams (xs_md5_desc, as launch_md5): 20 bytes per stream at digest + 20 i (4-byte
// aligned), ok[i] = 0 for an invalid descriptor (ok may be nullptr)
hipError_t launch_sha1(const xs_md5_desc* d, uint64_t n, const uint8_t* src, uint64_t src_len, uint8_t* digest,
                       uint8_t* ok, hipStream_t stream);

}  // namespace xs
