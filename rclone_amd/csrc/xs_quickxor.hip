// QuickXorHash of many byte streams in HBM, many workgroups per stream
// (backend/onedrive/quickxorhash/quickxorhash.go:69-111).
//
// Why: crypt's Fs.put and cryptcheck hash the ciphertext with the wrapped remote's
// Hashes().GetOne() (crypt.go:516, cryptcheck.go:74-79).  OneDrive (Personal, Business, SharePoint)
// offers "quickxor" alone (backend/onedrive/onedrive.go:113, :344-351).  The descriptor and the
// contract are xs_md5's and xs_sha1's: an optional 16-byte-multiple prefix held in the descriptor,
// then `len` bytes at a 16-byte aligned offset of the source buffer; 20 bytes per stream back.
//
// The hash XORs stream byte i into a 160-bit ring at bit (11 i) mod 160 and the stream length into
// the last 8 of the ring's 20 bytes.  XOR is associative and commutative, so unlike MD5 and SHA-1
// one stream is split over the whole device:
//   * 11 * 160 is a multiple of 160: bytes i and i + 160 meet the same bit.  The column-wise XOR of
//     the stream in rows of 160 bytes (ten 16-byte chunks) holds everything.
//   * A workgroup has 320 lanes and walks 16-byte chunks with a stride of 320, a multiple of 10, from
//     a slice start that is a multiple of 160 bytes: lane t only ever meets chunks of row place
//     t mod 10, so one uint4 accumulator per lane is the whole state and a loop step is a 16-byte
//     coalesced load and four XORs.
//   * At the end the 32 lanes of each row place are XORed through LDS into the 160-byte row, 40 lanes
//     fold one dword each into the ring, a butterfly over the first wave sums the ring, and five
//     lanes XOR one word each into the digest with a 32-bit atomic.  The launcher zeroes the digests
//     first.  Slices start at ring position 0, so no rotation is needed, and the result does not
//     depend on the order in which workgroups arrive.
// The grid is (object, slice lane): workgroup (i, y) takes slices y, y + gridDim.y, ... of object i,
// and exits at once if its first slice starts past the object's full chunks.  Workgroup (i, 0) also
// takes the prefix chunks, the 0-15 tail bytes, the length and ok[i].
#include <hip/hip_runtime.h>

#include <cstdint>

#include "xs_quickxor.h"

static_assert(sizeof(xs_md5_desc) == 64, "xs_md5_desc layout");

namespace xs {

namespace {

constexpr unsigned kLanes = 320;                          // 5 waves; 320 = 32 * 10
constexpr uint64_t kSliceChunks = kQuickXorSlice / 16;    // 1280 chunks = 4 loads per lane
static_assert(kQuickXorSlice % 160 == 0 && kSliceChunks == 4 * kLanes, "slice shape");

__device__ __forceinline__ void xor4(uint4& a, const uint4& v) {
  a.x ^= v.x;
  a.y ^= v.y;
  a.z ^= v.z;
  a.w ^= v.w;
}

}  // namespace

__global__ void __launch_bounds__(kLanes) xs_quickxor(const xs_md5_desc* __restrict__ descs, uint64_t n,
                                                      const uint8_t* __restrict__ src, uint64_t src_len,
                                                      uint8_t* __restrict__ digest, uint8_t* __restrict__ ok) {
  __shared__ uint32_t sh[4 * kLanes];
  const uint64_t i = blockIdx.x;
  const unsigned t = threadIdx.x, y = blockIdx.y;
  if (i >= n) return;
  const xs_md5_desc& d = descs[i];
  const uint64_t off = d.off, len = d.len;
  const uint32_t plen = d.prefix_len;
  const bool valid = plen <= 32u && (plen & 15u) == 0 && (off & 15u) == 0 && off <= src_len && len <= src_len - off;
  // everything below is uniform over the workgroup: the whole group leaves, or none of it
  if (!valid) {
    if (ok && y == 0 && t == 0) ok[i] = 0;  // the digest stays zero
    return;
  }
  const uint64_t total = plen + len;
  const uint64_t nfull = total >> 4;  // whole 16-byte chunks of prefix || data
  if (y > 0 && (uint64_t)y * kSliceChunks >= nfull) return;
  const uint64_t pc = plen >> 4;  // stream chunk c >= pc is data chunk c - pc
  const uint4* __restrict__ data = reinterpret_cast<const uint4*>(src + off);
  uint4 acc = {0, 0, 0, 0};
  for (uint64_t s = y; s * kSliceChunks < nfull; s += gridDim.y) {
    const uint64_t c0 = s * kSliceChunks + t;
    if (s > 0 && (s + 1) * kSliceChunks <= nfull) {  // a whole slice of data: four loads in flight
      const uint4* p = data + (c0 - pc);
      const uint4 v0 = p[0], v1 = p[kLanes], v2 = p[2 * kLanes], v3 = p[3 * kLanes];
      xor4(acc, v0);
      xor4(acc, v1);
      xor4(acc, v2);
      xor4(acc, v3);
    } else {  // the first slice (the prefix chunks are not in src) and the last
#pragma unroll
      for (unsigned u = 0; u < 4; u++) {
        const uint64_t c = c0 + u * kLanes;
        if (c >= pc && c < nfull) xor4(acc, data[c - pc]);
      }
    }
  }
  if (y == 0) {
    if (ok && t == 0) ok[i] = 1;
    // chunks 0 and 1 of a prefixed stream come from the descriptor (lanes 0 and 1: their row place)
    if (t < pc) xor4(acc, *reinterpret_cast<const uint4*>(d.prefix + 16u * t));
    // the 0-15 bytes after the last whole chunk, as a zero-padded chunk at row place nfull mod 10.
    // The prefix is a multiple of 16, so they are the last bytes of the data.
    const uint32_t rem = (uint32_t)(total & 15u);
    if (rem && t == (unsigned)(nfull % 10u)) {
      const uint8_t* tail = src + off + (len - rem);
      uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
      for (uint32_t j = 0; j < 15u; j++)
        if (j < rem) w[j >> 2] |= (uint32_t)tail[j] << (8u * (j & 3u));
      acc.x ^= w[0];
      acc.y ^= w[1];
      acc.z ^= w[2];
      acc.w ^= w[3];
    }
  }
  // 320 accumulators -> the 160-byte row: lane t holds row bytes 16 (t mod 10) .. +15, so dword
  // 4 t + c of sh is row dword (4 t + c) mod 40
  sh[4 * t + 0] = acc.x;
  sh[4 * t + 1] = acc.y;
  sh[4 * t + 2] = acc.z;
  sh[4 * t + 3] = acc.w;
  __syncthreads();
  if (t >= 64) return;  // the first wave finishes
  uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0, r4 = 0;  // this lane's share of the ring, little-endian words
  if (t < 40) {
    uint32_t row = 0;
#pragma unroll
    for (unsigned k = 0; k < 32; k++) row ^= sh[t + 40 * k];
    // row byte q goes to ring bit (11 q) mod 160; a byte that starts above bit 24 of its word
    // spills into the next word, and the word after word 4 is word 0 (bits past 159 wrap)
#pragma unroll
    for (unsigned b = 0; b < 4; b++) {
      const uint32_t v = (row >> (8u * b)) & 0xffu;
      const uint32_t bit = (11u * (4u * t + b)) % 160u;
      const uint32_t wd = bit >> 5, sft = bit & 31u;
      const uint32_t lo = v << sft, hi = sft > 24u ? v >> (32u - sft) : 0u;
      const uint32_t wn = wd == 4u ? 0u : wd + 1u;
      r0 ^= (wd == 0u ? lo : 0u) ^ (wn == 0u ? hi : 0u);
      r1 ^= (wd == 1u ? lo : 0u) ^ (wn == 1u ? hi : 0u);
      r2 ^= (wd == 2u ? lo : 0u) ^ (wn == 2u ? hi : 0u);
      r3 ^= (wd == 3u ? lo : 0u) ^ (wn == 3u ? hi : 0u);
      r4 ^= (wd == 4u ? lo : 0u) ^ (wn == 4u ? hi : 0u);
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    r0 ^= __shfl_xor(r0, m);
    r1 ^= __shfl_xor(r1, m);
    r2 ^= __shfl_xor(r2, m);
    r3 ^= __shfl_xor(r3, m);
    r4 ^= __shfl_xor(r4, m);
  }
  if (y == 0) {  // the stream length, 64-bit little-endian, into digest bytes 12..19
    r3 ^= (uint32_t)total;
    r4 ^= (uint32_t)(total >> 32);
  }
  // one 32-bit atomic per word: the workgroups of one object meet here in any order
  const uint32_t mine = t == 0 ? r0 : t == 1 ? r1 : t == 2 ? r2 : t == 3 ? r3 : r4;
  if (t < 5 && mine) atomicXor(reinterpret_cast<uint32_t*>(digest + 20u * i) + t, mine);
}

hipError_t launch_quickxor(const xs_md5_desc* d, uint64_t n, const uint8_t* src, uint64_t src_len, uint8_t* digest,
                           uint8_t* ok, uint64_t max_len, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (n > 0x7fffffffull) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(digest, 0, 20 * n, stream);
  if (e != hipSuccess) return e;
  // Workgroups per object (DESIGN.md 3b has the measurements).  Never more than the longest
  // object has slices.  A workgroup ends with a reduction and five atomics on its object's digest,
  // so long objects want few workgroups with many slices each: one 1 GiB or 4 GiB object reads at
  // 6.1-6.3 TB/s on 512 to 1 280 workgroups and at 1.7 and 4.3 TB/s on one per slice.  kTarget / n
  // is that plateau shared by n equally long objects.  kSkew is the floor that keeps one long
  // object among many short ones off a single workgroup, as long as the grid, whose workgroups
  // past an object's end cost a dispatch each and do nothing, stays within kGrid.
  constexpr uint64_t kTarget = 768, kSkew = 128, kGrid = 1u << 18;
  const uint64_t want = (max_len + 32 + kQuickXorSlice - 1) / kQuickXorSlice;
  const uint64_t skew = kSkew < kGrid / n ? kSkew : kGrid / n;
  uint64_t ny = kTarget / n > skew ? kTarget / n : skew;
  if (ny > want) ny = want;
  if (ny < 1) ny = 1;
  hipLaunchKernelGGL(xs_quickxor, dim3((unsigned)n, (unsigned)ny), dim3(kLanes), 0, stream, d, n, src, src_len,
                     digest, ok);
  return hipGetLastError();
}

}  // namespace xs
