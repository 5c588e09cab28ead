// SHA-1 of many byte streams in HBM, one lane per stream (FIPS 180-4).
//
// Why: crypt's Fs.put and cryptcheck hash the ciphertext with the wrapped remote's
// Hashes().GetOne() (crypt.go:516, cryptcheck.go:74-79): MD5 where the remote has it, SHA-1 for
// Backblaze B2, Box and the other SHA-1-only remotes (fs/hash/hash.go:123-127).  This is xs_md5's
// twin for those remotes: the same descriptor (xs_md5_desc: an optional 16-byte-multiple prefix held
// in the descriptor, then `len` bytes at a 16-byte aligned offset of the source buffer), the same
// skeleton (aligned 16-byte loads two blocks ahead of the compression, block 0 through the
// prefix-aware chunk(), the tail built byte-wise), 20 bytes per stream back.  SHA-1 is sequential
// within a stream, so the parallelism is across streams: lane i hashes stream i.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "xs_sha1.h"

static_assert(sizeof(xs_md5_desc) == 64, "xs_md5_desc layout");

namespace xs {

namespace {

__device__ __forceinline__ uint32_t rotl(uint32_t x, int s) { return __builtin_amdgcn_alignbit(x, x, 32 - s); }
// x ^ y ^ z in one v_bitop3_b32 (truth table 0x96); written as two xors the compiler emits two
// instructions, and at one wave per SIMD the lane is bound by instructions issued
__device__ __forceinline__ uint32_t xor3(uint32_t x, uint32_t y, uint32_t z) {
  return __builtin_amdgcn_bitop3_b32(x, y, z, 0x96);
}

// One round: T = rotl(a, 5) + f(b, c, d) + e + K + W[t]; e = d; d = c; c = rotl(b, 30); b = a; a = T.
// The five words rotate by name (e receives T), so nothing moves.  Only rotl(a, 5) depends on the
// newest word: e + K + W[t] + f(b, c, d) is summed first (b is the word of the round before), then
// the rotate is added -- two dependent instructions per round, the shortest the function allows.
// The schedule word and rotl(b, 30) are off that chain.
#define XS_SHA1_ROUND(f, k, w, a, b, c, d, e) \
  e += (k) + (w) + f(b, c, d);                \
  e += rotl(a, 5);                            \
  b = rotl(b, 30)
// W[t] for t >= 16, kept in a 16-word ring (all indices are compile-time: the ring stays in registers)
#define XS_SHA1_W(t) \
  (W[(t) & 15] = rotl(xor3(W[((t) + 13) & 15], W[((t) + 8) & 15], W[((t) + 2) & 15]) ^ W[(t) & 15], 1))
#define XS_SHA1_W0(t) W[(t)]
#define XS_SHA1_CH(x, y, z) ((z) ^ ((x) & ((y) ^ (z))))
#define XS_SHA1_PAR(x, y, z) xor3(x, y, z)
#define XS_SHA1_MAJ(x, y, z) ((y) ^ (((x) ^ (y)) & ((z) ^ (y))))
#define XS_SHA1_R5(f, k, t, w)                      \
  XS_SHA1_ROUND(f, k, w((t) + 0), a, b, c, d, e);   \
  XS_SHA1_ROUND(f, k, w((t) + 1), e, a, b, c, d);   \
  XS_SHA1_ROUND(f, k, w((t) + 2), d, e, a, b, c);   \
  XS_SHA1_ROUND(f, k, w((t) + 3), c, d, e, a, b);   \
  XS_SHA1_ROUND(f, k, w((t) + 4), b, c, d, e, a)

// W: the block's 16 big-endian words (overwritten by the schedule)
__device__ __forceinline__ void sha1_block(uint32_t st[5], uint32_t W[16]) {
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4];
  XS_SHA1_R5(XS_SHA1_CH, 0x5a827999u, 0, XS_SHA1_W0);
  XS_SHA1_R5(XS_SHA1_CH, 0x5a827999u, 5, XS_SHA1_W0);
  XS_SHA1_R5(XS_SHA1_CH, 0x5a827999u, 10, XS_SHA1_W0);
  XS_SHA1_ROUND(XS_SHA1_CH, 0x5a827999u, XS_SHA1_W0(15), a, b, c, d, e);
  XS_SHA1_ROUND(XS_SHA1_CH, 0x5a827999u, XS_SHA1_W(16), e, a, b, c, d);
  XS_SHA1_ROUND(XS_SHA1_CH, 0x5a827999u, XS_SHA1_W(17), d, e, a, b, c);
  XS_SHA1_ROUND(XS_SHA1_CH, 0x5a827999u, XS_SHA1_W(18), c, d, e, a, b);
  XS_SHA1_ROUND(XS_SHA1_CH, 0x5a827999u, XS_SHA1_W(19), b, c, d, e, a);
  XS_SHA1_R5(XS_SHA1_PAR, 0x6ed9eba1u, 20, XS_SHA1_W);
  XS_SHA1_R5(XS_SHA1_PAR, 0x6ed9eba1u, 25, XS_SHA1_W);
  XS_SHA1_R5(XS_SHA1_PAR, 0x6ed9eba1u, 30, XS_SHA1_W);
  XS_SHA1_R5(XS_SHA1_PAR, 0x6ed9eba1u, 35, XS_SHA1_W);
  XS_SHA1_R5(XS_SHA1_MAJ, 0x8f1bbcdcu, 40, XS_SHA1_W);
  XS_SHA1_R5(XS_SHA1_MAJ, 0x8f1bbcdcu, 45, XS_SHA1_W);
  XS_SHA1_R5(XS_SHA1_MAJ, 0x8f1bbcdcu, 50, XS_SHA1_W);
  XS_SHA1_R5(XS_SHA1_MAJ, 0x8f1bbcdcu, 55, XS_SHA1_W);
  XS_SHA1_R5(XS_SHA1_PAR, 0xca62c1d6u, 60, XS_SHA1_W);
  XS_SHA1_R5(XS_SHA1_PAR, 0xca62c1d6u, 65, XS_SHA1_W);
  XS_SHA1_R5(XS_SHA1_PAR, 0xca62c1d6u, 70, XS_SHA1_W);
  XS_SHA1_R5(XS_SHA1_PAR, 0xca62c1d6u, 75, XS_SHA1_W);
  st[0] += a;
  st[1] += b;
  st[2] += c;
  st[3] += d;
  st[4] += e;
}
#undef XS_SHA1_R5
#undef XS_SHA1_MAJ
#undef XS_SHA1_PAR
#undef XS_SHA1_CH
#undef XS_SHA1_W0
#undef XS_SHA1_W
#undef XS_SHA1_ROUND

// 16-byte chunk q (byte offset 16q) of prefix || data; the prefix is read from the
// descriptor in global memory (a dynamically indexed local copy would go to scratch)
__device__ __forceinline__ uint4 chunk(const uint8_t* __restrict__ prefix, uint32_t prefix_len, uint64_t off,
                                       const uint8_t* __restrict__ src, uint64_t q) {
  const uint64_t p = 16u * q;
  if (p < prefix_len) return *reinterpret_cast<const uint4*>(prefix + p);
  return *reinterpret_cast<const uint4*>(src + off + (p - prefix_len));
}

__device__ __forceinline__ uint32_t byte_at(const uint8_t* __restrict__ prefix, uint32_t prefix_len, uint64_t off,
                                            const uint8_t* __restrict__ src, uint64_t p) {
  return p < prefix_len ? prefix[p] : src[off + (p - prefix_len)];
}

}  // namespace

__global__ void __launch_bounds__(64) xs_sha1(const xs_md5_desc* __restrict__ descs, uint64_t n,
                                              const uint8_t* __restrict__ src, uint64_t src_len,
                                              uint8_t* __restrict__ digest, uint8_t* __restrict__ ok) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const xs_md5_desc& d = descs[i];
  const uint64_t off = d.off, len = d.len;
  const uint32_t plen = d.prefix_len;
  const uint8_t* prefix = d.prefix;
  const bool valid = plen <= 32u && (plen & 15u) == 0 && (off & 15u) == 0 && off <= src_len && len <= src_len - off;
  if (ok) ok[i] = valid ? 1 : 0;
  uint32_t st[5] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u, 0xc3d2e1f0u};
  if (valid) {
    const uint64_t total = plen + len;
    const uint64_t nfull = total >> 6;
    uint32_t m[16];
    // Full blocks, loads two blocks ahead of the compression (one lane's stream is a serial
    // chain: without the prefetch every block waits a whole HBM round trip).  Block 0 holds
    // the prefix; from block 1 on the stream is plain data at body + 64 b - prefix_len.
    const uint8_t* body = src + off - plen;
    uint4 A[4], B[4], C[4];
    auto fetch = [&](uint4 (&q)[4], uint64_t b) {
#pragma unroll
      for (int j = 0; j < 4; j++) q[j] = *reinterpret_cast<const uint4*>(body + 64u * b + 16u * j);
    };
    auto compress = [&](const uint4 (&q)[4]) {  // words are big-endian: one v_perm_b32 each
#pragma unroll
      for (int j = 0; j < 4; j++) {
        m[4 * j] = __builtin_bswap32(q[j].x);
        m[4 * j + 1] = __builtin_bswap32(q[j].y);
        m[4 * j + 2] = __builtin_bswap32(q[j].z);
        m[4 * j + 3] = __builtin_bswap32(q[j].w);
      }
      sha1_block(st, m);
    };
    if (nfull > 0) {
#pragma unroll
      for (int j = 0; j < 4; j++) A[j] = chunk(prefix, plen, off, src, j);
    }
    if (nfull > 1) fetch(B, 1);
#pragma unroll 1
    for (uint64_t b = 0; b < nfull; b += 3) {  // A, B, C rotate: no register moves, no early waits
      if (b + 2 < nfull) fetch(C, b + 2);
      compress(A);
      if (b + 1 >= nfull) break;
      if (b + 3 < nfull) fetch(A, b + 3);
      compress(B);
      if (b + 2 >= nfull) break;
      if (b + 4 < nfull) fetch(B, b + 4);
      compress(C);
    }
    // tail: remaining bytes, 0x80, zero pad, 64-bit big-endian bit length
    const uint32_t rem = (uint32_t)(total & 63u);
    const uint64_t base = nfull << 6;
    const uint64_t bits = total << 3;
    const int tail_blocks = rem < 56u ? 1 : 2;
#pragma unroll 1
    for (int t = 0; t < tail_blocks; t++) {
#pragma unroll
      for (int j = 0; j < 16; j++) m[j] = 0;
#pragma unroll
      for (uint32_t k = 0; k < 64u; k++) {
        const uint32_t pos = 64u * (uint32_t)t + k;  // position after base
        uint32_t v = 0;
        if (pos < rem) v = byte_at(prefix, plen, off, src, base + pos);
        else if (pos == rem) v = 0x80u;
        m[k >> 2] |= v << (8u * (3u - (k & 3u)));
      }
      if (t == tail_blocks - 1) {
        m[14] = (uint32_t)(bits >> 32);
        m[15] = (uint32_t)bits;
      }
      sha1_block(st, m);
    }
  }
  uint8_t* o = digest + 20u * i;  // 20-byte stride: only 4-byte aligned
#pragma unroll
  for (int j = 0; j < 5; j++) *reinterpret_cast<uint32_t*>(o + 4 * j) = __builtin_bswap32(st[j]);
}

hipError_t launch_sha1(const xs_md5_desc* d, uint64_t n, const uint8_t* src, uint64_t src_len, uint8_t* digest,
                       uint8_t* ok, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(xs_sha1, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, d, n, src, src_len, digest, ok);
  return hipGetLastError();
}

}  // namespace xs
