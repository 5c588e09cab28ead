// xs_host_sha1.h -- SHA-1 (FIPS 180-4) on a host core: the host tier of the ciphertext hash for
// wrapped remotes whose Hashes().GetOne() is SHA-1 (Backblaze B2, Box; fs/hash/hash.go:123-127),
// with the interface of HostMd5 (xs_host_md5.h).  It hashes the objects the engine routes off the
// GPU's one-lane-per-object SHA-1 (xs_sha1.hip) and the per-object streams (md5_workers.h):
// SHA-1("RCLONE\0\0" || nonce || wire blocks).
//
// Two block functions with the same result: portable C++, and the x86 SHA extensions (four rounds
// per instruction) where the CPU has them, chosen at run time.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__x86_64__) || defined(__i386__)
#include <immintrin.h>
#define XS_SHA1_X86 1
#endif

namespace xs {

class HostSha1 {
 public:
  // true when the CPU has the SHA extensions (the block function then used by default)
  static bool has_shani() {
#ifdef XS_SHA1_X86
    static const bool ok = __builtin_cpu_supports("sha") && __builtin_cpu_supports("sse4.1");
    return ok;
#else
    return false;
#endif
  }

  HostSha1() : ni_(has_shani()) {}
  // portable_only: never the SHA extensions (the stand-alone test runs both and compares)
  explicit HostSha1(bool portable_only) : ni_(!portable_only && has_shani()) {}

  void update(const uint8_t* p, size_t len) {
    if (len == 0) return;
    size_t have = (size_t)(n_ & 63);
    n_ += len;
    if (have) {
      size_t k = 64 - have < len ? 64 - have : len;
      memcpy(buf_ + have, p, k);
      p += k;
      len -= k;
      if (have + k < 64) return;
      blocks(buf_, 1);
    }
    if (len >= 64) {
      blocks(p, len / 64);
      p += len & ~(size_t)63;
      len &= 63;
    }
    if (len) memcpy(buf_, p, len);
  }

  void final(uint8_t out[20]) {
    const uint64_t bits = n_ * 8;
    uint8_t pad[72] = {0x80};
    const size_t have = (size_t)(n_ & 63);
    const size_t padlen = have < 56 ? 56 - have : 120 - have;
    update(pad, padlen);
    uint8_t lb[8];
    for (int i = 0; i < 8; i++) lb[i] = (uint8_t)(bits >> (8 * (7 - i)));  // big-endian bit length
    update(lb, 8);
    for (int i = 0; i < 5; i++) {
      out[4 * i] = (uint8_t)(h_[i] >> 24);
      out[4 * i + 1] = (uint8_t)(h_[i] >> 16);
      out[4 * i + 2] = (uint8_t)(h_[i] >> 8);
      out[4 * i + 3] = (uint8_t)h_[i];
    }
  }

 private:
  uint32_t h_[5] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u, 0xc3d2e1f0u};
  uint8_t buf_[64];
  uint64_t n_ = 0;
  bool ni_;

  static inline uint32_t rol(uint32_t x, int c) { return (x << c) | (x >> (32 - c)); }
  static inline uint32_t be32(const uint8_t* p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
  }

  void blocks(const uint8_t* p, size_t nblk) {
#ifdef XS_SHA1_X86
    if (ni_) {
      blocks_ni(h_, p, nblk);
      return;
    }
#endif
    blocks_portable(h_, p, nblk);
  }

  // The round is T = rol(a, 5) + f(b, c, d) + e + K + W[t]; e = d; d = c; c = rol(b, 30); b = a;
  // a = T.  Only rol(a, 5) depends on the newest word, so everything else is summed first and the
  // chain through `a` is one rotate and one add per round.  The five words rotate by name instead
  // of moving; W is a 16-word ring with compile-time indices.
  static void blocks_portable(uint32_t h[5], const uint8_t* p, size_t nblk) {
    uint32_t a0 = h[0], b0 = h[1], c0 = h[2], d0 = h[3], e0 = h[4];
    for (; nblk; nblk--, p += 64) {
      uint32_t W[16];
      for (int i = 0; i < 16; i++) W[i] = be32(p + 4 * i);
      uint32_t a = a0, b = b0, c = c0, d = d0, e = e0;
#define XS_W(t) \
  (W[(t) & 15] = rol(W[((t) + 13) & 15] ^ W[((t) + 8) & 15] ^ W[((t) + 2) & 15] ^ W[(t) & 15], 1))
#define XS_CH(x, y, z) ((z) ^ ((x) & ((y) ^ (z))))
#define XS_PAR(x, y, z) ((x) ^ (y) ^ (z))
#define XS_MAJ(x, y, z) (((x) & (y)) | ((z) & ((x) | (y))))
#define XS_R(f, k, w, a, b, c, d, e) \
  e += (k) + (w) + f(b, c, d);       \
  e += rol(a, 5);                    \
  b = rol(b, 30)
#define XS_R5(f, k, t, w)                    \
  XS_R(f, k, w((t) + 0), a, b, c, d, e);     \
  XS_R(f, k, w((t) + 1), e, a, b, c, d);     \
  XS_R(f, k, w((t) + 2), d, e, a, b, c);     \
  XS_R(f, k, w((t) + 3), c, d, e, a, b);     \
  XS_R(f, k, w((t) + 4), b, c, d, e, a)
#define XS_W0(t) W[(t)]
      XS_R5(XS_CH, 0x5a827999u, 0, XS_W0);
      XS_R5(XS_CH, 0x5a827999u, 5, XS_W0);
      XS_R5(XS_CH, 0x5a827999u, 10, XS_W0);
      XS_R(XS_CH, 0x5a827999u, XS_W0(15), a, b, c, d, e);
      XS_R(XS_CH, 0x5a827999u, XS_W(16), e, a, b, c, d);
      XS_R(XS_CH, 0x5a827999u, XS_W(17), d, e, a, b, c);
      XS_R(XS_CH, 0x5a827999u, XS_W(18), c, d, e, a, b);
      XS_R(XS_CH, 0x5a827999u, XS_W(19), b, c, d, e, a);
      XS_R5(XS_PAR, 0x6ed9eba1u, 20, XS_W);
      XS_R5(XS_PAR, 0x6ed9eba1u, 25, XS_W);
      XS_R5(XS_PAR, 0x6ed9eba1u, 30, XS_W);
      XS_R5(XS_PAR, 0x6ed9eba1u, 35, XS_W);
      XS_R5(XS_MAJ, 0x8f1bbcdcu, 40, XS_W);
      XS_R5(XS_MAJ, 0x8f1bbcdcu, 45, XS_W);
      XS_R5(XS_MAJ, 0x8f1bbcdcu, 50, XS_W);
      XS_R5(XS_MAJ, 0x8f1bbcdcu, 55, XS_W);
      XS_R5(XS_PAR, 0xca62c1d6u, 60, XS_W);
      XS_R5(XS_PAR, 0xca62c1d6u, 65, XS_W);
      XS_R5(XS_PAR, 0xca62c1d6u, 70, XS_W);
      XS_R5(XS_PAR, 0xca62c1d6u, 75, XS_W);
#undef XS_W0
#undef XS_R5
#undef XS_R
#undef XS_MAJ
#undef XS_PAR
#undef XS_CH
#undef XS_W
      a0 += a;
      b0 += b;
      c0 += c;
      d0 += d;
      e0 += e;
    }
    h[0] = a0;
    h[1] = b0;
    h[2] = c0;
    h[3] = d0;
    h[4] = e0;
  }

#ifdef XS_SHA1_X86
  // x86 SHA extensions: sha1rnds4 runs four rounds (its immediate picks f and K), sha1nexte
  // supplies rol(a, 30) of four rounds ago as the next e, sha1msg1 / sha1msg2 the schedule.  Group
  // g is rounds 4g..4g+3; the four message registers and the two e registers rotate by name.
  __attribute__((target("sha,sse4.1"))) static void blocks_ni(uint32_t h[5], const uint8_t* p, size_t nblk) {
    const __m128i bswap = _mm_set_epi64x(0x0001020304050607ll, 0x08090a0b0c0d0e0fll);
    __m128i abcd = _mm_shuffle_epi32(_mm_loadu_si128((const __m128i*)h), 0x1b);
    __m128i e0 = _mm_set_epi32((int)h[4], 0, 0, 0), e1 = _mm_setzero_si128();
    for (; nblk; nblk--, p += 64) {
      const __m128i abcd_save = abcd, e_save = e0;
      __m128i m0 = _mm_shuffle_epi8(_mm_loadu_si128((const __m128i*)(p + 0)), bswap);
      __m128i m1 = _mm_shuffle_epi8(_mm_loadu_si128((const __m128i*)(p + 16)), bswap);
      __m128i m2 = _mm_shuffle_epi8(_mm_loadu_si128((const __m128i*)(p + 32)), bswap);
      __m128i m3 = _mm_shuffle_epi8(_mm_loadu_si128((const __m128i*)(p + 48)), bswap);
// one group: ec = this group's e, eo = the other e register; mc = this group's message words,
// mn / mp / mq = the next, previous and second-previous message registers
#define XS_G(fn, ec, eo, mc, mn, mp, mq, msg2, msg1, mix) \
  ec = _mm_sha1nexte_epu32(ec, mc);                       \
  eo = abcd;                                              \
  if (msg2) mn = _mm_sha1msg2_epu32(mn, mc);              \
  abcd = _mm_sha1rnds4_epu32(abcd, ec, fn);               \
  if (msg1) mp = _mm_sha1msg1_epu32(mp, mc);              \
  if (mix) mq = _mm_xor_si128(mq, mc)
      e0 = _mm_add_epi32(e0, m0);  // group 0: e is added, not derived
      e1 = abcd;
      abcd = _mm_sha1rnds4_epu32(abcd, e0, 0);
      XS_G(0, e1, e0, m1, m2, m0, m3, 0, 1, 0);
      XS_G(0, e0, e1, m2, m3, m1, m0, 0, 1, 1);
      XS_G(0, e1, e0, m3, m0, m2, m1, 1, 1, 1);
      XS_G(0, e0, e1, m0, m1, m3, m2, 1, 1, 1);
      XS_G(1, e1, e0, m1, m2, m0, m3, 1, 1, 1);
      XS_G(1, e0, e1, m2, m3, m1, m0, 1, 1, 1);
      XS_G(1, e1, e0, m3, m0, m2, m1, 1, 1, 1);
      XS_G(1, e0, e1, m0, m1, m3, m2, 1, 1, 1);
      XS_G(1, e1, e0, m1, m2, m0, m3, 1, 1, 1);
      XS_G(2, e0, e1, m2, m3, m1, m0, 1, 1, 1);
      XS_G(2, e1, e0, m3, m0, m2, m1, 1, 1, 1);
      XS_G(2, e0, e1, m0, m1, m3, m2, 1, 1, 1);
      XS_G(2, e1, e0, m1, m2, m0, m3, 1, 1, 1);
      XS_G(2, e0, e1, m2, m3, m1, m0, 1, 1, 1);
      XS_G(3, e1, e0, m3, m0, m2, m1, 1, 1, 1);
      XS_G(3, e0, e1, m0, m1, m3, m2, 1, 1, 1);
      XS_G(3, e1, e0, m1, m2, m0, m3, 1, 0, 1);
      XS_G(3, e0, e1, m2, m3, m1, m0, 1, 0, 0);
      XS_G(3, e1, e0, m3, m0, m2, m1, 0, 0, 0);
#undef XS_G
      e0 = _mm_sha1nexte_epu32(e0, e_save);
      abcd = _mm_add_epi32(abcd, abcd_save);
    }
    abcd = _mm_shuffle_epi32(abcd, 0x1b);
    _mm_storeu_si128((__m128i*)h, abcd);
    h[4] = (uint32_t)_mm_extract_epi32(e0, 3);
  }
#endif
};

}  // namespace xs
