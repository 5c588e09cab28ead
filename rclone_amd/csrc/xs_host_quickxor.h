// xs_host_quickxor.h -- QuickXorHash on a host core: the ciphertext hash for wrapped remotes whose
// Hashes().GetOne() is "quickxor" (OneDrive Personal, Business and SharePoint;
// backend/onedrive/quickxorhash/quickxorhash.go:69-111), with the call shape of HostSha1
// (xs_host_sha1.h).  It serves the per-object streams (md5_workers.h) and xs_host_hash:
// QuickXorHash("RCLONE\0\0" || nonce || wire blocks).
//
// The hash: stream byte i (0-based) is XORed into a 160-bit ring at bit (11 i) mod 160, bits past
// 159 wrapping to bit 0; the ring is written as 20 little-endian bytes and the stream length, a
// 64-bit little-endian value, is XORed into bytes 12..19.  11 * 160 is a multiple of 160, so bytes
// i and i + 160 meet the same bit: the state kept here is the column-wise XOR of the stream in
// rows of 160 bytes, and update() is a word-wise XOR the compiler vectorises.  The fold of that row
// into the ring happens in final(), which leaves the state alone: the encrypter's tee reads the
// digest of exactly the bytes returned so far after any read and goes on hashing.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace xs {

class HostQuickXor {
 public:
  static constexpr size_t kRow = 160;  // bytes after which the bit position repeats

  void update(const uint8_t* p, size_t len) {
    if (len == 0) return;
    size_t col = (size_t)(n_ % kRow);
    n_ += len;
    if (col) {  // up to the next row boundary
      size_t k = kRow - col < len ? kRow - col : len;
      for (size_t j = 0; j < k; j++) row_[col + j] ^= p[j];
      p += k;
      len -= k;
    }
    // whole rows, word-wise (memcpy: p is not aligned)
    while (len >= kRow) {
      uint64_t a[kRow / 8], b[kRow / 8];
      memcpy(a, row_, kRow);
      memcpy(b, p, kRow);
      for (size_t j = 0; j < kRow / 8; j++) a[j] ^= b[j];
      memcpy(row_, a, kRow);
      p += kRow;
      len -= kRow;
    }
    for (size_t j = 0; j < len; j++) row_[j] ^= p[j];
  }

  // digest of the bytes fed so far; the state is not disturbed
  void final(uint8_t out[20]) const {
    uint8_t ring[21] = {0};  // one spare byte: a byte placed at bit 152 + s spills into ring[20]
    for (size_t k = 0; k < kRow; k++) {
      const unsigned bit = (unsigned)(11 * k % 160);
      const unsigned v = (unsigned)row_[k] << (bit & 7);
      ring[bit >> 3] ^= (uint8_t)v;
      ring[(bit >> 3) + 1] ^= (uint8_t)(v >> 8);
    }
    ring[0] ^= ring[20];  // bits past 159 wrap to bit 0
    memcpy(out, ring, 20);
    for (int j = 0; j < 8; j++) out[12 + j] ^= (uint8_t)(n_ >> (8 * j));
  }

 private:
  uint8_t row_[kRow] = {0};
  uint64_t n_ = 0;
};

}  // namespace xs
