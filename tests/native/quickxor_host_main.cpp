// TEST INFRASTRUCTURE: stand-alone driver of xs::HostQuickXor (rclone_amd/csrc/xs_host_quickxor.h),
// built by tests/test_quickxor_cpu.py with the host compiler under AddressSanitizer + UBSan and run
// as its own process.  It feeds one buffer of 4003 bytes (byte i = 131 i + 7 mod 256) in pieces of
// 1, 7, 16, 64, 100, 160 and 1760 bytes and whole (piece 0), calls final() after every piece -- the
// encrypter's tee reads the digest after any read and goes on hashing -- and prints one line per
// digest:
//   <piece> <bytes fed so far> <hex digest>
// The test compares every line with its own restatement of the hash over the bytes fed so far.
#include <cstdio>
#include <vector>

#include "../../rclone_amd/csrc/xs_host_quickxor.h"

int main() {
  static const size_t pieces[] = {1, 7, 16, 64, 100, 160, 1760, 0};
  const size_t len = 4003;
  std::vector<uint8_t> buf(len);
  for (size_t i = 0; i < len; i++) buf[i] = (uint8_t)(131 * i + 7);
  for (size_t piece : pieces) {
    xs::HostQuickXor h;
    const size_t step = piece ? piece : len;
    for (size_t pos = 0; pos < len; pos += step) {
      h.update(buf.data() + pos, step < len - pos ? step : len - pos);
      const size_t fed = pos + step < len ? pos + step : len;
      xs::HostQuickXor copy = h;  // the state is copyable: both give the same digest
      uint8_t out[20], again[20], out2[20];
      h.final(out);
      h.final(again);  // final() leaves the state alone
      copy.final(out2);
      if (memcmp(out, again, 20) != 0 || memcmp(out, out2, 20) != 0) {
        fprintf(stderr, "final() disturbed the state at piece %zu fed %zu\n", piece, fed);
        return 1;
      }
      printf("%zu %zu ", piece, fed);
      for (int i = 0; i < 20; i++) printf("%02x", out[i]);
      printf("\n");
    }
  }
  return 0;
}
