// TEST INFRASTRUCTURE: stand-alone driver of xs::HostSha1 (rclone_amd/csrc/xs_host_sha1.h), built by
// tests/test_sha1_cpu.py with the host compiler under AddressSanitizer + UBSan and run as its own
// process.  For each length it feeds the buffer (byte i = 131 i + 7 mod 256) in pieces of 1, 7, 64
// and 100 bytes and whole (piece 0), with the portable block function and, where the CPU has the
// SHA extensions, with those too, and prints one line per digest:
//   <impl> <len> <piece> <hex digest>
// The test compares every line with hashlib.sha1.
#include <cstdio>
#include <vector>

#include "../../rclone_amd/csrc/xs_host_sha1.h"

static void run(const char* impl, bool portable_only) {
  static const size_t lens[] = {0, 1, 55, 56, 63, 64, 65, 119, 120, 128, 1000, 65584};
  static const size_t pieces[] = {1, 7, 64, 100, 0};
  for (size_t len : lens) {
    std::vector<uint8_t> buf(len);
    for (size_t i = 0; i < len; i++) buf[i] = (uint8_t)(131 * i + 7);
    for (size_t piece : pieces) {
      xs::HostSha1 h(portable_only);
      if (piece == 0) {
        h.update(buf.data(), len);
      } else {
        for (size_t pos = 0; pos < len; pos += piece) h.update(buf.data() + pos, piece < len - pos ? piece : len - pos);
      }
      xs::HostSha1 copy = h;  // the state is copyable: both finish alike
      uint8_t out[20], out2[20];
      h.final(out);
      copy.final(out2);
      if (memcmp(out, out2, 20) != 0) {
        fprintf(stderr, "copied state differs at len %zu piece %zu\n", len, piece);
        return;
      }
      printf("%s %zu %zu ", impl, len, piece);
      for (int i = 0; i < 20; i++) printf("%02x", out[i]);
      printf("\n");
    }
  }
}

int main() {
  run("portable", true);
  if (xs::HostSha1::has_shani()) run("shani", false);
  printf("shani %d\n", xs::HostSha1::has_shani() ? 1 : 0);
  return 0;
}
