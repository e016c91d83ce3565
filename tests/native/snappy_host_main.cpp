// Runs the host SNAPPY decoder (snappy_host.cpp) over records read from a file, for
// tests/test_snappy_host.py. A record is <u32 n_out> <u32 n_in> <u8 unused> <n_in bytes>, little endian;
// per record the program prints the output in hex ("-" for an empty one), or "error".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "snappy_host.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> all;
  uint8_t chunk[1 << 16];
  for (size_t k; (k = std::fread(chunk, 1, sizeof chunk, f)) > 0;) all.insert(all.end(), chunk, chunk + k);
  std::fclose(f);
  auto u32 = [&](size_t at) {
    return uint32_t(all[at]) | uint32_t(all[at + 1]) << 8 | uint32_t(all[at + 2]) << 16 | uint32_t(all[at + 3]) << 24;
  };
  size_t at = 0;
  std::vector<char> line;
  while (at + 9 <= all.size()) {
    const uint32_t n_out = u32(at), n_in = u32(at + 4);
    at += 9;
    if (n_in > all.size() - at) return 3;
    // exact-size copies, so that the sanitizer sees a read or a write one byte out of range
    std::vector<uint8_t> in(all.begin() + at, all.begin() + at + n_in), out(n_out);
    at += n_in;
    if (!dr::snappy_decompress(in.data(), in.size(), out.data(), out.size())) {
      std::printf("error\n");
      continue;
    }
    line.assign(size_t(n_out) * 2 + 2, 0);
    size_t w = 0;
    for (uint8_t b : out) {
      line[w++] = "0123456789abcdef"[b >> 4];
      line[w++] = "0123456789abcdef"[b & 15];
    }
    if (!n_out) line[w++] = '-';
    line[w++] = '\n';
    std::fwrite(line.data(), 1, w, stdout);
  }
  return at == all.size() ? 0 : 3;
}
