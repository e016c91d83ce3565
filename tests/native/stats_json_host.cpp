// Host build of delta_amd/csrc/stats_json.h, run stand-alone by tests/test_stats_json.py (once plain, once
// with -fsanitize=address,undefined): reads a case file, runs locate() over every case and prints one
// line per case. The file: u32 nwant, then per want {i32 source, u32 path_len, path bytes}; then u32
// ncases and per case {u32 len, bytes}. Every case is copied into a heap block of exactly its length, so
// that a read past n is a sanitizer report. Output per case: `kind:offset:len` for every want, joined
// by spaces (offset -1 when there is no token).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../delta_amd/csrc/stats_json.h"

using namespace dr;

static bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t nwant = 0, ncases = 0;
  if (!rd(f, &nwant, 4) || nwant > uint32_t(PV_MAXC)) return 2;
  std::vector<std::string> paths(nwant);
  std::vector<sj::Want> want(nwant);
  for (uint32_t w = 0; w < nwant; ++w) {
    int32_t src;
    uint32_t len;
    if (!rd(f, &src, 4) || !rd(f, &len, 4)) return 2;
    paths[w].resize(len);
    if (len && !rd(f, &paths[w][0], len)) return 2;
    want[w] = sj::Want{src, reinterpret_cast<const uint8_t*>(paths[w].data()), len};
  }
  if (!rd(f, &ncases, 4)) return 2;
  std::vector<sj::Found> found(nwant);
  for (uint32_t c = 0; c < ncases; ++c) {
    uint32_t len;
    if (!rd(f, &len, 4)) return 2;
    uint8_t* s = static_cast<uint8_t*>(malloc(len ? len : 1));  // exactly the case's bytes (an empty one: never read)
    if (len && !rd(f, s, len)) return 2;
    sj::locate(len ? s : nullptr, len, want.data(), int(nwant), found.data());
    for (uint32_t w = 0; w < nwant; ++w)
      printf("%s%d:%ld:%u", w ? " " : "", int(found[w].kind), found[w].ptr ? long(found[w].ptr - s) : -1L, found[w].len);
    printf("\n");
    free(s);
  }
  fclose(f);
  return 0;
}
