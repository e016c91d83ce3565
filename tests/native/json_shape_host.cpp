// Host build of the writer-shape matcher (match_writer_line, delta_amd/csrc/json_lane.h) for
// tests/test_json_shape.py: a line is tokenized by the fast tokenizer into a strided token buffer (as
// the bulk kernel's lanes do), the matcher runs over the buffer, and the General walker decides the
// same line independently. With JS_MAIN the same source is a stand-alone program that checks
// "accept => every field equals the general walk, which is an add or a remove" over a file of
// lines at every alignment (built with AddressSanitizer + UBSan by the test). Test infrastructure only.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../delta_amd/csrc/json_lane.h"

namespace {
struct Placed {
  std::vector<unsigned char> buf;
  unsigned char* p;
  // the line at the requested alignment inside a 16-byte aligned, padded buffer filled with bytes
  // that must never influence the result
  Placed(const unsigned char* line, unsigned n, unsigned align) : buf(n + 64 + 32) {
    unsigned char* base = buf.data();
    while (reinterpret_cast<uintptr_t>(base) & 15) ++base;
    std::memset(buf.data(), '"', buf.size());
    p = base + (align & 15);
    std::memcpy(p, line, n);
  }
};

constexpr uint32_t STRIDE = 3;  // tokens are read through the stride, as from a lane's LDS column

// Returns 1 if the matcher accepted; m = its LineOut (zeroed when declined), g = the general walk's.
int check(const unsigned char* line, unsigned n, unsigned align, dr::jl::LineOut& m, dr::jl::LineOut& g) {
  using namespace dr::jl;
  Placed pl(line, n, align);
  parse_line_general(pl.p, n, g);
  m = LineOut{0, 0, 0, 0, 0, 0, 0};
  Tokenizer tz;
  if (n > TOK_MAX_LINE) tz.status = ST_HARD;
  // every slot the matcher must not read holds a token that would match a writer's line nowhere
  std::vector<uint32_t> tok((size_t(n) + 8) * STRIDE, tok_make(0, 0, T_ARR_CLOSE));
  uint32_t nt = 0;
  auto push = [&](uint32_t t) { tok[size_t(nt++) * STRIDE] = t; };
  const uint32_t o0 = align & 15;
  const uint32_t nwin = tz.status == ST_OK ? (o0 + n + 15) >> 4 : 0;
  for (uint32_t j = 0; j < nwin && tz.status == ST_OK; ++j) {
    uint32_t w[4];
    load_window(pl.p - o0 + 16u * j, w);
    tokenize_window<false>(pl.p, n, w, int32_t(16u * j) - int32_t(o0), tz, push);
    if (j + 1 == nwin) tokenize_end(n, tz, push);
  }
  // exactly nt slots: a read at or past nt is a heap overflow under the sanitizer
  std::vector<uint32_t> col(tok.begin(), tok.begin() + (nt ? (size_t(nt) - 1) * STRIDE + 1 : 0));
  LineOut o{0, 0, 0, 0, 0, 0, 0};
  if (!match_writer_line(pl.p, n, col.data(), STRIDE, nt, tz, o)) return 0;
  m = o;
  return 1;
}

void store(const dr::jl::LineOut& o, long long* r) {
  r[0] = o.kind;
  r[1] = o.flags;
  r[2] = o.hard;
  r[3] = o.path_off;
  r[4] = o.path_len;
  r[5] = o.size;
  r[6] = o.delts;
}
}  // namespace

// matched[7] / general[7]: kind, flags, hard, path_off, path_len, size, delts. Returns the accept flag.
extern "C" int js_check(const unsigned char* line, unsigned n, unsigned align, long long* matched, long long* general) {
  dr::jl::LineOut m, g;
  const int acc = check(line, n, align, m, g);
  store(m, matched);
  store(g, general);
  return acc;
}

#ifdef JS_MAIN
// argv[1]: lines as (u32 little-endian length, bytes)*. Prints "lines N accepted A" (A over every
// alignment); exit status 1 and the line on the first violation of the property.
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  unsigned long lines = 0, accepted = 0;
  for (;;) {
    unsigned char h[4];
    if (std::fread(h, 1, 4, f) != 4) break;
    const unsigned n = h[0] | (h[1] << 8) | (h[2] << 16) | (unsigned(h[3]) << 24);
    std::vector<unsigned char> line(n + 1);
    if (n && std::fread(line.data(), 1, n, f) != n) return 2;
    ++lines;
    for (unsigned align = 0; align < 16; ++align) {
      long long m[7], g[7];
      if (!js_check(line.data(), n, align, m, g)) continue;
      ++accepted;
      if (std::memcmp(m, g, sizeof m) != 0 || !(g[0] == dr::jl::K_ADD || g[0] == dr::jl::K_REMOVE)) {
        std::fprintf(stderr, "mismatch at align %u: %.*s\n", align, int(n), reinterpret_cast<const char*>(line.data()));
        return 1;
      }
    }
  }
  std::fclose(f);
  std::printf("lines %lu accepted %lu\n", lines, accepted);
  return 0;
}
#endif
