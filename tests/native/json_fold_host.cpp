// Host build of the K1 line walker (delta_amd/csrc/json_lane.h) for tests/test_json_fold.py: the
// whole-line walk of both instantiations, the token stream of a line, and the bulk kernel's
// two-phase walk (tokens into a bounded buffer, flushed through the DFA) restated for one line.
// Test infrastructure only.
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

void store(const dr::jl::LineOut& o, unsigned char* kind, unsigned char* flags, unsigned* path_off, unsigned* path_len,
           long long* size, long long* delts) {
  *kind = o.kind;
  *flags = o.flags;
  *path_off = o.path_off;
  *path_len = o.path_len;
  *size = o.size;
  *delts = o.delts;
}
}  // namespace

extern "C" int jf_parse(const unsigned char* line, unsigned n, unsigned align, int general, unsigned char* kind,
                        unsigned char* flags, unsigned* path_off, unsigned* path_len, long long* size,
                        long long* delts) {
  Placed pl(line, n, align);
  dr::jl::LineOut o;
  if (general) dr::jl::parse_line_general(pl.p, n, o);
  else dr::jl::parse_line(pl.p, n, o);
  store(o, kind, flags, path_off, path_len, size, delts);
  return o.hard;
}

// The tokens of the line (General: tab / CR are whitespace) into out[0..cap); returns their number,
// or -1 - status when the tokenizer stopped (ST_BAD / ST_HARD).
extern "C" int jf_tokens(const unsigned char* line, unsigned n, unsigned align, int general, unsigned* out, int cap) {
  using namespace dr::jl;
  Placed pl(line, n, align);
  Tokenizer tz;
  int nt = 0;
  auto push = [&](uint32_t t) {
    if (nt < cap) out[nt] = t;
    ++nt;
  };
  const uint32_t o0 = align & 15;
  const uint32_t nwin = (o0 + n + 15) >> 4;
  for (uint32_t j = 0; j < nwin && tz.status == ST_OK; ++j) {
    uint32_t w[4];
    load_window(pl.p - o0 + 16u * j, w);
    if (general) tokenize_window<true>(pl.p, n, w, int32_t(16u * j) - int32_t(o0), tz, push);
    else tokenize_window<false>(pl.p, n, w, int32_t(16u * j) - int32_t(o0), tz, push);
  }
  tokenize_end(n, tz, push);
  return tz.status == ST_OK ? nt : -1 - int(tz.status);
}

// walk_line of k_json.hip for one lane: tokens go to a buffer of `cap` slots, which runs through the
// DFA when it holds more than `flush` tokens after a window, and at the end. Returns the hard flag,
// or -1 if a window would have written past the buffer.
extern "C" int jf_parse_buffered(const unsigned char* line, unsigned n, unsigned align, int cap, int flush,
                                 unsigned char* kind, unsigned char* flags, unsigned* path_off, unsigned* path_len,
                                 long long* size, long long* delts, int* nflush) {
  using namespace dr::jl;
  Placed pl(line, n, align);
  Tokenizer tz;
  Dfa<false> d;
  if (n > TOK_MAX_LINE) tz.status = ST_HARD;
  std::vector<uint32_t> buf(size_t(cap), 0u);
  int nt = 0;
  bool over = false;
  auto push = [&](uint32_t t) {
    if (nt < cap) buf[size_t(nt)] = t;
    else over = true;
    ++nt;
  };
  const uint32_t o0 = align & 15;
  const uint32_t nwin = tz.status == ST_OK ? (o0 + n + 15) >> 4 : 0;
  *nflush = 0;
  for (uint32_t j = 0;; ++j) {
    if (j < nwin && tz.status == ST_OK) {
      uint32_t w[4];
      load_window(pl.p - o0 + 16u * j, w);
      tokenize_window<false>(pl.p, n, w, int32_t(16u * j) - int32_t(o0), tz, push);
      if (j + 1 == nwin) tokenize_end(n, tz, push);
    }
    const bool more = j + 1 < nwin && tz.status == ST_OK;
    if (!more || nt > flush) {
      for (int t = 0; t < nt && t < cap; ++t)
        if (d.status == ST_OK) dfa_token<false>(pl.p, buf[size_t(t)], d);
      nt = 0;
      ++*nflush;
    }
    if (!more) break;
  }
  if (over) return -1;
  LineOut o;
  dfa_finish<false>(tz, d, o);
  store(o, kind, flags, path_off, path_len, size, delts);
  return o.hard;
}
