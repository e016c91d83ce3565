// Host build of the K5 pattern matcher (delta_amd/csrc/like_lane.h: the device's own like_match and
// bytewise tests, and the host's pattern compiler) for tests/test_like_lane.py.
#include "../../delta_amd/csrc/like_lane.h"

#include <cstring>

using namespace dr::lk;

extern "C" {

// Compiles pattern[0, n) with `escape`: 0 and *kind (LikeKind) / out[0, *outlen) (the needle or the
// program), or 1 and the message in err.
int lk_compile(const uint8_t* pattern, uint32_t n, uint32_t escape, int* kind, uint8_t* out, uint32_t cap,
               uint32_t* outlen, char* err, uint32_t errcap) {
  const LikeCompiled c = like_compile(pattern, n, escape);
  if (!c.error.empty()) {
    std::strncpy(err, c.error.c_str(), errcap - 1);
    err[errcap - 1] = 0;
    return 1;
  }
  if (c.text.size() > cap) return 2;
  *kind = c.kind;
  *outlen = uint32_t(c.text.size());
  std::memcpy(out, c.text.data(), c.text.size());
  return 0;
}

// The compiled form against a value, as the evaluators apply it.
int lk_eval(int kind, const uint8_t* s, uint32_t n, const uint8_t* t, uint32_t tn) {
  switch (kind) {
    case LIKE_EQ: return n == tn && bytes_eq(s, t, n);
    case LIKE_STARTSWITH: return starts_with(s, n, t, tn);
    case LIKE_ENDSWITH: return ends_with(s, n, t, tn);
    case LIKE_CONTAINS: return contains(s, n, t, tn);
    default: return like_match(s, n, t, tn);
  }
}

}  // extern "C"
