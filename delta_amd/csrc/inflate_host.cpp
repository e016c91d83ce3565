#include "inflate_host.h"

namespace dr {

bool gzip_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t out_len, int* why) {
  const int e = dfl::inflate_members(in, n, out, out_len);
  if (why) *why = e;
  return e == dfl::E_OK;
}

}  // namespace dr
