#include "zstd_host.h"

namespace dr {

bool zstd_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t out_len, int* why) {
  const int e = zst::decode_frames(in, n, out, out_len);
  if (why) *why = e;
  return e == zst::E_OK;
}

}  // namespace dr
