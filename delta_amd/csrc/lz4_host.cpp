#include "lz4_host.h"

namespace dr {

bool lz4_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t out_len, uint32_t framing, int* why) {
  const int e = lz4::decode_page(in, n, out, out_len, framing);
  if (why) *why = e;
  return e == lz4::E_OK;
}

}  // namespace dr
