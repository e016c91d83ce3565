// Host GZIP page inflater (RFC 1952 members around RFC 1951 streams; the rules are deflate_fmt.h's,
// which the device kernel walks too). No zlib: the project carries its own, as it does for SNAPPY.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>

#include "deflate_fmt.h"

namespace dr {
// Inflates the concatenated gzip members `in[0..n)` into `out[0..out_len)`. True only if the
// members' outputs fill exactly out_len bytes and each member's ISIZE is its output length mod 2^32;
// the CRC32 is not verified. `why` (optional) receives the dfl::Err code.
bool gzip_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t out_len, int* why = nullptr);

namespace dfl {
// The same, as the dfl::Err code. Inline, so that a unit which needs a page inflated (the host
// decoders of parquet_meta.cpp) links without inflate_host.cpp.
inline int inflate_members(const uint8_t* in, size_t n, uint8_t* out, size_t out_len) {
  const PtrSrc src{in, n};
  auto tables = std::make_unique<Tables>();
  Tables& T = *tables;
  uint64_t pos = 0;
  size_t op = 0;
  do {
    if (const int e = gz_header(src, pos)) return e;
    const size_t member = op;
    Bits<PtrSrc> br(src, pos * 8);
    for (;;) {
      Block b{};
      if (const int e = block_header(br, T, &b)) return e;
      if (b.kind == BK_STORED) {
        const uint64_t at = br.bitpos() / 8;
        if (b.stored_len > n - at) return E_INPUT;
        if (b.stored_len > out_len - op) return E_OUTPUT;
        if (b.stored_len) memcpy(out + op, in + at, b.stored_len);
        op += b.stored_len;
        br.seek(at + b.stored_len);
      } else {
        if (const int e = build_codes(T, b, 0, 1, NoSync())) return e;
        for (;;) {
          Symbol s{};
          if (const int e = next_symbol(br, T, &s)) return e;
          if (s.kind == SY_END) break;
          if (s.kind == SY_LITERAL) {
            if (op >= out_len) return E_OUTPUT;
            out[op++] = uint8_t(s.value);
            continue;
          }
          if (s.dist > op - member) return E_DISTANCE;
          if (s.value > out_len - op) return E_OUTPUT;
          for (uint32_t k = 0; k < s.value; ++k) out[op + k] = out[op - s.dist + k];  // overlap-safe
          op += s.value;
        }
      }
      if (b.final) break;
    }
    br.align();
    pos = br.bitpos() / 8;
    if (const int e = gz_trailer(src, pos, op - member)) return e;
  } while (pos < n);
  return op == out_len ? E_OK : E_OUTPUT;
}
}  // namespace dfl
}  // namespace dr
