// Host LZ4 page decoder (Parquet codecs 7, LZ4_RAW, and 5, Hadoop-framed LZ4; the rules are lz4_fmt.h's,
// which the device kernel walks too). No liblz4: the project carries its own, as it does for SNAPPY,
// GZIP and ZSTD.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "lz4_fmt.h"

namespace dr {
// Decodes the page body `in[0..n)` into `out[0..out_len)`: one bare block (framing lz4::F_BARE) or
// Hadoop units (lz4::F_HADOOP). True only if the output fills exactly out_len bytes. `why` (optional)
// receives the lz4::Err code.
bool lz4_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t out_len, uint32_t framing, int* why = nullptr);

namespace lz4 {
// The bare block in[at, at + n) into out[0, cap); *produced receives its output length.
inline int decode_block(const PtrSrc& src, const uint8_t* in, uint64_t at, uint64_t n, uint8_t* out, uint64_t cap,
                        uint64_t* produced) {
  Block b{};
  begin(b, at, n, cap);
  uint64_t op = 0;
  for (;;) {
    Seq q{};
    if (const int e = next(src, b, &q)) return e;
    if (uint64_t(q.ll) + q.ml > cap - op) return E_OUTPUT;  // next() has checked it: kept for the copies below
    if (q.ll) memcpy(out + op, in + q.lit, q.ll);
    op += q.ll;
    for (uint32_t k = 0; k < q.ml; ++k) out[op + k] = out[op - q.off + k];  // overlap-safe
    op += q.ml;
    if (q.last) break;
  }
  *produced = op;
  return E_OK;
}

// A page body, as the lz4::Err code. Inline, so that a unit which needs a page decoded (the host
// decoders of parquet_meta.cpp) links without lz4_host.cpp.
inline int decode_page(const uint8_t* in, size_t n, uint8_t* out, size_t out_len, uint32_t framing) {
  const PtrSrc src{in, n};
  uint64_t op = 0;
  if (framing == F_BARE) {
    if (const int e = decode_block(src, in, 0, n, out, out_len, &op)) return e;
    return op == out_len ? E_OK : E_OUTPUT;
  }
  uint64_t pos = 0;
  while (pos < n) {
    uint32_t U = 0;
    if (const int e = unit_header(src, pos, n, out_len - op, &U)) return e;
    for (uint64_t left = U; left;) {
      uint32_t C = 0;
      uint64_t got = 0;
      if (const int e = inner_header(src, pos, n, &C)) return e;
      if (const int e = decode_block(src, in, pos, C, out + op, left, &got)) return e;
      pos += C;
      op += got;
      left -= got;
    }
  }
  return op == out_len ? E_OK : E_OUTPUT;
}
}  // namespace lz4
}  // namespace dr
