// K2: the DELTA_* Parquet value encodings (5 DELTA_BINARY_PACKED, 6 DELTA_LENGTH_BYTE_ARRAY,
// 7 DELTA_BYTE_ARRAY) as the host decoder (parquet_meta.cpp) and the device kernels (k_parquet.hip)
// both read them: varints, the packed header, the per-block step, the unpacking and the value
// arithmetic. Plain C++, no HIP type: g++ compiles it, and hipcc compiles it as device code.
//
// A packed sequence is
//   <block size> <miniblocks per block> <total count> <first value: zigzag>          (ULEB128 each)
//   then per block: <min delta: zigzag> <one width byte per miniblock> <miniblocks, LSB-first packed>
// Value i (i >= 1) is value i-1 + min delta + delta i-1, wrapping in 64 bits. The last block holds only
// the miniblocks that carry a value; the width bytes of the others are padding and are not looked at.
#pragma once
#include <cstdint>
#include "filter_plan.h"  // DR_HD

namespace dr {
namespace denc {

// Bytes [0, n) behind a pointer; -1 past the end. The device walks block headers through a reader
// of its own (an LDS window over the same bytes).
struct PtrReader {
  const uint8_t* b;
  uint64_t n;
  DR_HD int operator()(uint64_t pos) const { return pos < n ? int(b[pos]) : -1; }
};

// ULEB128 at `pos` (advanced past it). False: the varint runs past the end or past 10 bytes.
template <class R>
DR_HD inline bool uleb(const R& rd, uint64_t& pos, uint64_t* out) {
  uint64_t v = 0;
  for (int s = 0; s < 70; s += 7) {
    const int b = rd(pos);
    if (b < 0) return false;
    ++pos;
    v |= uint64_t(b & 0x7f) << (s & 63);
    if (!(b & 0x80)) {
      *out = v;
      return true;
    }
  }
  return false;
}
template <class R>
DR_HD inline bool zigzag(const R& rd, uint64_t& pos, int64_t* out) {
  uint64_t u;
  if (!uleb(rd, pos, &u)) return false;
  *out = int64_t((u >> 1) ^ (~(u & 1) + 1));
  return true;
}

struct DbpHeader {
  uint32_t block;    // values per block: a non-zero multiple of 128
  uint32_t nmb;      // miniblocks per block
  uint32_t mbv;      // values per miniblock: a multiple of 32
  uint32_t count;    // values of the sequence (the first one included)
  int64_t first;
};
// The header at `pos`. `max_count`: the page's defined levels (a sequence never holds more).
template <class R>
DR_HD inline bool dbp_header(const R& rd, uint64_t& pos, uint64_t max_count, DbpHeader* h) {
  uint64_t block, nmb, count;
  if (!uleb(rd, pos, &block) || !uleb(rd, pos, &nmb) || !uleb(rd, pos, &count) || !zigzag(rd, pos, &h->first))
    return false;
  if (block == 0 || block % 128 != 0 || block > (uint64_t(1) << 30)) return false;
  if (nmb == 0 || nmb > block || block % nmb != 0 || (block / nmb) % 32 != 0) return false;
  if (count > max_count) return false;
  h->block = uint32_t(block);
  h->nmb = uint32_t(nmb);
  h->mbv = uint32_t(block / nmb);
  h->count = uint32_t(count);
  return true;
}
DR_HD inline uint64_t dbp_blocks(const DbpHeader& h) {  // blocks that follow the header
  return h.count <= 1 ? 0 : (uint64_t(h.count) - 1 + h.block - 1) / h.block;
}

struct DbpBlock {
  int64_t min_delta;
  uint64_t w_pos;     // the width bytes (nmb of them); the miniblocks start at w_pos + nmb
  uint64_t next_pos;  // the byte after the block's last present miniblock
  uint32_t used;      // miniblocks present
};
// The block at `pos` holding the next `left` deltas (left >= 1; a block takes at most h.block of
// them). max_w: 64, or 32 for an INT32 column. False: a varint or the block runs past the end, or a
// present miniblock's width exceeds max_w.
template <class R>
DR_HD inline bool dbp_block(const R& rd, uint64_t pos, uint64_t end, const DbpHeader& h, uint64_t left, int max_w,
                            DbpBlock* b) {
  if (!zigzag(rd, pos, &b->min_delta)) return false;
  b->w_pos = pos;
  if (end - pos < h.nmb) return false;
  const uint64_t here = left < h.block ? left : h.block;
  b->used = uint32_t((here + h.mbv - 1) / h.mbv);
  uint64_t bytes = 0;
  for (uint32_t m = 0; m < b->used; ++m) {
    const int w = rd(pos + m);
    if (w < 0 || w > max_w) return false;
    bytes += uint64_t(w) * (h.mbv / 8);
  }
  pos += h.nmb;
  if (end - pos < bytes) return false;
  b->next_pos = pos + bytes;
  return true;
}

// Value j of a miniblock of width w (0..64) that starts at mb: LSB-first. Reads the bytes that hold
// the value's bits and no other.
DR_HD inline uint64_t dbp_unpack(const uint8_t* mb, uint32_t w, uint32_t j) {
  if (w == 0) return 0;
  const uint64_t bit = uint64_t(j) * w;
  const uint8_t* p = mb + (bit >> 3);
  const uint32_t sh = uint32_t(bit & 7), nb = (sh + w + 7) >> 3;  // nb <= 9
  uint64_t lo = 0;
  for (uint32_t k = 0; k < nb && k < 8; ++k) lo |= uint64_t(p[k]) << (8 * k);
  uint64_t v = lo >> sh;
  if (nb == 9) v |= uint64_t(p[8]) << (64 - sh);
  return w == 64 ? v : v & ((uint64_t(1) << w) - 1);
}

// Delta d (0-based: it leads from value d to value d + 1) of a sequence whose block `bi = d / block`
// was parsed into (w_pos): its unpacked bits. `base` addresses position 0 of the reader.
DR_HD inline uint64_t dbp_delta(const uint8_t* base, const DbpHeader& h, uint64_t w_pos, uint32_t r) {
  const uint32_t m = r / h.mbv, j = r % h.mbv;
  const uint8_t* wb = base + w_pos;
  uint64_t off = 0;
  for (uint32_t q = 0; q < m; ++q) off += uint64_t(wb[q]) * (h.mbv / 8);
  return dbp_unpack(wb + h.nmb + off, wb[m], j);
}

// value + min delta + delta, wrapping; an INT32 column keeps the low 32 bits, sign-extended.
DR_HD inline int64_t dbp_step(int64_t prev, int64_t min_delta, uint64_t delta) {
  return int64_t(uint64_t(prev) + uint64_t(min_delta) + delta);
}
DR_HD inline int64_t dbp_narrow32(int64_t v) { return int64_t(int32_t(uint32_t(uint64_t(v)))); }

}  // namespace denc
}  // namespace dr
