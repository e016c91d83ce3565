// K2: LZ4 pages (Parquet CompressionCodec 7, LZ4_RAW: one bare LZ4 block per page; and codec 5, LZ4:
// Hadoop's BlockCompressorStream framing around bare blocks) as the host decoder (lz4_host.h) and the
// device kernel (k_lz4.hip) both read them. Plain C++, no HIP type and no allocation: g++ compiles it,
// and hipcc compiles it as device code. A byte stream takes the same decisions on both sides because
// both walk these functions.
//
// A block is a run of sequences: a token (high nibble: literal length, low nibble: match length - 4),
// the literal length's extension bytes (each adds its value; the first below 255 ends the run), the
// literals, a 2-byte little-endian offset, the match length's extension bytes. The last sequence is
// literals only and ends exactly at the end of the input.
//
// What a block is accepted for is what liblz4's LZ4_decompress_safe accepts when its destination
// capacity is the number of bytes the block may still produce (the page's declared size, or what is
// left of a Hadoop unit), followed by the caller's check that the page came out at its declared size.
// next() below is that function's control flow without its copies. It differs from the LZ4 block
// format note ("the last five bytes are literals", "the last match starts at least twelve bytes before
// the end") where liblz4 does:
//   - the end-of-block conditions count from the capacity, not from the block's own length: a block that
//     produces less than the capacity may end in a match (the caller refuses a short page, so this
//     shows only in Hadoop units of several inner blocks);
//   - a non-final literal run must end 12 bytes before the capacity and 8 bytes before the end of the
//     input, and a match must end 5 bytes before the capacity -- but liblz4 checks neither on its
//     fast paths. In its first loop (taken while the capacity is 64 or more): a literal run below 15
//     with at least 17 bytes of input behind its token, and any match that ends more than 64 bytes
//     before the capacity. In its second loop (entered for good by the first sequence that comes
//     within 64 bytes of the capacity or fails the first loop's input conditions): a literal run
//     below 15 with more than 16 bytes of input behind its token and 32 bytes of capacity left,
//     followed by a match below 19 at an offset of 8 or more. So a block may end in a match and an
//     empty literal run. `Block::safe` is that loop state;
//   - a literal length extension must stop 15 bytes before the end of the input and a match length
//     extension 4 bytes before it (both follow from the rules above for a block that is otherwise
//     good; they decide which error a bad one gets, not whether it gets one);
//   - an empty block (capacity 0) is the single byte 0.
// One rule here is stricter than liblz4: offset 0 is refused. liblz4 does not look at it and copies
// whatever its destination held (tests/lz4_corpus.zero_offset is the structural predicate for it).
//
// Codec 5: a page body is one or more units: a big-endian u32 U (uncompressed bytes of the unit), then
// inner blocks -- a big-endian u32 C and a bare block of C bytes -- until the unit has produced exactly
// U bytes. Every inner block is on its own: an offset never reaches below its block's output. This is
// Hadoop's grammar; Arrow's reader knows only units of one inner block, and its second attempt (the
// body as one bare block when the framing does not parse) is not taken.
#pragma once
#include <cstdint>
#include "filter_plan.h"  // DR_HD

namespace dr {
namespace lz4 {

enum Err : int32_t {
  E_OK = 0,
  E_INPUT = 1,     // a length extension, a literal run or an offset runs off the input
  E_OFFSET = 2,    // offset 0, or beyond the block's output so far
  E_OUTPUT = 3,    // more output than the capacity, or a page short of its size
  E_END = 4,       // an end-of-block condition
  E_TRAILING = 5,  // input left behind the last literals
  E_FRAME = 6,     // codec 5: a unit or inner-block header
  E_INTERNAL = 7,
};

enum Framing : uint32_t { F_BARE = 0, F_HADOOP = 1 };

// Bytes [0, n) behind a pointer; -1 past the end.
struct PtrSrc {
  const uint8_t* b;
  uint64_t n;
  DR_HD int operator()(uint64_t pos) const { return pos < n ? int(b[pos]) : -1; }
};

// One bare block: src[ip, iend) into at most `oend` bytes (counted from the block's own output).
struct Block {
  int64_t ip, iend;
  int64_t op, oend;
  uint32_t safe;   // liblz4 has left its first loop
  uint32_t fresh;
};
struct Seq {
  uint64_t lit;    // position of the literals in the source
  uint32_t ll;     // literals
  uint32_t off;    // match offset (0 with ml = 0: none)
  uint32_t ml;
  uint32_t last;   // the block ends here
};

DR_HD inline void begin(Block& b, uint64_t at, uint64_t n_in, uint64_t cap) {
  b.ip = int64_t(at);
  b.iend = int64_t(at + n_in);
  b.op = 0;
  b.oend = int64_t(cap);
  b.safe = cap < 64;
  b.fresh = 1;
}

// Extension bytes of a length: liblz4's read_variable_length against `limit`.
template <class R>
DR_HD inline bool extend(const R& rd, int64_t& ip, int64_t limit, bool initial_check, int64_t& len) {
  if (initial_check && ip >= limit) return false;
  for (;;) {
    const int s = rd(uint64_t(ip));
    if (s < 0) return false;
    ++ip;
    len += s;
    if (ip > limit) return false;
    if (s != 255) return true;
  }
}

// The next sequence of the block. The caller copies q->ll literals from q->lit and then q->ml bytes
// from q->off back; b.op has moved over both.
template <class R>
DR_HD inline int next(const R& rd, Block& b, Seq* q) {
  int64_t ip = b.ip, op = b.op;
  const int64_t iend = b.iend, oend = b.oend;
  q->off = q->ml = q->last = 0;
  if (b.fresh) {
    b.fresh = 0;
    if (oend == 0) {
      if (iend - ip != 1 || rd(uint64_t(ip)) != 0) return E_OUTPUT;
      q->lit = uint64_t(iend);
      q->ll = 0;
      q->last = 1;
      b.ip = iend;
      return E_OK;
    }
    if (iend == ip) return E_INPUT;
  }
  const int token = rd(uint64_t(ip));
  if (token < 0 || ip >= iend) return E_INPUT;
  ++ip;
  int64_t ll = token >> 4, ml = token & 15;
  bool checked_literals = false;  // liblz4's safe_literal_copy
  bool shortcut = false;
  if (!b.safe) {
    if (ll == 15) {
      if (!extend(rd, ip, iend - 15, true, ll)) return E_INPUT;
      if (op + ll > oend - 32 || ip + ll > iend - 32) b.safe = 1, checked_literals = true;
    } else if (ip > iend - 17) {
      b.safe = 1, checked_literals = true;
    }
  } else if (ll != 15 && ip < iend - 16 && op <= oend - 32) {
    shortcut = true;
  } else {
    if (ll == 15 && !extend(rd, ip, iend - 15, true, ll)) return E_INPUT;
    checked_literals = true;
  }
  if (checked_literals && (op + ll > oend - 12 || ip + ll > iend - 8)) {
    if (ip + ll > iend) return E_INPUT;
    if (ip + ll != iend) return op + ll > oend - 12 ? E_END : E_TRAILING;
    if (op + ll > oend) return E_OUTPUT;
    q->lit = uint64_t(ip);
    q->ll = uint32_t(ll);
    q->last = 1;
    b.ip = iend;
    b.op = op + ll;
    return E_OK;
  }
  q->lit = uint64_t(ip);
  q->ll = uint32_t(ll);
  ip += ll;
  op += ll;
  const int lo = rd(uint64_t(ip)), hi = rd(uint64_t(ip) + 1);
  if (lo < 0 || hi < 0 || ip + 2 > iend) return E_INPUT;
  const int64_t off = lo | (hi << 8);
  ip += 2;
  bool checked_match = true;  // liblz4's safe_match_copy
  if (shortcut && ml != 15 && off >= 8 && off <= op) {
    ml += 4;
    checked_match = false;
  } else {
    if (ml == 15 && !extend(rd, ip, iend - 4, false, ml)) return E_INPUT;
    ml += 4;
    if (!b.safe) {
      if (op + ml >= oend - 64) b.safe = 1;
      else checked_match = false;
    }
  }
  if (off == 0 || off > op) return E_OFFSET;
  if (checked_match && op + ml > oend - 5) return op + ml > oend ? E_OUTPUT : E_END;
  q->off = uint32_t(off);
  q->ml = uint32_t(ml);
  b.ip = ip;
  b.op = op + ml;
  return E_OK;
}

// ---- codec 5: Hadoop's units -----------------------------------------------------------------------
template <class R>
DR_HD inline uint32_t be32(const R& rd, uint64_t pos) {
  return uint32_t(rd(pos)) << 24 | uint32_t(rd(pos + 1)) << 16 | uint32_t(rd(pos + 2)) << 8 | uint32_t(rd(pos + 3));
}
// A unit's U at `pos` (advanced to the first inner block's header): at least the two words, and
// 0 < U <= out_left.
template <class R>
DR_HD inline int unit_header(const R& rd, uint64_t& pos, uint64_t n_in, uint64_t out_left, uint32_t* U) {
  if (pos > n_in || n_in - pos < 8) return E_FRAME;
  *U = be32(rd, pos);
  if (*U == 0 || *U > out_left) return E_FRAME;
  pos += 4;
  return E_OK;
}
// An inner block's C at `pos` (advanced to the block): C bytes must follow.
template <class R>
DR_HD inline int inner_header(const R& rd, uint64_t& pos, uint64_t n_in, uint32_t* C) {
  if (pos > n_in || n_in - pos < 4) return E_FRAME;
  *C = be32(rd, pos);
  pos += 4;
  if (*C > n_in - pos) return E_FRAME;
  return E_OK;
}

}  // namespace lz4
}  // namespace dr
