// K2: GZIP pages (Parquet CompressionCodec 2) as the host inflater (inflate_host.cpp) and the device
// kernel (k_inflate.hip) both read them: the gzip member framing of RFC 1952 and the DEFLATE format of
// RFC 1951 -- the LSB-first bit reader, the block header, the dynamic header, canonical code
// construction and the one step that yields the next symbol. Plain C++, no HIP type and no allocation:
// g++ compiles it, and hipcc compiles it as device code. A byte stream takes the same decisions on
// both sides because both walk these functions; what a stream is accepted for follows zlib's inflate:
//   - block type 3, a stored block whose NLEN is not ~LEN, HLIT > 286 (nlen > 286) or HDIST > 30;
//   - a code-length code that is over-subscribed or incomplete; a repeat (16) with no previous
//     length, or a repeat that runs past HLIT + HDIST lengths;
//   - a dynamic block whose symbol 256 has length 0;
//   - a literal/length or distance code that is over-subscribed, or incomplete unless it is a single
//     code of one bit (zlib accepts that for either alphabet; the unused bit pattern is an error
//     when it is met);
//   - the length symbols 286 / 287 and the distance symbols 30 / 31;
//   - input that ends inside a block (no zero fill)
// are errors. What the caller checks with its own positions: a distance beyond the bytes the member
// has produced, output past the page, ISIZE. The member's CRC32 is read over and not verified.
#pragma once
#include <cstdint>
#include "filter_plan.h"  // DR_HD

namespace dr {
namespace dfl {

enum Err : int32_t {
  E_OK = 0,
  E_INPUT = 1,      // the input ends inside a header, a block or the trailer
  E_MAGIC = 2,      // not a gzip member: magic, CM or a reserved FLG bit
  E_BTYPE = 3,      // block type 3
  E_STORED = 4,     // LEN / NLEN
  E_COUNTS = 5,     // HLIT or HDIST out of range
  E_CLEN = 6,       // code-length code not complete, or a bad repeat
  E_NO_EOB = 7,     // symbol 256 has no code
  E_LITCODE = 8,    // literal/length code lengths refused
  E_DISTCODE = 9,   // distance code lengths refused
  E_SYMBOL = 10,    // a bit pattern without a symbol, or symbol 286 / 287 / distance 30 / 31
  E_DISTANCE = 11,  // a distance beyond the member's output so far
  E_OUTPUT = 12,    // more output than the page holds, or less
  E_ISIZE = 13,
  E_INTERNAL = 14,
};

// Bytes [0, n) behind a pointer; -1 past the end.
struct PtrSrc {
  const uint8_t* b;
  uint64_t n;
  DR_HD int operator()(uint64_t pos) const { return pos < n ? int(b[pos]) : -1; }
};

// ---- gzip member framing (RFC 1952) ------------------------------------------------------------
// The member header at `pos` (advanced to the first byte of the DEFLATE stream).
template <class R>
DR_HD inline int gz_header(const R& rd, uint64_t& pos) {
  int h[10];
  for (int i = 0; i < 10; ++i) {
    h[i] = rd(pos + uint64_t(i));
    if (h[i] < 0) return E_INPUT;
  }
  if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || (h[3] & 0xe0)) return E_MAGIC;
  const int flg = h[3];
  pos += 10;
  if (flg & 4) {  // FEXTRA: XLEN, then XLEN bytes
    const int lo = rd(pos), hi = rd(pos + 1);
    if (lo < 0 || hi < 0) return E_INPUT;
    pos += 2 + uint64_t(lo | (hi << 8));
  }
  for (int f = 8; f <= 16; f <<= 1) {  // FNAME, FCOMMENT: zero-terminated
    if (!(flg & f)) continue;
    for (;;) {
      const int b = rd(pos);
      if (b < 0) return E_INPUT;
      ++pos;
      if (b == 0) break;
    }
  }
  if (flg & 2) pos += 2;  // FHCRC (not verified)
  if (rd(pos) < 0) return E_INPUT;  // the header is followed by at least one byte of the stream
  return E_OK;
}
constexpr uint32_t GZ_TRAILER = 8;  // CRC32, ISIZE
// The trailer at `pos` (advanced past it): ISIZE must be the member's output length mod 2^32.
template <class R>
DR_HD inline int gz_trailer(const R& rd, uint64_t& pos, uint64_t produced) {
  uint32_t isize = 0;
  for (int i = 0; i < 8; ++i) {
    const int b = rd(pos + uint64_t(i));
    if (b < 0) return E_INPUT;
    if (i >= 4) isize |= uint32_t(b) << (8 * (i - 4));
  }
  pos += 8;
  return isize == uint32_t(produced) ? E_OK : E_ISIZE;
}

// ---- bit reader ------------------------------------------------------------------------------
// LSB-first over a byte source. `pos` is the next byte to load, `cnt` the bits held in `buf`; bits
// past the end of the source are never invented: need(k) fails instead.
template <class R>
struct Bits {
  R rd;
  uint64_t pos;
  uint64_t buf;
  uint32_t cnt;
  DR_HD Bits(const R& r, uint64_t bitpos) : rd(r), pos(bitpos >> 3), buf(0), cnt(0) {
    fill();
    const uint32_t skip = uint32_t(bitpos & 7);
    if (cnt >= skip) {
      buf >>= skip;
      cnt -= skip;
    }
  }
  DR_HD void fill() {
    while (cnt <= 56) {
      const int b = rd(pos);
      if (b < 0) return;
      buf |= uint64_t(b) << cnt;
      cnt += 8;
      ++pos;
    }
  }
  DR_HD bool need(uint32_t k) {  // k <= 32
    if (cnt < k) fill();
    return cnt >= k;
  }
  DR_HD uint32_t peek(uint32_t k) const { return uint32_t(buf) & ((uint32_t(1) << k) - 1); }
  DR_HD void drop(uint32_t k) {
    buf >>= k;
    cnt -= k;
  }
  DR_HD bool take(uint32_t k, uint32_t* v) {  // k <= 16
    if (!need(k)) return false;
    *v = peek(k);
    drop(k);
    return true;
  }
  DR_HD uint64_t bitpos() const { return pos * 8 - cnt; }
  DR_HD void align() { drop(cnt & 7); }
  DR_HD void seek(uint64_t byte) {
    pos = byte;
    buf = 0;
    cnt = 0;
  }
};

// ---- codes ------------------------------------------------------------------------------------
constexpr int MAX_BITS = 15;
constexpr int LIT_SYMS = 288, DIST_SYMS = 32, MAX_LENS = LIT_SYMS + DIST_SYMS;
constexpr int LIT_FAST = 10, DIST_FAST = 8;  // bits of the direct lookup tables

// A canonical code: the symbols sorted by (length, value), how many have each length, where each
// length starts in `sym` and its first code; `fast` maps the next `fbits` input bits to
// (symbol << 4 | length) for the codes no longer than that, 0 for the others.
struct Code {
  uint16_t count[MAX_BITS + 1];
  uint16_t offs[MAX_BITS + 2];
  uint16_t first[MAX_BITS + 1];
  int32_t status;
};
struct Tables {
  uint16_t lit_fast[1 << LIT_FAST];
  uint16_t dist_fast[1 << DIST_FAST];
  uint16_t lit_sym[LIT_SYMS];
  uint16_t dist_sym[DIST_SYMS];
  Code lit, dist;
  uint8_t lens[MAX_LENS];  // the block's code lengths: nlen literal/length, then ndist distance
};

struct NoSync {
  DR_HD void operator()() const {}
};

DR_HD inline uint32_t bit_reverse(uint32_t v, int n) {
  uint32_t r = 0;
  for (int i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1 - i);
  return r;
}

// Builds the code of lens[0, n). `lane` of `nl` workers take part (the host: 0 of 1), `sync` is a
// barrier among them that also orders their writes. The result is c.status: E_OK, or `refused`.
// zlib's rules: over-subscribed is refused; incomplete is refused unless the code is one symbol of
// one bit, or `codes` (the code-length code) where every incomplete set is refused; no symbol at all
// is accepted (every pattern is then an error when met).
template <class Sync>
DR_HD inline void build_code(const uint8_t* lens, int n, Code& c, uint16_t* sym, uint16_t* fast, int fbits, bool codes,
                             int refused, int lane, int nl, Sync sync) {
  for (int L = lane; L <= MAX_BITS; L += nl) {
    uint16_t k = 0;
    for (int s = 0; s < n; ++s) k += lens[s] == L;
    c.count[L] = k;
  }
  if (fast)
    for (int i = lane; i < (1 << fbits); i += nl) fast[i] = 0;
  sync();
  if (lane == 0) {
    int left = 1, max = 0;
    uint32_t off = 0, code = 0;
    int status = E_OK;
    for (int L = 1; L <= MAX_BITS; ++L) {
      left <<= 1;
      left -= int(c.count[L]);
      if (left < 0) {
        status = refused;
        break;
      }
      if (c.count[L]) max = L;
      c.offs[L] = uint16_t(off);
      c.first[L] = uint16_t(code);
      off += c.count[L];
      code = (code + c.count[L]) << 1;
    }
    c.offs[MAX_BITS + 1] = uint16_t(off);
    if (status == E_OK && left > 0 && max != 0 && (codes || max != 1)) status = refused;
    c.status = status;
  }
  sync();
  if (c.status != E_OK) return;
  for (int L = 1 + lane; L <= MAX_BITS; L += nl) {
    uint32_t at = c.offs[L];
    if (!c.count[L]) continue;
    for (int s = 0; s < n; ++s)
      if (lens[s] == L) sym[at++] = uint16_t(s);
  }
  sync();
  if (fast) {
    const int total = c.offs[MAX_BITS + 1];
    for (int i = lane; i < total; i += nl) {
      int L = 1;
      while (L < MAX_BITS && i >= int(c.offs[L + 1])) ++L;
      if (L > fbits) continue;
      const uint32_t code = uint32_t(c.first[L]) + uint32_t(i - int(c.offs[L]));
      const uint16_t e = uint16_t((uint32_t(sym[i]) << 4) | uint32_t(L));
      for (uint32_t k = bit_reverse(code, L); k < (uint32_t(1) << fbits); k += uint32_t(1) << L) fast[k] = e;
    }
  }
  sync();
}

// The next symbol of a code, or -E_INPUT / -E_SYMBOL.
template <class B>
DR_HD inline int decode_sym(B& br, const Code& c, const uint16_t* sym, const uint16_t* fast, int fbits) {
  br.fill();
  if (fast) {
    const uint32_t e = fast[br.peek(uint32_t(fbits))];
    if (e) {
      const uint32_t L = e & 15;
      if (br.cnt < L) return -E_INPUT;
      br.drop(L);
      return int(e >> 4);
    }
  }
  uint32_t code = 0;
  for (int L = 1; L <= MAX_BITS; ++L) {
    if (br.cnt < uint32_t(L)) return -E_INPUT;
    code |= uint32_t(br.buf >> (L - 1)) & 1u;
    const uint32_t cnt = c.count[L], first = c.first[L];
    if (code >= first && code - first < cnt) {
      br.drop(uint32_t(L));
      return int(sym[c.offs[L] + (code - first)]);
    }
    code <<= 1;
  }
  return -E_SYMBOL;
}

// ---- blocks -------------------------------------------------------------------------------------
enum BlockKind : int32_t { BK_STORED = 0, BK_CODED = 1 };
struct Block {
  int32_t kind;
  int32_t final;
  uint32_t stored_len;  // BK_STORED: the bytes follow at br.bitpos() / 8
  int32_t nlen, ndist;  // BK_CODED: T.lens holds the lengths; build_codes() comes next
};
// the most input a block header takes: 3 + 14 bits, 19 * 3 bits, 320 lengths of at most 7 + 7 bits
constexpr uint32_t BLOCK_HEADER_MAX_BYTES = (17 + 57 + MAX_LENS * 14 + 7) / 8 + 8;

DR_HD inline uint8_t clen_order(int i) {  // where the i-th length of the code-length code belongs
  return uint8_t("\x10\x11\x12\x00\x08\x07\x09\x06\x0a\x05\x0b\x04\x0c\x03\x0d\x02\x0e\x01\x0f"[i]);
}

// The block header at the reader: BFINAL, BTYPE, and what the type brings with it (a stored block's
// LEN / NLEN, after which the reader stands on a byte boundary; the fixed code's lengths; the dynamic
// header's lengths). One worker calls it.
template <class B>
DR_HD inline int block_header(B& br, Tables& T, Block* b) {
  uint32_t v;
  if (!br.take(3, &v)) return E_INPUT;
  b->final = int32_t(v & 1);
  const uint32_t type = v >> 1;
  if (type == 3) return E_BTYPE;
  if (type == 0) {
    br.align();
    uint32_t len, nlen;
    if (!br.take(16, &len) || !br.take(16, &nlen)) return E_INPUT;
    if ((len ^ 0xffffu) != nlen) return E_STORED;
    b->kind = BK_STORED;
    b->stored_len = len;
    return E_OK;
  }
  b->kind = BK_CODED;
  if (type == 1) {
    for (int s = 0; s < LIT_SYMS; ++s) T.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
    for (int s = 0; s < DIST_SYMS; ++s) T.lens[LIT_SYMS + s] = 5;
    b->nlen = LIT_SYMS;
    b->ndist = DIST_SYMS;
    return E_OK;
  }
  uint32_t hlit, hdist, hclen;
  if (!br.take(5, &hlit) || !br.take(5, &hdist) || !br.take(4, &hclen)) return E_INPUT;
  const int nlen = int(hlit) + 257, ndist = int(hdist) + 1, ncode = int(hclen) + 4;
  if (nlen > 286 || ndist > 30) return E_COUNTS;
  // the code-length code is built in the distance code's slots, which are not in use yet
  uint8_t cl[19];
  for (int i = 0; i < 19; ++i) cl[i] = 0;
  for (int i = 0; i < ncode; ++i) {
    if (!br.take(3, &v)) return E_INPUT;
    cl[clen_order(i)] = uint8_t(v);
  }
  build_code(cl, 19, T.dist, T.dist_sym, static_cast<uint16_t*>(nullptr), 0, true, E_CLEN, 0, 1, NoSync());
  if (T.dist.status != E_OK) return E_CLEN;
  int have = 0;
  while (have < nlen + ndist) {
    const int s = decode_sym(br, T.dist, T.dist_sym, static_cast<const uint16_t*>(nullptr), 0);
    // zlib reads a pattern without a symbol (a code-length code with no symbol at all) as length 0
    // of one bit; such a block has no end-of-block code and is refused below either way
    if (s == -E_SYMBOL) return E_NO_EOB;
    if (s < 0) return -s;
    if (s < 16) {
      T.lens[have++] = uint8_t(s);
      continue;
    }
    uint32_t rep, val = 0;
    if (s == 16) {
      if (have == 0) return E_CLEN;
      val = T.lens[have - 1];
      if (!br.take(2, &rep)) return E_INPUT;
      rep += 3;
    } else if (s == 17) {
      if (!br.take(3, &rep)) return E_INPUT;
      rep += 3;
    } else {
      if (!br.take(7, &rep)) return E_INPUT;
      rep += 11;
    }
    if (have + int(rep) > nlen + ndist) return E_CLEN;
    while (rep--) T.lens[have++] = uint8_t(val);
  }
  if (T.lens[256] == 0) return E_NO_EOB;
  b->nlen = nlen;
  b->ndist = ndist;
  return E_OK;
}

// The two codes of a BK_CODED block from T.lens. Every worker calls it; E_OK or the error, the same
// for all of them.
template <class Sync>
DR_HD inline int build_codes(Tables& T, const Block& b, int lane, int nl, Sync sync) {
  build_code(T.lens, b.nlen, T.lit, T.lit_sym, T.lit_fast, LIT_FAST, false, E_LITCODE, lane, nl, sync);
  build_code(T.lens + b.nlen, b.ndist, T.dist, T.dist_sym, T.dist_fast, DIST_FAST, false, E_DISTCODE, lane, nl, sync);
  return T.lit.status != E_OK ? T.lit.status : T.dist.status;
}

DR_HD inline uint32_t len_base(int i) {  // length symbol 257 + i
  return i < 8 ? uint32_t(3 + i) : i == 28 ? 258u : ((uint32_t(4 + (i & 3))) << ((i >> 2) - 1)) + 3;
}
DR_HD inline uint32_t len_extra(int i) { return i < 8 || i == 28 ? 0u : uint32_t((i >> 2) - 1); }
DR_HD inline uint32_t dist_base(int i) {  // distance symbol i
  return i < 4 ? uint32_t(1 + i) : ((uint32_t(2 + (i & 1))) << ((i >> 1) - 1)) + 1;
}
DR_HD inline uint32_t dist_extra(int i) { return i < 4 ? 0u : uint32_t((i >> 1) - 1); }

enum SymKind : int32_t { SY_LITERAL = 0, SY_MATCH = 1, SY_END = 2 };
struct Symbol {
  int32_t kind;
  uint32_t value;  // SY_LITERAL: the byte; SY_MATCH: the length (3..258)
  uint32_t dist;   // SY_MATCH: 1..32768
};
// the most input one symbol takes: 15 + 5 + 15 + 13 bits
constexpr uint32_t SYMBOL_MAX_BYTES = 6;

// The next symbol of a coded block. Consumes at least one bit, or fails.
template <class B>
DR_HD inline int next_symbol(B& br, const Tables& T, Symbol* out) {
  const int s = decode_sym(br, T.lit, T.lit_sym, T.lit_fast, LIT_FAST);
  if (s < 0) return -s;
  if (s < 256) {
    out->kind = SY_LITERAL;
    out->value = uint32_t(s);
    return E_OK;
  }
  if (s == 256) {
    out->kind = SY_END;
    return E_OK;
  }
  if (s >= 286) return E_SYMBOL;
  uint32_t x = 0;
  const uint32_t le = len_extra(s - 257);
  if (le && !br.take(le, &x)) return E_INPUT;
  out->kind = SY_MATCH;
  out->value = len_base(s - 257) + x;
  const int d = decode_sym(br, T.dist, T.dist_sym, T.dist_fast, DIST_FAST);
  if (d < 0) return -d;
  if (d >= 30) return E_SYMBOL;
  x = 0;
  const uint32_t de = dist_extra(d);
  if (de && !br.take(de, &x)) return E_INPUT;
  out->dist = dist_base(d) + x;
  return E_OK;
}

}  // namespace dfl
}  // namespace dr
