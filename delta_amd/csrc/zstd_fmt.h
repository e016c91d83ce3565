// K2: ZSTD pages (Parquet CompressionCodec 6) as the host decoder (zstd_host.h) and the device kernel
// (k_zstd.hip) both read them: the frame, block, literals and sequences layers of RFC 8878, the FSE and
// Huffman table builders, the backward bit reader, the step that yields the next sequence, and XXH64
// for the content checksum. Plain C++, no HIP type and no allocation: g++ compiles it, and hipcc
// compiles it as device code. A byte stream takes the same decisions on both sides because both walk
// these functions. What a stream is accepted for follows libzstd 1.5.7's one-shot ZSTD_decompress,
// which is what the acceptance tests compare against; where it differs from the RFC it decides:
//   - a Raw or RLE block may be larger than Block_Maximum_Size (only a Compressed block's Block_Size
//     and a literals section's regenerated size are held to it);
//   - Huffman codes may be 12 bits long (the RFC says 11);
//   - an offset may exceed the window as long as it stays inside the frame's own output; it never
//     reaches into an earlier frame of the same page;
//   - a repeat offset that comes out as 0 is an error; a sequence bitstream, a Huffman stream and the
//     sequences section of a block without sequences must be consumed exactly;
//   - four Huffman streams of eight bytes or more each are decoded as libzstd's loop decodes them,
//     which does not look for a stream's end (huf_loose4);
//   - the reserved bits of the frame descriptor (bit 3) and of the sequence modes byte must be 0; the
//     unused descriptor bit 4 is ignored; a Dictionary_ID field that holds 0 is accepted.
// Builders take `lane` of `nl` workers and a barrier functor `sync` that also orders their writes (the
// host: 0 of 1 and NoSync). Everything else is called by one worker.
#pragma once
#include <cstdint>
#include "filter_plan.h"  // DR_HD

// the bit readers and the sequence step sit in the kernel's inner loops: their state must stay in registers
#define DR_ZST_INLINE DR_HD inline __attribute__((always_inline))

namespace dr {
namespace zst {

enum Err : int32_t {
  E_OK = 0,
  E_INPUT = 1,      // the input ends inside a header, a block or a section
  E_MAGIC = 2,      // neither a zstd frame nor a skippable one
  E_FRAME = 3,      // reserved descriptor bit, window too large
  E_DICT = 4,       // a non-zero Dictionary_ID
  E_BTYPE = 5,      // block type 3
  E_BSIZE = 6,      // a compressed block over Block_Maximum_Size
  E_LITERALS = 7,   // literals section header or sizes
  E_HUF = 8,        // Huffman tree description refused, or a stream not consumed exactly
  E_NOTREE = 9,     // Treeless literals without a previous tree
  E_SEQHDR = 10,    // sequence count / modes byte
  E_FSE = 11,       // normalised counts refused, accuracy log over the limit, RLE symbol out of range
  E_NOTABLE = 12,   // Repeat mode without a previous table
  E_SEQBITS = 13,   // the sequence bitstream: empty, last byte 0, or not consumed exactly
  E_OFFSET = 14,    // an offset beyond the frame's output so far, or a zero repeat offset
  E_LITLEN = 15,    // a literal length beyond the block's literals
  E_OUTPUT = 16,    // more output than the page holds, or less
  E_CONTENT = 17,   // Frame_Content_Size differs from the frame's output
  E_CHECKSUM = 18,
  E_INTERNAL = 19,
};

struct NoSync {
  DR_HD void operator()() const {}
};
// Bytes [0, n) behind a pointer; -1 past the end.
struct PtrSrc {
  const uint8_t* b;
  uint64_t n;
  DR_HD int operator()(uint64_t pos) const { return pos < n ? int(b[pos]) : -1; }
};

DR_HD inline uint32_t highbit(uint32_t v) {  // v != 0
  uint32_t r = 0;
  while (v >>= 1) ++r;
  return r;
}
// little-endian value of k <= 8 bytes at pos; false past `end`
template <class R>
DR_HD inline bool le(const R& rd, uint64_t pos, uint64_t end, int k, uint64_t* v) {
  if (end < pos || end - pos < uint64_t(k)) return false;
  uint64_t x = 0;
  for (int i = 0; i < k; ++i) x |= uint64_t(uint32_t(rd(pos + uint64_t(i))) & 0xffu) << (8 * i);
  *v = x;
  return true;
}

// ---- frames -------------------------------------------------------------------------------------
constexpr uint32_t MAGIC = 0xFD2FB528u, SKIP_MAGIC = 0x184D2A50u;
constexpr uint32_t BLOCK_MAX = 128 * 1024;
constexpr uint32_t WINDOW_LOG_MAX = 31;

struct Frame {
  int32_t skippable;      // 1: nothing but `pos` (past the frame) is set
  int32_t checksum;       // a 4-byte checksum follows the last block
  int32_t has_size;
  uint64_t content_size;  // if has_size
  uint32_t block_max;     // min(window, 128 KiB)
};
// The frame at `pos` of rd[0, n): pos moves to its first block header (past it, if skippable).
template <class R>
DR_HD inline int frame_header(const R& rd, uint64_t n, uint64_t& pos, Frame* f) {
  uint64_t v;
  // libzstd looks at a frame only if 5 bytes are left
  if (n - pos < 5 || !le(rd, pos, n, 4, &v)) return E_INPUT;
  if ((uint32_t(v) & 0xfffffff0u) == SKIP_MAGIC) {
    uint64_t size;
    if (!le(rd, pos + 4, n, 4, &size)) return E_INPUT;
    if (size > n - pos - 8) return E_INPUT;
    pos += 8 + size;
    f->skippable = 1;
    return E_OK;
  }
  if (uint32_t(v) != MAGIC) return E_MAGIC;
  f->skippable = 0;
  const int d = rd(pos + 4);
  uint64_t at = pos + 5;
  if (d & 0x08) return E_FRAME;
  const int single = (d >> 5) & 1, fcs_code = d >> 6, did_code = d & 3;
  f->checksum = (d >> 2) & 1;
  uint64_t window = 0;
  if (!single) {
    const int w = rd(at++);
    if (w < 0) return E_INPUT;
    const uint32_t wlog = uint32_t(w >> 3) + 10;
    if (wlog > WINDOW_LOG_MAX) return E_FRAME;
    window = uint64_t(1) << wlog;
    window += (window >> 3) * uint64_t(w & 7);
  }
  const int did_bytes = did_code == 3 ? 4 : did_code;
  if (!le(rd, at, n, did_bytes, &v)) return E_INPUT;
  if (did_bytes && v != 0) return E_DICT;
  at += uint64_t(did_bytes);
  const int fcs_bytes = fcs_code == 0 ? single : 1 << fcs_code;
  if (!le(rd, at, n, fcs_bytes, &v)) return E_INPUT;
  at += uint64_t(fcs_bytes);
  f->has_size = fcs_bytes != 0;
  f->content_size = fcs_bytes == 2 ? v + 256 : v;
  if (single) window = f->content_size;
  f->block_max = window < BLOCK_MAX ? uint32_t(window) : BLOCK_MAX;
  pos = at;
  return E_OK;
}

// ---- blocks -------------------------------------------------------------------------------------
enum BlockType : int32_t { BT_RAW = 0, BT_RLE = 1, BT_COMPRESSED = 2 };
struct Block {
  int32_t type, last;
  uint32_t size;   // Block_Size: the bytes a Raw or Compressed block takes; the output of an RLE block
};
// The block header at `pos` (moved past it). What follows is inside the input: `size` bytes, 1 for RLE.
template <class R>
DR_HD inline int block_header(const R& rd, uint64_t n, uint64_t& pos, uint32_t block_max, Block* b) {
  uint64_t v;
  if (!le(rd, pos, n, 3, &v)) return E_INPUT;
  pos += 3;
  b->last = int32_t(v & 1);
  b->type = int32_t((v >> 1) & 3);
  b->size = uint32_t(v >> 3);
  if (b->type == 3) return E_BTYPE;
  if ((b->type == BT_RLE ? 1u : b->size) > n - pos) return E_INPUT;
  if (b->type == BT_COMPRESSED && b->size > block_max) return E_BSIZE;
  return E_OK;
}

// ---- the backward bit stream ----------------------------------------------------------------------
// Bits of rd[start, end) read from the last byte's final-bit marker down to bit 0 of the first byte.
// `left` counts the bits not yet read and goes negative when more are asked for than the stream
// holds: such bits read as 0, and the caller's check that left == 0 at the end refuses the stream.
template <class R>
struct BackBits {
  R rd;
  uint64_t start;
  int64_t left;
  int64_t span;     // 8 * the stream's bytes
  uint64_t win;     // 64 bits of the stream from bit win_lo up (0 below the stream's first bit)
  int64_t win_lo;   // a multiple of 8; INT64_MAX: nothing loaded
  DR_HD BackBits() : rd(), start(0), left(0), span(0), win(0), win_lo(INT64_MAX) {}
  DR_HD BackBits(const R& r) : rd(r), start(0), left(0), span(0), win(0), win_lo(INT64_MAX) {}
  // `loose`: a last byte of 0 carries no marker and counts as eight bits (see huf_loose4)
  DR_ZST_INLINE bool init(uint64_t s, uint64_t e, bool loose = false) {
    if (e <= s) return false;
    const int lastb = rd(e - 1);
    if (lastb < 0 || (lastb == 0 && !loose)) return false;
    start = s;
    span = int64_t(8 * (e - s));
    left = int64_t(8 * (e - 1 - s)) + (lastb ? int64_t(highbit(uint32_t(lastb))) : 8);
    win_lo = INT64_MAX;
    return true;
  }
  DR_ZST_INLINE void load(int64_t top) {  // a window whose upper end covers bit top - 1
    win_lo = ((top + 7) & ~int64_t(7)) - 64;
    win = 0;
    for (int i = 0; i < 8; ++i) {
      const int64_t bit = win_lo + 8 * i;
      if (bit >= 0 && bit < span)  // never outside the stream
        win |= uint64_t(uint32_t(rd(start + uint64_t(bit >> 3))) & 0xffu) << (8 * i);
    }
  }
  // the k <= 32 bits below `left`, without taking them
  DR_ZST_INLINE uint32_t peek(uint32_t k) {
    if (k == 0) return 0;
    int64_t lo = left - int64_t(k);
    uint32_t shift = 0;
    if (lo < 0) {
      if (left <= 0) return 0;
      shift = uint32_t(-lo);
      k -= shift;
      lo = 0;
    }
    if (lo < win_lo || lo + int64_t(k) > win_lo + 64) load(lo + int64_t(k));
    const uint64_t v = (win >> uint32_t(lo - win_lo)) & ((uint64_t(1) << k) - 1);
    return uint32_t(v) << shift;
  }
  DR_ZST_INLINE uint32_t take(uint32_t k) {
    const uint32_t v = peek(k);
    left -= int64_t(k);
    return v;
  }
};

// ---- FSE ----------------------------------------------------------------------------------------
constexpr int LL_MAX = 35, OF_MAX = 31, ML_MAX = 52;
constexpr int LL_LOG = 9, OF_LOG = 8, ML_LOG = 9, HUFW_LOG = 6;
constexpr int NORM_SYMS = 256;  // the Huffman weight table's counts may name this many symbols

struct FseEntry {
  uint16_t base;   // of the next state
  uint8_t sym;
  uint8_t nbits;   // read and added to base
};

// The normalised counts at rd[pos, end) (FSE_readNCount): norm[0, *nsym), the accuracy log, and the
// bytes taken. `maxsym` is the alphabet's largest symbol.
template <class R>
DR_HD inline int read_ncount(const R& rd, uint64_t pos, uint64_t end, int maxsym, int16_t* norm, int* tlog, int* nsym,
                             uint32_t* used) {
  const uint64_t avail_bits = 8 * (end - pos);
  uint64_t bp = 0;
  auto peek = [&](uint32_t k) {  // LSB first, zeros past the end
    uint64_t v = 0;
    const uint64_t byte = pos + (bp >> 3);
    for (int i = 0; i < 5; ++i)
      if (byte + uint64_t(i) < end) v |= uint64_t(uint32_t(rd(byte + uint64_t(i))) & 0xffu) << (8 * i);
    return uint32_t((v >> (bp & 7)) & ((uint64_t(1) << k) - 1));
  };
  if (end <= pos) return E_INPUT;
  int nb = int(peek(4)) + 5;
  bp = 4;
  if (nb > 15) return E_FSE;
  *tlog = nb;
  int remaining = (1 << nb) + 1, threshold = 1 << nb, charnum = 0;
  const int maxsv1 = maxsym + 1;
  bool previous0 = false;
  ++nb;
  for (int s = 0; s < maxsv1; ++s) norm[s] = 0;
  for (;;) {
    if (bp > avail_bits) return E_FSE;
    if (previous0) {
      for (;;) {
        const uint32_t r = peek(2);
        bp += 2;
        charnum += int(r);
        if (r != 3 || charnum >= maxsv1 || bp > avail_bits) break;
      }
      if (charnum >= maxsv1) break;
    }
    const int max = (2 * threshold - 1) - remaining;
    const int v = int(peek(uint32_t(nb)));
    int count;
    if ((v & (threshold - 1)) < max) {
      count = v & (threshold - 1);
      bp += uint64_t(nb - 1);
    } else {
      count = v & (2 * threshold - 1);
      if (count >= threshold) count -= max;
      bp += uint64_t(nb);
    }
    --count;
    remaining -= count >= 0 ? count : -count;
    norm[charnum++] = int16_t(count);
    previous0 = count == 0;
    if (remaining < threshold) {
      if (remaining <= 1) break;
      nb = int(highbit(uint32_t(remaining))) + 1;
      threshold = 1 << (nb - 1);
    }
    if (charnum >= maxsv1) break;
  }
  if (remaining != 1 || charnum > maxsv1 || bp > avail_bits) return E_FSE;
  *nsym = charnum;
  *used = uint32_t((bp + 7) >> 3);
  return E_OK;
}

// The decoding table of norm[0, nsym) at accuracy log `tlog` (the counts sum to 1 << tlog, -1 counting
// as one). `next` is scratch for nsym words. Symbols are placed by worker 0; the states of a symbol
// are numbered by the worker that owns it.
template <class Sync>
DR_HD inline void build_fse(const int16_t* norm, int nsym, int tlog, FseEntry* tab, uint16_t* next, int lane, int nl,
                            Sync sync) {
  const uint32_t size = uint32_t(1) << tlog, mask = size - 1;
  if (lane == 0) {
    uint32_t high = size - 1;
    for (int s = 0; s < nsym; ++s) {
      if (norm[s] == -1) {
        tab[high--].sym = uint8_t(s);
        next[s] = 1;
      } else {
        next[s] = uint16_t(norm[s]);
      }
    }
    const uint32_t step = (size >> 1) + (size >> 3) + 3;
    uint32_t p = 0;
    for (int s = 0; s < nsym; ++s) {
      for (int i = 0; i < int(norm[s]); ++i) {
        tab[p].sym = uint8_t(s);
        p = (p + step) & mask;
        while (p > high) p = (p + step) & mask;
      }
    }
  }
  sync();
  for (uint32_t u = 0; u < size; ++u) {
    const uint32_t s = tab[u].sym;
    if (int(s % uint32_t(nl)) != lane) continue;
    const uint32_t ns = next[s]++;
    const uint32_t nb = uint32_t(tlog) - highbit(ns);
    tab[u].nbits = uint8_t(nb);
    tab[u].base = uint16_t((ns << nb) - size);
  }
  sync();
}

// ---- Huffman --------------------------------------------------------------------------------------
constexpr int HUF_LOG_MAX = 12;
struct HufScratch {
  int16_t norm[NORM_SYMS];
  uint16_t next[NORM_SYMS];   // build_fse's scratch; then where each symbol's entries start
  FseEntry wtab[1 << HUFW_LOG];
  uint8_t weights[256];
};

// The Huffman tree description at rd[pos, end) (HUF_readStats): the weights of nsym symbols, the
// implied last one included, the table log and the bytes taken. One worker.
template <class R>
DR_HD inline int huf_read_weights(const R& rd, uint64_t pos, uint64_t end, HufScratch& H, int* nsym, int* tlog,
                                  uint32_t* used) {
  if (end <= pos) return E_INPUT;
  const uint32_t hb = uint32_t(rd(pos));
  uint32_t isize, n = 0;
  uint8_t* w = H.weights;
  if (hb >= 128) {
    n = hb - 127;
    isize = (n + 1) / 2;
    if (uint64_t(isize) + 1 > end - pos) return E_INPUT;
    for (uint32_t i = 0; i < n; i += 2) {
      const uint32_t b = uint32_t(rd(pos + 1 + i / 2));
      w[i] = uint8_t(b >> 4);
      w[i + 1] = uint8_t(b & 15);  // i + 1 <= 128
    }
  } else {
    isize = hb;
    if (uint64_t(isize) + 1 > end - pos) return E_INPUT;
    const uint64_t fend = pos + 1 + isize;
    int wl, ws;
    uint32_t hdr;
    if (const int e = read_ncount(rd, pos + 1, fend, 255, H.norm, &wl, &ws, &hdr)) return e == E_INPUT ? E_HUF : e;
    if (wl > HUFW_LOG) return E_FSE;
    build_fse(H.norm, ws, wl, H.wtab, H.next, 0, 1, NoSync());
    BackBits<R> br(rd);
    if (!br.init(pos + 1 + hdr, fend)) return E_HUF;
    uint32_t s1 = br.take(uint32_t(wl)), s2 = br.take(uint32_t(wl));
    for (;;) {  // two states take turns; the stream ends by running dry (FSE_decompress_usingDTable)
      if (n > 253) return E_HUF;
      w[n++] = H.wtab[s1].sym;
      s1 = H.wtab[s1].base + br.take(H.wtab[s1].nbits);
      if (br.left < 0) {
        w[n++] = H.wtab[s2].sym;
        break;
      }
      if (n > 253) return E_HUF;
      w[n++] = H.wtab[s2].sym;
      s2 = H.wtab[s2].base + br.take(H.wtab[s2].nbits);
      if (br.left < 0) {
        w[n++] = H.wtab[s1].sym;
        break;
      }
    }
  }
  uint32_t total = 0, rank1 = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (w[i] > HUF_LOG_MAX) return E_HUF;
    total += (uint32_t(1) << w[i]) >> 1;
    rank1 += w[i] == 1;
  }
  if (total == 0) return E_HUF;
  const uint32_t tl = highbit(total) + 1;
  if (tl > uint32_t(HUF_LOG_MAX)) return E_HUF;
  const uint32_t rest = (uint32_t(1) << tl) - total;
  if ((uint32_t(1) << highbit(rest)) != rest) return E_HUF;
  w[n] = uint8_t(highbit(rest) + 1);
  rank1 += w[n] == 1;
  if (rank1 < 2 || (rank1 & 1)) return E_HUF;
  *nsym = int(n) + 1;
  *tlog = int(tl);
  *used = isize + 1;
  return E_OK;
}

// The lookup table of a tree: tab[the next tlog bits] = symbol << 4 | code length. Codes are numbered
// from the lightest weight up, each weight in symbol order. `start` is scratch for nsym words.
template <class Sync>
DR_HD inline void build_huf(const uint8_t* weights, int nsym, int tlog, uint16_t* tab, uint16_t* start, int lane,
                            int nl, Sync sync) {
  for (int wv = 1 + lane; wv <= tlog; wv += nl) {  // the worker of a weight numbers that weight's symbols
    uint32_t at = 0;
    for (int s = 0; s < nsym; ++s)
      if (weights[s] && weights[s] < wv) at += uint32_t(1) << (weights[s] - 1);
    for (int s = 0; s < nsym; ++s) {
      if (weights[s] != wv) continue;
      start[s] = uint16_t(at);
      at += uint32_t(1) << (wv - 1);
    }
  }
  sync();
  for (int s = 0; s < nsym; ++s) {
    const uint32_t wv = weights[s];
    if (!wv) continue;
    const uint32_t len = uint32_t(1) << (wv - 1);
    const uint16_t e = uint16_t((uint32_t(s) << 4) | (uint32_t(tlog) + 1 - wv));
    for (uint32_t k = uint32_t(lane); k < len; k += uint32_t(nl)) tab[start[s] + k] = e;
  }
  sync();
}

// One Huffman stream rd[s, e) into `count` symbols, each handed to put(index, byte). The stream must be
// consumed exactly.
template <class R, class Put>
DR_HD inline int huf_stream(const R& rd, uint64_t s, uint64_t e, const uint16_t* tab, int tlog, uint32_t count, Put put) {
  BackBits<R> br(rd);
  if (!br.init(s, e)) return E_HUF;
  for (uint32_t i = 0; i < count; ++i) {
    const uint32_t ent = tab[br.peek(uint32_t(tlog))];
    br.left -= int64_t(ent & 15);
    if (br.left < 0) return E_HUF;
    put(i, uint8_t(ent >> 4));
  }
  return br.left == 0 ? E_OK : E_HUF;
}

// Four Huffman streams the way libzstd 1.5.7 decodes them on a CPU with BMI2 when each has eight bytes
// or more, codes are at most 11 bits and the last segment is not empty (HufStreams::loose): its loop
// (HUF_decompress4X1_usingDTable_internal_fast) looks neither for a stream's end nor for its first byte.
// A stream may leave bits over; one that runs dry goes on into the bytes in front of it, down to
// `low`, the first byte of the jump table; below that the bits of the eight bytes at `low` come round
// again. What it does refuse depends on how far its lock-step rounds of five symbols per stream ran
// (their number follows from the first stream's position and the last segment's room, and they stop
// when a stream's position falls below the previous stream's): a stream whose position then lies more
// than eight bytes below its first byte. All of that is reproduced here. Worker `lane` of `nl` decodes
// the streams lane + k * nl, k < NS (NS: 1 or 4); `ipbuf` (four words all workers see) and `sync` carry the
// positions between them; put(stream, index, byte) takes a symbol. Every worker returns the same code.
template <class R>
struct LooseStream {  // one stream's state in huf_loose4: libzstd's ip[] and the bits taken since its last reload
  BackBits<R> br;
  int64_t ip;
  uint32_t nb;
  int st;  // which stream; >= 4: none
  DR_ZST_INLINE void init(const R& rd, int stream, const uint32_t* s5, uint64_t low) {
    st = stream;
    if (st >= 4) return;
    br = BackBits<R>(rd);
    br.init(low, s5[st + 1], true);  // eight bytes or more: cannot fail
    nb = uint32_t(int64_t(8 * (uint64_t(s5[st + 1]) - low)) - br.left);
    ip = int64_t(s5[st + 1]) - 8;
  }
  template <class Put>
  DR_ZST_INLINE void rounds(const uint16_t* tab, int tlog, uint32_t iters, uint32_t done, Put& put) {
    if (st >= 4) return;
    for (uint32_t it = 0; it < iters; ++it) {
      for (uint32_t j = 0; j < 5; ++j) {
        const uint32_t ent = tab[br.peek(uint32_t(tlog))];
        br.left -= int64_t(ent & 15);
        nb += ent & 15;
        put(st, done + 5 * it + j, uint8_t(ent >> 4));
      }
      ip -= int64_t(nb >> 3);
      nb &= 7;
    }
  }
  template <class Put>
  DR_ZST_INLINE void tail(const uint16_t* tab, int tlog, uint32_t done, uint32_t count, uint64_t first8, Put& put) {
    if (st >= 4) return;
    for (uint32_t i = done; i < count; ++i) {
      const uint32_t idx = br.left <= 0 ? uint32_t((first8 << (uint64_t(64 - br.left) & 63)) >> (64 - tlog))
                                        : br.peek(uint32_t(tlog));
      const uint32_t ent = tab[idx];
      br.left -= int64_t(ent & 15);
      put(st, i, uint8_t(ent >> 4));
    }
  }
};
template <int NS, class R, class Put, class Sync>
DR_HD inline int huf_loose4(const R& rd, const uint32_t* s5, uint32_t seg, uint32_t regen, uint64_t low, const uint16_t* tab,
                            int tlog, int64_t* ipbuf, Put put, int lane, int nl, Sync sync) {
  static_assert(NS == 1 || NS == 4, "one stream per worker, or all four on one");
  // named, not an array: the state stays in registers
  LooseStream<R> w0, w1, w2, w3;
  w0.init(rd, lane, s5, low);
  if (NS == 4) {
    w1.init(rd, lane + nl, s5, low);
    w2.init(rd, lane + 2 * nl, s5, low);
    w3.init(rd, lane + 3 * nl, s5, low);
  }
  uint32_t done = 0, room3 = regen - 3 * seg;
  int64_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;  // the four positions, as every worker sees them
  for (;;) {
    if (w0.st < 4) ipbuf[w0.st] = w0.ip;
    if (NS == 4) {
      if (w1.st < 4) ipbuf[w1.st] = w1.ip;
      if (w2.st < 4) ipbuf[w2.st] = w2.ip;
      if (w3.st < 4) ipbuf[w3.st] = w3.ip;
    }
    sync();
    a0 = ipbuf[0];
    a1 = ipbuf[1];
    a2 = ipbuf[2];
    a3 = ipbuf[3];
    sync();
    const uint64_t oiters = room3 / 5, iiters = uint64_t(a0 - int64_t(low)) / 7;
    const uint32_t iters = uint32_t(oiters < iiters ? oiters : iiters);
    if (iters == 0 || a1 < a0 || a2 < a1 || a3 < a2) break;
    w0.rounds(tab, tlog, iters, done, put);
    if (NS == 4) {
      w1.rounds(tab, tlog, iters, done, put);
      w2.rounds(tab, tlog, iters, done, put);
      w3.rounds(tab, tlog, iters, done, put);
    }
    done += 5 * iters;
    room3 -= 5 * iters;
  }
  if (a0 + 8 < int64_t(s5[0]) || a1 + 8 < int64_t(s5[1]) || a2 + 8 < int64_t(s5[2]) || a3 + 8 < int64_t(s5[3]))
    return E_HUF;
  uint64_t first8 = 0;
  le(rd, low, low + 8, 8, &first8);
  const uint32_t last = regen - 3 * seg;
  w0.tail(tab, tlog, done, w0.st == 3 ? last : seg, first8, put);
  if (NS == 4) {
    w1.tail(tab, tlog, done, w1.st == 3 ? last : seg, first8, put);
    w2.tail(tab, tlog, done, w2.st == 3 ? last : seg, first8, put);
    w3.tail(tab, tlog, done, w3.st == 3 ? last : seg, first8, put);
  }
  return E_OK;
}

// ---- literals section -------------------------------------------------------------------------------
enum LitType : int32_t { LT_RAW = 0, LT_RLE = 1, LT_COMPRESSED = 2, LT_TREELESS = 3 };
struct Literals {
  int32_t type;
  int32_t streams;     // 1 or 4 (Compressed, Treeless)
  uint32_t regen;      // bytes the section stands for
  uint32_t body;       // the stream position of what follows the section header: the raw bytes, the
                       // RLE byte, or the tree description (Compressed) / the streams (Treeless)
  uint32_t body_len;   // its bytes; the sequences section starts at body + body_len
};
constexpr uint32_t MIN_LITERALS_4_STREAMS = 6;
// The literals section header of a compressed block rd[pos, end). `room` is the output the page still
// has: all literals are output, so a section that stands for more is refused here, as libzstd does.
template <class R>
DR_HD inline int literals_header(const R& rd, uint64_t pos, uint64_t end, uint32_t block_max, uint64_t room,
                                 Literals* L) {
  if (end - pos < 2) return E_LITERALS;  // the smallest compressed block
  const uint32_t b0 = uint32_t(rd(pos));
  L->type = int32_t(b0 & 3);
  L->streams = 1;
  uint64_t v = 0;
  uint32_t lh, regen, csize = 0;
  if (L->type == LT_RAW || L->type == LT_RLE) {
    const uint32_t fmt = (b0 >> 2) & 3;
    lh = fmt == 1 ? 2 : fmt == 3 ? 3 : 1;
    if (fmt == 3 && end - pos < 3) return E_LITERALS;
    le(rd, pos, end, int(lh), &v);
    regen = uint32_t(v) >> (lh == 1 ? 3 : 4);
    if (regen > block_max) return E_LITERALS;
    if (L->type == LT_RLE) {
      if (fmt == 3 && end - pos < 4) return E_LITERALS;
      csize = 1;
    } else {
      csize = regen;
    }
  } else {
    if (end - pos < 5) return E_LITERALS;
    const uint32_t fmt = (b0 >> 2) & 3;
    le(rd, pos, end, 5, &v);
    if (fmt < 2) {
      lh = 3;
      regen = uint32_t(v >> 4) & 0x3ff;
      csize = uint32_t(v >> 14) & 0x3ff;
      L->streams = fmt == 0 ? 1 : 4;
    } else if (fmt == 2) {
      lh = 4;
      regen = uint32_t(v >> 4) & 0x3fff;
      csize = uint32_t(v >> 18) & 0x3fff;
      L->streams = 4;
    } else {
      lh = 5;
      regen = uint32_t(v >> 4) & 0x3ffff;
      csize = uint32_t(v >> 22) & 0x3ffff;
      L->streams = 4;
    }
    if (regen > block_max) return E_LITERALS;
    if (L->streams == 4 && regen < MIN_LITERALS_4_STREAMS) return E_LITERALS;
  }
  if (uint64_t(csize) + lh > end - pos) return E_LITERALS;
  if (regen > room) return E_OUTPUT;
  L->regen = regen;
  L->body = uint32_t(pos + lh);
  L->body_len = csize;
  return E_OK;
}

// Where the Huffman streams of a literals section lie: rd[s[k], s[k + 1]) decodes into literals
// [k * seg, ...) -- `seg` each, the last one the rest. body/len: the section after the tree description.
struct HufStreams {
  uint32_t s[5];
  uint32_t seg;
  int32_t loose;   // huf_loose4 decodes them: four streams of >= 8 bytes, codes of <= 11 bits, a last segment
};
template <class R>
DR_HD inline int huf_streams(const R& rd, uint32_t body, uint32_t len, int streams, uint32_t regen, int tlog,
                             HufStreams* hs) {
  hs->loose = 0;
  if (len == 0) return E_HUF;
  if (streams == 1) {
    hs->s[0] = body;
    hs->s[1] = hs->s[2] = hs->s[3] = hs->s[4] = body + len;
    hs->seg = regen;
    return E_OK;
  }
  if (len < 10) return E_HUF;
  uint32_t at = body + 6;
  for (int k = 0; k < 3; ++k) {
    hs->s[k] = at;
    at += (uint32_t(rd(body + 2 * uint32_t(k))) & 0xffu) | (uint32_t(rd(body + 2 * uint32_t(k) + 1)) & 0xffu) << 8;
  }
  hs->s[3] = at;
  hs->s[4] = body + len;
  if (at > body + len) return E_HUF;
  hs->seg = (regen + 3) / 4;
  hs->loose = tlog <= 11 && 3 * hs->seg < regen;
  for (int k = 0; k < 4; ++k) hs->loose = hs->loose && hs->s[k + 1] - hs->s[k] >= 8;
  return E_OK;
}

// ---- sequences section ------------------------------------------------------------------------------
DR_HD inline uint32_t ll_bits(uint32_t c) {
  return uint32_t("\0\0\0\0\0\0\0\0\0\0\0\0\0\0\0\0\1\1\1\1\2\2\3\3\4\6\7\10\11\12\13\14\15\16\17\20"[c]);
}
DR_HD inline uint32_t ll_base(uint32_t c) {
  return c < 16 ? c : c < 20 ? 16 + 2 * (c - 16) : c < 22 ? 24 + 4 * (c - 20) : c == 22 ? 32 : c == 23 ? 40 : c == 24 ? 48
       : uint32_t(1) << (c - 19);  // 25: 64 ... 35: 65536
}
DR_HD inline uint32_t ml_bits(uint32_t c) {
  return c < 32 ? 0 : uint32_t("\1\1\1\1\2\2\3\3\4\4\5\7\10\11\12\13\14\15\16\17\20"[c - 32]);
}
DR_HD inline uint32_t ml_base(uint32_t c) {
  return c < 32 ? c + 3 : c < 36 ? 35 + 2 * (c - 32) : c == 36 ? 43 : c == 37 ? 47 : c == 38 ? 51 : c == 39 ? 59
       : c == 40 ? 67 : c == 41 ? 83 : c == 42 ? 99 : (uint32_t(1) << (c - 36)) + 3;  // 43: 131 ... 52: 65539
}
DR_HD inline int default_norm(int which, int s) {  // which: 0 LL (36, log 6), 1 OF (29, log 5), 2 ML (53, log 6)
  if (which == 0)
    return s == 0 ? 4 : s == 1 || s == 25 ? 3 : s >= 32 ? -1 : (s >= 13 && s <= 15) || s >= 27 ? 1 : 2;
  if (which == 1) return s >= 24 ? -1 : s >= 6 && s <= 8 ? 2 : 1;
  return s == 1 ? 4 : s == 2 ? 3 : s >= 3 && s <= 8 ? 2 : s >= 46 ? -1 : 1;
}
DR_HD inline int default_syms(int which) { return which == 0 ? 36 : which == 1 ? 29 : 53; }
DR_HD inline int default_log(int which) { return which == 1 ? 5 : 6; }
DR_HD inline int max_sym(int which) { return which == 0 ? LL_MAX : which == 1 ? OF_MAX : ML_MAX; }
DR_HD inline int max_log(int which) { return which == 0 ? LL_LOG : which == 1 ? OF_LOG : ML_LOG; }

enum SeqMode : int32_t { SM_PREDEFINED = 0, SM_RLE = 1, SM_FSE = 2, SM_REPEAT = 3 };
struct SeqHeader {
  uint32_t nseq;
  int32_t mode[3];   // LL, OF, ML
  uint32_t next;     // the stream position after the count and the modes byte
};
// The sequences section header at rd[pos, end). With nseq == 0 the section must end there.
template <class R>
DR_HD inline int seq_header(const R& rd, uint64_t pos, uint64_t end, SeqHeader* h) {
  if (end <= pos) return E_SEQHDR;
  uint32_t n = uint32_t(rd(pos++));
  if (n > 0x7f) {
    if (n == 0xff) {
      if (end - pos < 2) return E_SEQHDR;
      n = ((uint32_t(rd(pos)) & 0xffu) | (uint32_t(rd(pos + 1)) & 0xffu) << 8) + 0x7f00;
      pos += 2;
    } else {
      if (end <= pos) return E_SEQHDR;
      n = ((n - 0x80) << 8) + uint32_t(rd(pos++));
    }
  }
  h->nseq = n;
  h->next = uint32_t(pos);
  if (n == 0) return pos == end ? E_OK : E_SEQHDR;
  if (end <= pos) return E_SEQHDR;
  const uint32_t m = uint32_t(rd(pos));
  if (m & 3) return E_SEQHDR;
  h->mode[0] = int32_t(m >> 6);
  h->mode[1] = int32_t((m >> 4) & 3);
  h->mode[2] = int32_t((m >> 2) & 3);
  h->next = uint32_t(pos + 1);
  return E_OK;
}

// What a frame carries from block to block.
struct Entropy {
  FseEntry fse[3][1 << LL_LOG];   // LL, OF (the first 256), ML
  uint16_t huf[1 << HUF_LOG_MAX];
  int32_t fse_log[3];
  int32_t huf_log;
  int32_t have_huf, have_fse;
  uint32_t rep[3];
  DR_HD void reset() {
    have_huf = have_fse = 0;
    rep[0] = 1;
    rep[1] = 4;
    rep[2] = 8;
  }
};

// What one table of a sequences section needs before build_fse: the counts of `which` by its mode, read
// at rd[pos, end) (pos moves past them). `*build`: norm[0, *nsym) at *tlog wait for build_fse (not for
// Repeat). One worker.
template <class R>
DR_HD inline int seq_table_prepare(const R& rd, uint64_t& pos, uint64_t end, int which, int mode, const Entropy& en,
                                   int16_t* norm, int* nsym, int* tlog, bool* build) {
  *build = true;
  if (mode == SM_REPEAT) {
    *build = false;
    return en.have_fse ? E_OK : E_NOTABLE;
  }
  if (mode == SM_PREDEFINED) {
    *nsym = default_syms(which);
    *tlog = default_log(which);
    for (int s = 0; s < *nsym; ++s) norm[s] = int16_t(default_norm(which, s));
    return E_OK;
  }
  if (mode == SM_RLE) {
    if (end <= pos) return E_INPUT;
    const int s = rd(pos++);
    if (s > max_sym(which)) return E_FSE;
    for (int i = 0; i < s; ++i) norm[i] = 0;
    norm[s] = 1;
    *nsym = s + 1;
    *tlog = 0;
    return E_OK;
  }
  uint32_t used;
  if (const int e = read_ncount(rd, pos, end, max_sym(which), norm, tlog, nsym, &used)) return e == E_INPUT ? E_FSE : e;
  if (*tlog > max_log(which)) return E_FSE;
  pos += used;
  return E_OK;
}

struct Sequence {
  uint32_t ll, ml, off;  // the offset as a distance; 0xffffffff / 0xfffffffe: refused
};
// The sequence decoder's state over the block's bitstream.
template <class R>
struct SeqState {
  BackBits<R> br;
  uint32_t st[3];
  DR_HD SeqState(const R& r) : br(r) {}
  DR_ZST_INLINE int init(uint64_t s, uint64_t e, const Entropy& en) {
    if (!br.init(s, e)) return E_SEQBITS;
    st[0] = br.take(uint32_t(en.fse_log[0]));
    st[1] = br.take(uint32_t(en.fse_log[1]));
    st[2] = br.take(uint32_t(en.fse_log[2]));
    return br.left < 0 ? E_SEQBITS : E_OK;
  }
  // The next sequence; `last`: no state update follows. rep[] is the frame's (updated).
  DR_ZST_INLINE int next(const Entropy& en, uint32_t* rep, bool last, Sequence* q) {
    const FseEntry l = en.fse[0][st[0]], o = en.fse[1][st[1]], m = en.fse[2][st[2]];
    const uint32_t oc = o.sym;
    uint32_t off;
    if (oc > 1) {
      off = ((uint32_t(1) << oc) - 3) + br.take(oc);
      rep[2] = rep[1];
      rep[1] = rep[0];
      rep[0] = off;
    } else {
      const uint32_t ll0 = l.sym == 0;
      if (oc == 0) {
        off = rep[ll0];
        rep[1] = rep[!ll0];
        rep[0] = off;
      } else {
        const uint32_t k = 1 + ll0 + br.take(1);
        uint32_t t = k == 3 ? rep[0] - 1 : rep[k];
        if (t == 0) t = 0xffffffffu;
        if (k != 1) rep[2] = rep[1];
        rep[1] = rep[0];
        rep[0] = off = t;
      }
    }
    q->off = off;
    q->ml = ml_base(m.sym) + br.take(ml_bits(m.sym));
    q->ll = ll_base(l.sym) + br.take(ll_bits(l.sym));
    if (!last) {
      st[0] = l.base + br.take(l.nbits);
      st[2] = m.base + br.take(m.nbits);
      st[1] = o.base + br.take(o.nbits);
    }
    return br.left < 0 ? E_SEQBITS : E_OK;
  }
};

// ---- XXH64 (seed 0) over get(i), i in [0, n) ------------------------------------------------------
template <class Get>
DR_HD inline uint64_t xxh64(Get get, uint64_t n) {
  constexpr uint64_t P1 = 0x9E3779B185EBCA87ull, P2 = 0xC2B2AE3D27D4EB4Full, P3 = 0x165667B19E3779F9ull,
                     P4 = 0x85EBCA77C2B2AE63ull, P5 = 0x27D4EB2F165667C5ull;
  auto rotl = [](uint64_t x, int r) { return (x << r) | (x >> (64 - r)); };
  auto word = [&](uint64_t at, int k) {
    uint64_t v = 0;
    for (int i = 0; i < k; ++i) v |= uint64_t(get(at + uint64_t(i))) << (8 * i);
    return v;
  };
  auto round = [&](uint64_t acc, uint64_t in) { return rotl(acc + in * P2, 31) * P1; };
  uint64_t p = 0, h;
  if (n >= 32) {
    uint64_t v[4] = {P1 + P2, P2, 0, 0 - P1};
    for (; p + 32 <= n; p += 32)
      for (int k = 0; k < 4; ++k) v[k] = round(v[k], word(p + 8 * uint64_t(k), 8));
    h = rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18);
    for (int k = 0; k < 4; ++k) h = (h ^ round(0, v[k])) * P1 + P4;
  } else {
    h = P5;
  }
  h += n;
  for (; p + 8 <= n; p += 8) h = rotl(h ^ round(0, word(p, 8)), 27) * P1 + P4;
  if (p + 4 <= n) {
    h = rotl(h ^ (word(p, 4) * P1), 23) * P2 + P3;
    p += 4;
  }
  for (; p < n; ++p) h = rotl(h ^ (uint64_t(get(p)) * P5), 11) * P1;
  h ^= h >> 33;
  h *= P2;
  h ^= h >> 29;
  h *= P3;
  h ^= h >> 32;
  return h;
}

}  // namespace zst
}  // namespace dr
