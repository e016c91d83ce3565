// Host ZSTD page decoder (RFC 8878 frames; the rules are zstd_fmt.h's, which the device kernel walks
// too). No libzstd: the project carries its own, as it does for SNAPPY and GZIP.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "zstd_fmt.h"

namespace dr {
// Decodes the concatenated frames `in[0..n)` (skippable ones are passed over) into `out[0..out_len)`.
// True only if the frames' outputs fill exactly out_len bytes; a frame's content size and content
// checksum are verified where it carries them. `why` (optional) receives the zst::Err code.
bool zstd_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t out_len, int* why = nullptr);

namespace zst {
// One compressed block in[pos, end) of a frame whose output began at out[frame0]; `op` moves on.
inline int decode_block(const PtrSrc& src, const uint8_t* in, uint64_t pos, uint64_t end, const Frame& f, Entropy& en,
                        HufScratch& hs, std::vector<uint8_t>& litbuf, uint8_t* out, size_t out_len, size_t frame0,
                        size_t& op) {
  Literals L{};
  if (const int e = literals_header(src, pos, end, f.block_max, out_len - op, &L)) return e;
  const uint8_t* lit = in + L.body;  // LT_RAW
  if (L.type == LT_COMPRESSED || L.type == LT_TREELESS) {
    uint32_t body = L.body, len = L.body_len;
    if (L.type == LT_COMPRESSED) {
      int nsym, tlog;
      uint32_t used;
      if (const int e = huf_read_weights(src, body, uint64_t(body) + len, hs, &nsym, &tlog, &used)) return e;
      if (used >= len) return E_HUF;
      build_huf(hs.weights, nsym, tlog, en.huf, hs.next, 0, 1, NoSync());
      en.huf_log = tlog;
      en.have_huf = 1;
      body += used;
      len -= used;
    } else if (!en.have_huf) {
      return E_NOTREE;
    }
    HufStreams st{};
    if (const int e = huf_streams(src, body, len, L.streams, L.regen, en.huf_log, &st)) return e;
    litbuf.resize(L.regen + 1);
    if (st.loose) {
      int64_t ipbuf[4];
      uint8_t* lb = litbuf.data();
      if (const int e = huf_loose4<4>(src, st.s, st.seg, L.regen, uint64_t(body), en.huf, en.huf_log, ipbuf,
                                      [&](int k, uint32_t i, uint8_t b) { lb[uint32_t(k) * st.seg + i] = b; }, 0, 1, NoSync()))
        return e;
    } else {
      for (int k = 0; k < L.streams; ++k) {
        const uint32_t first = uint32_t(k) * st.seg, count = k == L.streams - 1 ? L.regen - first : st.seg;
        uint8_t* dst = litbuf.data() + first;
        if (const int e = huf_stream(src, st.s[k], st.s[k + 1], en.huf, en.huf_log, count,
                                     [&](uint32_t i, uint8_t b) { dst[i] = b; }))
          return e;
      }
    }
    lit = litbuf.data();
  }
  const bool rle = L.type == LT_RLE;
  const uint8_t rle_byte = rle ? in[L.body] : 0;
  auto put_literals = [&](uint32_t from, uint32_t k) {
    if (!k) return;
    if (rle) memset(out + op, rle_byte, k);
    else memcpy(out + op, lit + from, k);
    op += k;
  };
  SeqHeader sh{};
  if (const int e = seq_header(src, uint64_t(L.body) + L.body_len, end, &sh)) return e;
  uint32_t lit_at = 0;
  if (sh.nseq) {
    uint64_t at = sh.next;
    for (int t = 0; t < 3; ++t) {
      int nsym = 0, tlog = 0;
      bool build;
      if (const int e = seq_table_prepare(src, at, end, t, sh.mode[t], en, hs.norm, &nsym, &tlog, &build)) return e;
      if (!build) continue;
      build_fse(hs.norm, nsym, tlog, en.fse[t], hs.next, 0, 1, NoSync());
      en.fse_log[t] = tlog;
    }
    en.have_fse = 1;
    SeqState<PtrSrc> ss(src);
    if (const int e = ss.init(at, end, en)) return e;
    for (uint32_t i = 0; i < sh.nseq; ++i) {
      Sequence q{};
      if (const int e = ss.next(en, en.rep, i + 1 == sh.nseq, &q)) return e;
      if (q.ll > L.regen - lit_at) return E_LITLEN;
      if (uint64_t(q.ll) + q.ml > out_len - op) return E_OUTPUT;
      put_literals(lit_at, q.ll);
      lit_at += q.ll;
      if (q.off > op - frame0) return E_OFFSET;
      for (uint32_t k = 0; k < q.ml; ++k) out[op + k] = out[op - q.off + k];  // overlap-safe
      op += q.ml;
    }
    if (ss.br.left != 0) return E_SEQBITS;
  }
  if (L.regen - lit_at > out_len - op) return E_OUTPUT;
  put_literals(lit_at, L.regen - lit_at);
  return E_OK;
}

// The frames of a page, as the zst::Err code. Inline, so that a unit which needs a page decoded (the
// host decoders of parquet_meta.cpp) links without zstd_host.cpp.
inline int decode_frames(const uint8_t* in, size_t n, uint8_t* out, size_t out_len) {
  const PtrSrc src{in, n};
  auto en = std::make_unique<Entropy>();
  auto hs = std::make_unique<HufScratch>();
  std::vector<uint8_t> litbuf;
  uint64_t pos = 0;
  size_t op = 0;
  while (pos < n) {
    Frame f{};
    if (const int e = frame_header(src, n, pos, &f)) return e;
    if (f.skippable) continue;
    const size_t frame0 = op;
    en->reset();
    for (;;) {
      Block b{};
      if (const int e = block_header(src, n, pos, f.block_max, &b)) return e;
      if (b.type == BT_COMPRESSED) {
        if (const int e = decode_block(src, in, pos, pos + b.size, f, *en, *hs, litbuf, out, out_len, frame0, op)) return e;
        pos += b.size;
      } else {
        if (b.size > out_len - op) return E_OUTPUT;
        if (b.type == BT_RAW) {
          if (b.size) memcpy(out + op, in + pos, b.size);
          pos += b.size;
        } else {
          if (b.size) memset(out + op, in[pos], b.size);
          pos += 1;
        }
        op += b.size;
      }
      if (b.last) break;
    }
    if (f.has_size && f.content_size != op - frame0) return E_CONTENT;
    if (f.checksum) {
      uint64_t want;
      if (!le(src, pos, n, 4, &want)) return E_INPUT;
      const uint8_t* base = out + frame0;
      if (uint32_t(xxh64([&](uint64_t i) { return base[i]; }, op - frame0)) != uint32_t(want)) return E_CHECKSUM;
      pos += 4;
    }
  }
  return op == out_len ? E_OK : E_OUTPUT;
}
}  // namespace zst
}  // namespace dr
