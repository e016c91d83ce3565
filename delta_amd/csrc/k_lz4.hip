// K2a''': LZ4 page decompression (Parquet CompressionCodec 7, LZ4_RAW, and 5, Hadoop-framed LZ4) for
// checkpoint column chunks.
//
// LZ4 has no entropy stage: a sequence is a token, length bytes, literals and an offset, all on byte
// boundaries. What is serial is the walk from one token to the next; the copies are not. One wave per
// page, every page of the plan in one launch, in rounds of two phases as in k_inflate:
//
//   decode   lane 0 walks sequence headers with lz4::next -- the function the host decoder calls, so
//            both take the same decisions on a byte stream -- out of a 4 KiB window of the input that
//            the wave staged with 16-byte loads (a header byte behind the window -- the offset and
//            the next token behind a literal run that ends past it, or a long run of length bytes --
//            is read from memory; the round ends there and the next one stages from that byte). For
//            codec 5 it also
//            walks the unit and inner-block words. It queues (literal source, literal length, output
//            position, offset, match length); the walk yields the output positions, so there is no
//            scan. A sequence that does not fit the round's output span is cut, and its rest opens
//            the next round.
//   execute  the wave copies all queued literal runs into the output ring -- out of the window where a
//            run lies inside it, from memory otherwise, one loop per run --, then runs
//            the matches in order, each spread over the lanes (a match whose offset is shorter than
//            its length is read modulo the offset, so every lane reads bytes that were complete before
//            the match began), and flushes the ring's new bytes to the arena with aligned 16-byte
//            stores.
//
// The ring covers the 65,535 bytes an offset may reach back plus one round's span, so every match
// source is an LDS read: the kernel never reads its own global stores. Ring, window and queue take
// 79.6 KiB, so two workgroups share a CU's 160 KiB.
//
// Every loop is bounded by the input: lz4::next consumes at least one input byte or ends the block, a
// header takes four, a round queues a sequence, fills its span or ends the page, and a round counter
// caps the total. Reading past n_in, writing past n_out and an offset beyond the block's output are
// errors of lz4::next; literal runs are read only after it has checked them against the input. A
// refused page stops there and raises the error word; waves never wait for one another.
#include "dev_common.h"
#include "kernels.h"
#include "lz4_fmt.h"

namespace dr {
namespace dev {

constexpr uint32_t LZ_WIN = 4096;  // input bytes staged per round
constexpr uint32_t LZ_RING = LZ4_RING_BYTES, LZ_SPAN = LZ4_ROUND_SPAN, LZ_BATCH = LZ4_ROUND_BATCH;
static_assert(LZ_RING % 16 == 0, "the ring keeps the arena's 16-byte phase");
static_assert(LZ_RING >= 65536 + LZ_SPAN, "a round's output would wrap onto a match's source");

typedef const __attribute__((address_space(1))) uint8_t* LzGlobalBytes;
typedef uint32_t LzVec __attribute__((ext_vector_type(4)));  // a plain vector: HIP's uint4 is a class of the generic space
typedef const __attribute__((address_space(1))) LzVec* LzGlobalVec;
typedef __attribute__((address_space(1))) uint8_t* LzGlobalOut;
typedef __attribute__((address_space(1))) LzVec* LzGlobalOutVec;

struct LzQueue {
  uint32_t lit[LZ_BATCH], ll[LZ_BATCH], out[LZ_BATCH], off[LZ_BATCH], ml[LZ_BATCH];
};
struct LzState {
  lz4::Block b;         // the block being walked
  uint64_t pos;         // where the next unit or inner-block word lies
  uint32_t produced;    // output bytes of the page so far
  uint32_t unit_left;   // codec 5: what the unit still owes, at the current block's start
  uint32_t in_block, started, done, err, nq;
  uint32_t c_lit, c_ll, c_off, c_ml;  // the rest of a sequence cut at a round's end
};

// The staged window as a byte source: w[i] is the stream's byte w0 + i; a byte outside it comes from
// memory; -1 past the stream's end.
struct LzSrc {
  const uint8_t* w;
  LzGlobalBytes g;
  uint64_t w0, n;
  __device__ __forceinline__ int operator()(uint64_t pos) const {
    if (pos >= n) return -1;
    const uint64_t i = pos - w0;
    return i < LZ_WIN ? int(w[i]) : int(g[pos]);
  }
};

// The decode phase of one round (lane 0).
__device__ __forceinline__ void lz4_decode(LzState& S, LzQueue& Q, const LzSrc& src, uint32_t n_in, uint32_t n_out,
                                           uint32_t framing) {
  uint32_t nq = 0, produced = S.produced;
  const uint32_t start = produced;
  const uint64_t wend = src.w0 + LZ_WIN;
  int err = lz4::E_OK;
  auto push = [&](uint32_t lit, uint32_t ll, uint32_t off, uint32_t ml) {  // as much of it as the span takes
    uint32_t room = LZ_SPAN - (produced - start);
    const uint32_t tl = ll < room ? ll : room;
    room -= tl;
    const uint32_t tm = tl == ll ? (ml < room ? ml : room) : 0;
    Q.lit[nq] = lit;
    Q.ll[nq] = tl;
    Q.out[nq] = produced;
    Q.off[nq] = off;
    Q.ml[nq] = tm;
    ++nq;
    produced += tl + tm;
    S.c_lit = lit + tl;
    S.c_ll = ll - tl;
    S.c_off = off;
    S.c_ml = ml - tm;
  };
  while (err == lz4::E_OK && !S.done && nq < LZ_BATCH && produced - start < LZ_SPAN) {
    if (S.c_ll | S.c_ml) {
      push(S.c_lit, S.c_ll, S.c_off, S.c_ml);
      continue;
    }
    if (!S.in_block) {
      if (framing == lz4::F_BARE) {
        if (S.started) {
          S.done = 1;
          break;
        }
        lz4::begin(S.b, 0, n_in, n_out);
      } else {
        uint64_t pos = S.pos;
        if (S.unit_left == 0) {
          if (pos >= n_in) {
            S.done = 1;
            break;
          }
          uint32_t U = 0;
          err = lz4::unit_header(src, pos, n_in, uint64_t(n_out - produced), &U);
          if (err) break;
          S.unit_left = U;
        }
        uint32_t C = 0;
        err = lz4::inner_header(src, pos, n_in, &C);
        if (err) break;
        lz4::begin(S.b, pos, C, S.unit_left);
        S.pos = pos + C;
      }
      S.in_block = S.started = 1;
    }
    if (uint64_t(S.b.ip) + 32 > wend && wend < n_in) break;  // the next header would leave the window
    lz4::Seq q{};
    err = lz4::next(src, S.b, &q);
    if (err) break;
    if (q.last) {
      S.in_block = 0;
      if (framing != lz4::F_BARE) S.unit_left -= uint32_t(S.b.op);
    }
    if (q.ll | q.ml) push(uint32_t(q.lit), q.ll, q.off, q.ml);
  }
  if (!err && S.done && produced != n_out) err = lz4::E_OUTPUT;
  S.produced = produced;
  S.nq = err ? 0 : nq;
  S.err = uint32_t(err);
}

__device__ __forceinline__ uint32_t lz_wrap(uint32_t i) { return i >= LZ_RING ? i - LZ_RING : i; }

__global__ void __launch_bounds__(64) k_lz4(const InflatePage* pages, uint32_t npages, uint32_t first, uint32_t* error) {
  __shared__ __attribute__((aligned(16))) uint8_t ring[LZ_RING];
  __shared__ __attribute__((aligned(16))) uint8_t win[LZ_WIN];
  __shared__ LzQueue Q;
  __shared__ LzState S;
  const uint32_t lane = threadIdx.x, page = blockIdx.x;
  if (page >= npages) return;
  const InflatePage pg = pages[page];
  const LzGlobalBytes in = (LzGlobalBytes) reinterpret_cast<const uint8_t*>(pg.in);
  const LzGlobalOut out = (LzGlobalOut) reinterpret_cast<uint8_t*>(pg.out);
  const uint32_t n_in = pg.n_in, n_out = pg.n_out, framing = pg.pad_;
  // the window and the ring keep the 16-byte phase of the addresses they mirror: a 16-byte global
  // access is a 16-byte aligned LDS access
  const uint32_t A = uint32_t(pg.in & 15), B = uint32_t(pg.out & 15);
  if (lane == 0) {
    S.pos = 0;
    S.produced = S.unit_left = 0;
    S.in_block = S.started = S.done = S.err = S.nq = 0;
    S.c_lit = S.c_ll = S.c_off = S.c_ml = 0;
    S.b = lz4::Block{};
  }
  __syncthreads();
  uint32_t flushed = 0;
  // a round queues a sequence (at least one input byte), fills its span, or ends the page
  const uint64_t max_rounds = 2 * uint64_t(n_in) + uint64_t(n_out) / LZ_SPAN + 64;
  for (uint64_t round = 0;; ++round) {
    if (S.done || S.err) break;
    if (round >= max_rounds) {
      __syncthreads();
      if (lane == 0) S.err = lz4::E_INTERNAL;
      __syncthreads();
      break;
    }
    // stage the window: 16-byte loads from the 16-byte line that holds the walker's byte, none past
    // the line that holds the stream's last byte (the staged bytes are followed by a 64-byte pad)
    const uint64_t rpos = S.in_block ? uint64_t(S.b.ip) : S.pos;
    const uint64_t vb = (rpos + A) & ~uint64_t(15);
    const uint64_t vend = (uint64_t(n_in) + A + 15) & ~uint64_t(15);
    const LzGlobalBytes g0 = in - A;
    for (uint32_t k = lane; k < LZ_WIN / 16; k += 64) {
      const uint64_t v = vb + 16 * uint64_t(k);
      LzVec x = {0, 0, 0, 0};
      if (v < vend) x = *(LzGlobalVec)(g0 + v);
      *reinterpret_cast<LzVec*>(win + 16 * k) = x;
    }
    __syncthreads();
    if (lane == 0) lz4_decode(S, Q, LzSrc{win, in, vb - A, n_in}, n_in, n_out, framing);
    __syncthreads();
    const uint32_t nq = S.nq;
    for (uint32_t e = 0; e < nq; ++e) {  // literal runs: independent of one another
      const uint32_t ll = Q.ll[e];
      if (!ll) continue;
      const uint32_t d0 = (Q.out[e] + B) % LZ_RING;
      const uint64_t w = uint64_t(Q.lit[e]) - (vb - A);  // the run's place in the window, if it lies there
      if (w < LZ_WIN && w + ll <= LZ_WIN) {
        for (uint32_t k = lane; k < ll; k += 64) ring[lz_wrap(d0 + k)] = win[uint32_t(w) + k];
      } else {
        const LzGlobalBytes lit = in + Q.lit[e];
        for (uint32_t k = lane; k < ll; k += 64) ring[lz_wrap(d0 + k)] = lit[k];
      }
    }
    __syncthreads();
    for (uint32_t e = 0; e < nq; ++e) {  // matches, in order: one may read the one before it
      const uint32_t ml = Q.ml[e];
      if (!ml) continue;
      const uint32_t off = Q.off[e], m = Q.out[e] + Q.ll[e];
      const uint32_t d0 = (m + B) % LZ_RING, s0 = (m - off + B) % LZ_RING;
      if (off >= ml) {
        for (uint32_t k = lane; k < ml; k += 64) ring[lz_wrap(d0 + k)] = ring[lz_wrap(s0 + k)];
      } else {  // offsets 1, 2, 3 are the runs: the source index steps by 64 modulo the offset
        const uint32_t step = 64 % off;
        uint32_t o = lane % off;
        for (uint32_t k = lane; k < ml; k += 64) {
          ring[lz_wrap(d0 + k)] = ring[lz_wrap(s0 + o)];
          o += step;
          if (o >= off) o -= off;
        }
      }
      __syncthreads();
    }
    // flush [flushed, produced): bytes up to the arena's next 16-byte line, then whole lines
    const uint32_t to = S.produced;
    uint32_t head_end = flushed + ((16 - ((flushed + B) & 15)) & 15);
    if (head_end > to) head_end = to;
    for (uint32_t i = flushed + lane; i < head_end; i += 64) out[i] = ring[(i + B) % LZ_RING];
    const uint32_t nvec = (to - head_end) / 16;
    for (uint32_t v = lane; v < nvec; v += 64) {
      const uint32_t p = head_end + 16 * v;
      *(LzGlobalOutVec)(out + p) = *reinterpret_cast<const LzVec*>(ring + ((p + B) % LZ_RING));
    }
    flushed = head_end + 16 * nvec;
    __syncthreads();
  }
  if (S.err) {
    if (lane == 0) atomicMax(error, ~(first + page));
    return;
  }
  for (uint32_t i = flushed + lane; i < S.produced; i += 64) out[i] = ring[(i + B) % LZ_RING];
}

}  // namespace dev

void launch_lz4(const InflatePage* pages, uint32_t npages, uint32_t first, uint32_t* error, hipStream_t st) {
  if (npages) DR_LAUNCH(dev::k_lz4, dim3(npages), dim3(64), 0, st, pages, npages, first, error);
}

}  // namespace dr
