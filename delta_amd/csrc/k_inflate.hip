// K2a': GZIP page decompression (Parquet CompressionCodec 2) for checkpoint column chunks.
//
// DEFLATE is serial inside a stream: a symbol's position in the input is known only when the one
// before it has been decoded, and its meaning depends on the block's codes. The parallelism is the
// pages: one wave per page, every page of the plan in one launch. A wave keeps everything it touches
// in LDS and works in rounds of two phases:
//
//   decode   lane 0 walks the stream with the step functions of deflate_fmt.h -- the same ones the
//            host inflater calls, so both take the same decisions on a byte stream -- out of a
//            4 KiB window of the input that the wave staged with 16-byte loads. Literals go straight
//            into the output ring; matches are queued (position, length, distance). The phase ends
//            when the queue or the round's output span is full, the window runs low, or the block
//            needs the wave: new codes to build, a stored block to copy.
//   execute  the wave runs the queue in order, each match spread over the lanes (a match whose
//            distance is shorter than its length is read modulo the distance, so every lane reads
//            bytes that were complete before the match began), builds the codes of a new block
//            (dfl::build_codes: counts per length, offsets, symbol placement and the lookup tables
//            are spread over the lanes), copies a stored block's bytes from the window, and flushes
//            the ring's new bytes to the arena with aligned 16-byte stores.
//
// The ring is 64 KiB: the 32 KiB a distance may reach back plus the span of one round (literals are
// written ahead of the round's queued matches, so a round's output must not wrap onto bytes a queued
// match still reads). Back-references never read the wave's own global stores.
//
// Every loop is bounded by the input: a decode step consumes at least one bit or ends the block, a
// round consumes input or moves to the next phase, reading past n_in, writing past n_out and a
// distance beyond the member's output are errors. A refused page stops there and raises the error
// word; waves never wait for one another.
#include "deflate_fmt.h"
#include "dev_common.h"
#include "kernels.h"

namespace dr {
namespace dev {

constexpr uint32_t INF_WIN = 4096;     // input bytes staged per round
constexpr uint32_t INF_RING = 65536;   // output ring
constexpr uint32_t INF_SPAN = 16384;   // output bytes a round adds, at most (+ one match)
constexpr uint32_t INF_BATCH = 512;    // matches queued per round
static_assert(INF_RING >= 32768 + INF_SPAN + 258 + 16, "a round's output would wrap onto a match's source");

enum InfPhase : uint32_t { PH_HEADER = 0, PH_BLOCK, PH_SYMS, PH_STORED, PH_TRAILER, PH_DONE };
enum InfAction : uint32_t { ACT_NONE = 0, ACT_BUILD, ACT_COPY };

struct InfState {
  uint64_t bitpos;       // of the stream
  uint32_t produced;     // output bytes of the page so far
  uint32_t member;       // `produced` at the current member's start
  uint32_t phase, err, final, stored_left;
  uint32_t nent, action;
  uint32_t copy_src, copy_dst, copy_n;  // ACT_COPY: stream position, output position, bytes
  dfl::Block blk;
};

// The staged window as a byte source: w[i] is the stream's byte i - off; past the stream's end or the
// window's, -1 (the decode phase keeps its reads inside the window: see room() below).
struct WinSrc {
  const uint8_t* w;
  uint64_t off;
  uint64_t n;
  __device__ int operator()(uint64_t pos) const {
    const uint64_t i = pos + off;
    return pos < n && i < INF_WIN ? int(w[i]) : -1;
  }
};
struct BlockSync {
  __device__ void operator()() const { __syncthreads(); }
};

// The decode phase of one round (lane 0).
__device__ void inflate_decode(InfState& S, dfl::Tables& T, uint8_t* ring, const uint8_t* win, uint2* ent,
                               const uint8_t* in, uint32_t n_in, uint32_t n_out, uint64_t vb, uint32_t A, uint32_t B) {
  using namespace dfl;
  const WinSrc src{win, uint64_t(A) - vb, n_in};
  const PtrSrc whole{in, n_in};
  const bool covers_end = vb + INF_WIN >= uint64_t(n_in) + A;
  Bits<WinSrc> br(src, S.bitpos);
  // the reader may load `bytes` more without leaving the window
  auto room = [&](uint32_t bytes) { return covers_end || br.pos + A - vb + bytes <= INF_WIN; };
  uint32_t produced = S.produced, nent = 0, phase = S.phase;
  const uint32_t start = produced;
  int err = E_OK;
  S.action = ACT_NONE;
  for (bool go = true; go && err == E_OK;) {
    switch (phase) {
      case PH_HEADER: {  // read from memory: an extra field or a name may be longer than the window
        uint64_t pos = br.bitpos() >> 3;
        err = gz_header(whole, pos);
        S.member = produced;
        br.seek(pos);
        phase = PH_BLOCK;
        go = false;
        break;
      }
      case PH_BLOCK: {
        if (!room(BLOCK_HEADER_MAX_BYTES + 8)) {
          go = false;
          break;
        }
        err = block_header(br, T, &S.blk);
        if (err != E_OK) break;
        S.final = uint32_t(S.blk.final);
        if (S.blk.kind == BK_STORED) {
          S.stored_left = S.blk.stored_len;
          phase = PH_STORED;
        } else {
          S.action = ACT_BUILD;
          phase = PH_SYMS;
          go = false;
        }
        break;
      }
      case PH_STORED: {
        const uint64_t at = br.bitpos() >> 3;
        if (S.stored_left > n_in - at) {
          err = E_INPUT;
          break;
        }
        if (S.stored_left > n_out - produced) {
          err = E_OUTPUT;
          break;
        }
        const uint64_t wend = vb + INF_WIN - A;  // stream position of the window's end
        const uint64_t avail = covers_end ? n_in - at : wend > at ? wend - at : 0;
        const uint32_t used = produced - start, span = used < INF_SPAN ? INF_SPAN - used : 0;
        uint32_t n = S.stored_left;
        if (n > avail) n = uint32_t(avail);
        if (n > span) n = span;
        if (n) {
          S.action = ACT_COPY;
          S.copy_src = uint32_t(at);
          S.copy_dst = produced;
          S.copy_n = n;
          produced += n;
          S.stored_left -= n;
          br.seek(at + n);
        }
        if (S.stored_left == 0) phase = S.final ? PH_TRAILER : PH_BLOCK;
        if (n || S.stored_left) go = false;
        break;
      }
      case PH_SYMS: {
        for (;;) {
          if (nent >= INF_BATCH || produced - start >= INF_SPAN || !room(16)) {
            go = false;
            break;
          }
          Symbol s{};
          err = next_symbol(br, T, &s);
          if (err != E_OK) break;
          if (s.kind == SY_END) {
            phase = S.final ? PH_TRAILER : PH_BLOCK;
            break;
          }
          if (s.kind == SY_LITERAL) {
            if (produced >= n_out) {
              err = E_OUTPUT;
              break;
            }
            ring[(produced + B) & (INF_RING - 1)] = uint8_t(s.value);
            ++produced;
            continue;
          }
          if (s.dist > produced - S.member) {
            err = E_DISTANCE;
            break;
          }
          if (s.value > n_out - produced) {
            err = E_OUTPUT;
            break;
          }
          ent[nent++] = make_uint2(produced, (s.value << 16) | (s.dist - 1));
          produced += s.value;
        }
        break;
      }
      case PH_TRAILER: {
        br.align();
        uint64_t pos = br.bitpos() >> 3;
        err = gz_trailer(whole, pos, produced - S.member);
        if (err != E_OK) break;
        br.seek(pos);
        if (pos == n_in) {
          if (produced != n_out) err = E_OUTPUT;
          phase = PH_DONE;
          go = false;
        } else {
          phase = PH_HEADER;
        }
        break;
      }
      default:
        go = false;
        break;
    }
  }
  S.bitpos = br.bitpos();
  S.produced = produced;
  S.nent = nent;
  S.phase = phase;
  S.err = uint32_t(err);
}

__global__ void __launch_bounds__(64) k_inflate(const InflatePage* pages, uint32_t npages, uint32_t* error) {
  __shared__ __attribute__((aligned(16))) uint8_t ring[INF_RING];
  __shared__ __attribute__((aligned(16))) uint8_t win[INF_WIN];
  __shared__ dfl::Tables T;
  __shared__ uint2 ent[INF_BATCH];
  __shared__ InfState S;
  const uint32_t lane = threadIdx.x, page = blockIdx.x;
  if (page >= npages) return;
  const InflatePage pg = pages[page];
  const uint8_t* in = reinterpret_cast<const uint8_t*>(pg.in);
  uint8_t* out = reinterpret_cast<uint8_t*>(pg.out);
  const uint32_t n_in = pg.n_in, n_out = pg.n_out;
  // the window and the ring keep the 16-byte phase of the addresses they mirror: a 16-byte global
  // access is a 16-byte aligned LDS access
  const uint32_t A = uint32_t(pg.in & 15), B = uint32_t(pg.out & 15);
  constexpr uint32_t M = INF_RING - 1;
  if (lane == 0) {
    S.bitpos = 0;
    S.produced = S.member = 0;
    S.phase = PH_HEADER;
    S.err = 0;
    S.final = S.stored_left = S.nent = S.action = 0;
  }
  __syncthreads();
  uint32_t flushed = 0;
  // a round consumes at least one bit of input or moves to the next phase of a block
  const uint64_t max_rounds = 8 * (uint64_t(n_in) + 8) + 64;
  for (uint64_t round = 0;; ++round) {
    if (S.phase == PH_DONE || S.err) break;
    if (round >= max_rounds) {
      __syncthreads();
      if (lane == 0) S.err = dfl::E_INTERNAL;
      __syncthreads();
      break;
    }
    // stage the window: 16-byte loads from the 16-byte line that holds the reader's byte, none past
    // the line that holds the stream's last byte (the staged bytes are followed by a 64-byte pad)
    const uint64_t vb = ((S.bitpos >> 3) + A) & ~uint64_t(15);
    const uint64_t vend = (uint64_t(n_in) + A + 15) & ~uint64_t(15);
    const uint8_t* g0 = in - A;
    for (uint32_t k = lane; k < INF_WIN / 16; k += 64) {
      const uint64_t v = vb + 16 * uint64_t(k);
      uint4 x = make_uint4(0, 0, 0, 0);
      if (v < vend) x = *reinterpret_cast<const uint4*>(g0 + v);
      *reinterpret_cast<uint4*>(win + 16 * k) = x;
    }
    __syncthreads();
    if (lane == 0) inflate_decode(S, T, ring, win, ent, in, n_in, n_out, vb, A, B);
    __syncthreads();
    const uint32_t nent = S.nent, action = S.action;
    for (uint32_t e = 0; e < nent; ++e) {  // in order: a match may read the one before it
      const uint2 m = ent[e];
      const uint32_t pos = m.x, len = m.y >> 16, dist = (m.y & 0xffffu) + 1;
      for (uint32_t k = lane; k < len; k += 64) {
        const uint32_t o = dist >= len ? k : k % dist;
        ring[(pos + k + B) & M] = ring[(pos - dist + o + B) & M];
      }
      __syncthreads();
    }
    if (action == ACT_BUILD) {
      const int e = dfl::build_codes(T, S.blk, int(lane), 64, BlockSync());
      if (e != dfl::E_OK && lane == 0) S.err = uint32_t(e);
    } else if (action == ACT_COPY) {
      const uint32_t src = S.copy_src, dst = S.copy_dst, n = S.copy_n;
      const uint32_t w0 = uint32_t(uint64_t(src) + A - vb);  // < INF_WIN, and w0 + n <= INF_WIN
      for (uint32_t k = lane; k < n; k += 64) ring[(dst + k + B) & M] = win[(w0 + k) & (INF_WIN - 1)];
    }
    __syncthreads();
    // flush [flushed, produced): bytes up to the arena's next 16-byte line, then whole lines
    const uint32_t to = S.produced;
    uint32_t head_end = flushed + ((16 - ((flushed + B) & 15)) & 15);
    if (head_end > to) head_end = to;
    for (uint32_t i = flushed + lane; i < head_end; i += 64) out[i] = ring[(i + B) & M];
    const uint32_t nvec = (to - head_end) / 16;
    for (uint32_t v = lane; v < nvec; v += 64) {
      const uint32_t p = head_end + 16 * v;
      *reinterpret_cast<uint4*>(out + p) = *reinterpret_cast<const uint4*>(ring + ((p + B) & M));
    }
    flushed = head_end + 16 * nvec;
    __syncthreads();
  }
  if (S.err) {
    if (lane == 0) atomicMax(error, ~page);
    return;
  }
  for (uint32_t i = flushed + lane; i < S.produced; i += 64) out[i] = ring[(i + B) & M];
}

}  // namespace dev

void launch_inflate(const InflatePage* pages, uint32_t npages, uint32_t* error, hipStream_t st) {
  if (npages) DR_LAUNCH(dev::k_inflate, dim3(npages), dim3(64), 0, st, pages, npages, error);
}

}  // namespace dr
