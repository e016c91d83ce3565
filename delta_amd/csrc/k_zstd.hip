// K2a'': ZSTD page decompression (Parquet CompressionCodec 6) for checkpoint column chunks.
//
// One 64-lane workgroup (one wave: no wave ever waits for another) per page; workgroups take pages
// from an atomic counter, so the grid -- and with it the literal slabs below -- is capped while any
// number of pages is served. Every decision about the byte stream is taken by the functions of
// zstd_fmt.h, the ones the host decoder calls, so both sides accept and refuse alike. Per block:
//
//   headers    lane 0 reads the block, literals and sequences headers and the table descriptions;
//   tables     the Huffman lookup table and the three FSE tables are built by all lanes
//              (zst::build_huf / build_fse with __syncthreads as the barrier);
//   literals   up to four Huffman streams decode on four lanes into the workgroup's slab in global
//              memory (a block's literals may reach 128 KiB: too much for LDS) -- in libzstd's lock
//              step where its four-stream loop applies (zst::huf_loose4); Raw and RLE literals are read
//              where they lie;
//   sequences  lane 0 walks the FSE states and queues up to 64 (literal length, match length, offset)
//              triples with their literal and output positions, checking each against the block's
//              literals, the page's room and the frame's output so far; the wave then copies all
//              literal runs of the batch, and executes the matches in order, each spread over the
//              lanes (read modulo the offset when the offset is shorter than the match).
//
// A match may reach back over the whole frame, so it reads the wave's own earlier stores from the
// arena, and literal copies read the slab the same way: with agent-scope relaxed atomic loads, which
// bypass this CU's L1 (a plain load could hit a line the L1 took in before the store), and only after
// the stores they depend on have drained (s_waitcnt vmcnt(0)); `drained` tracks the output position
// below which that holds, so a match whose source lies below it -- a far match -- pays no wait.
//
// Every loop is bounded by the input: a frame takes at least 5 bytes, a block 3, a sequence batch is
// counted by the block's own sequence count, and a step counter caps the total. Reading past n_in,
// writing past n_out, an offset beyond the frame's output and a literal length beyond the block's
// literals are errors: headers, tables and bitstreams go through a bounds-checked reader; a Raw block's
// bytes, Raw literals and the RLE bytes are plain loads of extents that block_header and
// literals_header have checked against the input first. A refused page stops
// there and raises the error word.
#include <stdexcept>

#include "dev_common.h"
#include "kernels.h"
#include "zstd_fmt.h"

namespace dr {
namespace dev {

constexpr uint32_t ZS_BATCH = 64;

struct ZsSrc {  // the page's compressed bytes; -1 past the end
  const uint8_t* b;
  uint64_t n;
  __device__ int operator()(uint64_t pos) const { return pos < n ? int(b[pos]) : -1; }
};
struct ZsSync {
  __device__ void operator()() const { __syncthreads(); }
};
// a byte this workgroup stored earlier in this launch
__device__ __forceinline__ uint8_t zs_own(const uint8_t* p) {
  // as a global (not flat) load: the arena and the slabs are global memory
  typedef const __attribute__((address_space(1))) uint8_t* GlobalBytes;
  return __hip_atomic_load((GlobalBytes)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void zs_drain() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

struct ZsState {
  uint64_t pos;             // of the stream
  uint64_t at;              // inside the sequences section
  uint64_t steps;
  int64_t ip4[4];           // huf_loose4's exchange
  uint32_t op;              // output bytes of the page so far
  uint32_t frame0;          // `op` at the current frame's start
  uint32_t err;
  uint32_t job;
  uint32_t more_frames, skippable;
  uint32_t lit_at;          // literals of the block consumed so far
  uint32_t seq_done, nb;
  uint32_t used;
  int32_t nsym, tlog, build;
  zst::Frame f;
  zst::Block b;
  zst::Literals L;
  zst::HufStreams hs;
  zst::SeqHeader sh;
};
struct ZsBatch {
  uint32_t lit[ZS_BATCH], out[ZS_BATCH], ll[ZS_BATCH], ml[ZS_BATCH], off[ZS_BATCH];
};

__global__ void __launch_bounds__(64) k_zstd(const InflatePage* pages, uint32_t npages, uint32_t first, uint32_t* error,
                                             uint32_t* counter, uint8_t* slabs) {
  __shared__ zst::Entropy en;
  __shared__ zst::HufScratch H;
  __shared__ ZsBatch Q;
  __shared__ ZsState S;
  const uint32_t lane = threadIdx.x;
  uint8_t* slab = slabs + uint64_t(blockIdx.x) * ZSTD_SLAB_BYTES;
  for (;;) {
    __syncthreads();
    if (lane == 0) S.job = atomicAdd(counter, 1u);
    __syncthreads();
    const uint32_t job = S.job;
    if (job >= npages) return;
    const InflatePage pg = pages[job];
    const uint8_t* in = reinterpret_cast<const uint8_t*>(pg.in);
    uint8_t* out = reinterpret_cast<uint8_t*>(pg.out);
    const uint32_t n_in = pg.n_in, n_out = pg.n_out;
    const ZsSrc src{in, n_in};
    const uint64_t max_steps = 1024 * uint64_t(n_in) + 4096;
    if (lane == 0) {
      S.pos = 0;
      S.op = S.frame0 = 0;
      S.err = 0;
      S.steps = 0;
    }
    uint32_t drained = 0;  // output below this position has left the wave's store queue
    zst::SeqState<ZsSrc> ss(src);  // lane 0's
    // ---- frames ----
    for (;;) {
      __syncthreads();
      if (lane == 0) {
        S.more_frames = S.pos < n_in;
        S.skippable = 0;
        if (S.more_frames) {
          uint64_t pos = S.pos;
          S.err = uint32_t(zst::frame_header(src, n_in, pos, &S.f));
          S.pos = pos;
          S.skippable = uint32_t(S.f.skippable);
          S.frame0 = S.op;
          en.reset();
          if (++S.steps > max_steps) S.err = zst::E_INTERNAL;
        }
      }
      __syncthreads();
      if (S.err || !S.more_frames) break;
      if (S.skippable) continue;
      // ---- blocks ----
      for (;;) {
        __syncthreads();
        if (lane == 0) {
          uint64_t pos = S.pos;
          int e = zst::block_header(src, n_in, pos, S.f.block_max, &S.b);
          S.pos = pos;
          if (!e && S.b.type != zst::BT_COMPRESSED && S.b.size > n_out - S.op) e = zst::E_OUTPUT;
          if (++S.steps > max_steps) e = zst::E_INTERNAL;
          S.err = uint32_t(e);
        }
        __syncthreads();
        if (S.err) break;
        const uint32_t btype = uint32_t(S.b.type), bsize = S.b.size, op0 = S.op;
        const uint64_t bpos = S.pos;
        if (btype == zst::BT_RAW) {
          for (uint32_t k = lane; k < bsize; k += 64) out[op0 + k] = in[bpos + k];
          __syncthreads();
          if (lane == 0) {
            S.pos = bpos + bsize;
            S.op = op0 + bsize;
          }
        } else if (btype == zst::BT_RLE) {
          const uint8_t v = in[bpos];
          for (uint32_t k = lane; k < bsize; k += 64) out[op0 + k] = v;
          __syncthreads();
          if (lane == 0) {
            S.pos = bpos + 1;
            S.op = op0 + bsize;
          }
        } else {
          const uint64_t bend = bpos + bsize;
          // ---- literals ----
          if (lane == 0) {
            int e = zst::literals_header(src, bpos, bend, S.f.block_max, uint64_t(n_out - op0), &S.L);
            S.used = 0;
            if (!e && S.L.type == zst::LT_COMPRESSED) {
              e = zst::huf_read_weights(src, S.L.body, uint64_t(S.L.body) + S.L.body_len, H, &S.nsym, &S.tlog, &S.used);
              if (!e && S.used >= S.L.body_len) e = zst::E_HUF;
            } else if (!e && S.L.type == zst::LT_TREELESS && !en.have_huf) {
              e = zst::E_NOTREE;
            }
            S.err = uint32_t(e);
          }
          __syncthreads();
          if (S.err) break;
          const uint32_t ltype = uint32_t(S.L.type), regen = S.L.regen;
          if (ltype == zst::LT_COMPRESSED) {
            zst::build_huf(H.weights, S.nsym, S.tlog, en.huf, H.next, int(lane), 64, ZsSync());
            if (lane == 0) {
              en.huf_log = S.tlog;
              en.have_huf = 1;
            }
            __syncthreads();
          }
          if (ltype >= zst::LT_COMPRESSED) {
            if (lane == 0)
              S.err = uint32_t(zst::huf_streams(src, S.L.body + S.used, S.L.body_len - S.used, S.L.streams, regen,
                                                en.huf_log, &S.hs));
            __syncthreads();
            if (S.err) break;
            if (S.hs.loose) {  // the four streams in libzstd's lock step (zst::huf_loose4), one lane each
              const uint32_t seg = S.hs.seg;  // put: stream * seg + index < regen <= 128 KiB
              const int e = zst::huf_loose4<1>(src, S.hs.s, seg, regen, uint64_t(S.L.body) + S.used, en.huf, en.huf_log,
                                               S.ip4, [&](int st, uint32_t i, uint8_t b) { slab[uint32_t(st) * seg + i] = b; },
                                               int(lane), 64, ZsSync());
              if (e && lane == 0) S.err = uint32_t(e);
            } else if (lane < uint32_t(S.L.streams)) {
              const uint32_t firstsym = lane * S.hs.seg;
              const uint32_t count = lane + 1 == uint32_t(S.L.streams) ? regen - firstsym : S.hs.seg;
              uint8_t* dst = slab + firstsym;  // firstsym + count <= regen <= 128 KiB
              const int e = zst::huf_stream(src, S.hs.s[lane], S.hs.s[lane + 1], en.huf, en.huf_log, count,
                                            [&](uint32_t i, uint8_t b) { dst[i] = b; });
              if (e) atomicMax(&S.err, uint32_t(e));
            }
            zs_drain();
            if (S.err) break;
          }
          const uint8_t* raw_lit = in + S.L.body;
          const uint8_t rle_lit = ltype == zst::LT_RLE ? in[S.L.body] : uint8_t(0);
          auto literal = [&](uint32_t i) -> uint8_t {
            return ltype == zst::LT_RAW ? raw_lit[i] : ltype == zst::LT_RLE ? rle_lit : zs_own(slab + i);
          };
          // ---- sequences ----
          if (lane == 0) {
            S.err = uint32_t(zst::seq_header(src, uint64_t(S.L.body) + S.L.body_len, bend, &S.sh));
            S.at = S.sh.next;
            S.lit_at = 0;
            S.seq_done = 0;
          }
          __syncthreads();
          if (S.err) break;
          const uint32_t nseq = S.sh.nseq;
          if (nseq) {
            for (int t = 0; t < 3; ++t) {
              if (lane == 0) {
                uint64_t at = S.at;
                bool build = false;
                S.err = uint32_t(zst::seq_table_prepare(src, at, bend, t, S.sh.mode[t], en, H.norm, &S.nsym, &S.tlog, &build));
                S.at = at;
                S.build = build;
              }
              __syncthreads();
              if (S.err) break;
              if (S.build) {
                zst::build_fse(H.norm, S.nsym, S.tlog, en.fse[t], H.next, int(lane), 64, ZsSync());
                if (lane == 0) en.fse_log[t] = S.tlog;
              }
              __syncthreads();
            }
            if (S.err) break;
            if (lane == 0) {
              en.have_fse = 1;
              S.err = uint32_t(ss.init(S.at, bend, en));
            }
            __syncthreads();
            if (S.err) break;
            while (S.seq_done < nseq) {
              __syncthreads();
              if (lane == 0) {  // the next batch
                uint32_t nb = 0, lit_at = S.lit_at, op = S.op, done = S.seq_done;
                int e = zst::E_OK;
                while (nb < ZS_BATCH && done < nseq) {
                  zst::Sequence q{};
                  e = ss.next(en, en.rep, done + 1 == nseq, &q);
                  if (e) break;
                  if (q.ll > regen - lit_at) e = zst::E_LITLEN;
                  else if (uint64_t(q.ll) + q.ml > uint64_t(n_out - op)) e = zst::E_OUTPUT;
                  else if (q.off > op + q.ll - S.frame0) e = zst::E_OFFSET;
                  if (e) break;
                  Q.lit[nb] = lit_at;
                  Q.out[nb] = op;
                  Q.ll[nb] = q.ll;
                  Q.ml[nb] = q.ml;
                  Q.off[nb] = q.off;
                  lit_at += q.ll;
                  op += q.ll + q.ml;
                  ++nb;
                  ++done;
                }
                if (!e && done == nseq && ss.br.left != 0) e = zst::E_SEQBITS;
                if (++S.steps > max_steps) e = zst::E_INTERNAL;
                S.err = uint32_t(e);
                S.nb = e ? 0 : nb;
                S.lit_at = lit_at;
                S.op = op;
                S.seq_done = done;
              }
              __syncthreads();
              if (S.err) break;
              const uint32_t nb = S.nb;
              for (uint32_t i = 0; i < nb; ++i) {  // literal runs: independent of one another
                const uint32_t ll = Q.ll[i], o = Q.out[i], la = Q.lit[i];
                for (uint32_t k = lane; k < ll; k += 64) out[o + k] = literal(la + k);
              }
              for (uint32_t i = 0; i < nb; ++i) {  // matches, in order: one may read the one before it
                const uint32_t ml = Q.ml[i], off = Q.off[i], m = Q.out[i] + Q.ll[i];
                const uint32_t src_end = m - off + (off < ml ? off : ml);
                if (src_end > drained) {
                  zs_drain();
                  drained = m;
                }
                for (uint32_t k = lane; k < ml; k += 64) out[m + k] = zs_own(out + (m - off) + (off >= ml ? k : k % off));
              }
            }
            if (S.err) break;
          }
          // the literals no sequence took
          __syncthreads();
          if (lane == 0 && regen - S.lit_at > n_out - S.op) S.err = zst::E_OUTPUT;
          __syncthreads();
          if (S.err) break;
          const uint32_t rest = regen - S.lit_at, o = S.op, la = S.lit_at;
          for (uint32_t k = lane; k < rest; k += 64) out[o + k] = literal(la + k);
          zs_drain();  // the slab is free for the next block
          if (lane == 0) {
            S.op = o + rest;
            S.pos = bend;
          }
          drained = o + rest;
        }
        __syncthreads();
        if (S.b.last) break;
      }
      if (S.err) break;
      // ---- the frame's end ----
      __syncthreads();
      if (S.f.checksum) zs_drain();
      if (lane == 0) {
        int e = zst::E_OK;
        if (S.f.has_size && S.f.content_size != uint64_t(S.op - S.frame0)) e = zst::E_CONTENT;
        if (!e && S.f.checksum) {
          uint64_t want = 0;
          if (!zst::le(src, S.pos, n_in, 4, &want)) {
            e = zst::E_INPUT;
          } else {
            const uint8_t* base = out + S.frame0;
            const uint64_t h = zst::xxh64([&](uint64_t i) { return zs_own(base + i); }, uint64_t(S.op - S.frame0));
            if (uint32_t(h) != uint32_t(want)) e = zst::E_CHECKSUM;
            S.pos += 4;
          }
        }
        S.err = uint32_t(e);
      }
      __syncthreads();
      if (S.err) break;
    }
    __syncthreads();
    if (lane == 0 && (S.err || S.op != n_out)) atomicMax(error, ~(first + job));
  }
}

}  // namespace dev

uint64_t zstd_scratch_bytes(uint32_t npages) {
  const uint32_t wgs = npages < ZSTD_MAX_WORKGROUPS ? npages : ZSTD_MAX_WORKGROUPS;
  return 256 + uint64_t(wgs) * ZSTD_SLAB_BYTES;
}

void launch_zstd(const InflatePage* pages, uint32_t npages, uint32_t first, uint32_t* error, uint8_t* scratch,
                 hipStream_t st) {
  if (!npages) return;
  const uint32_t wgs = npages < ZSTD_MAX_WORKGROUPS ? npages : ZSTD_MAX_WORKGROUPS;
  if (hipMemsetAsync(scratch, 0, 256, st) != hipSuccess) throw std::runtime_error("k_zstd: hipMemsetAsync failed");
  DR_LAUNCH(dev::k_zstd, dim3(wgs), dim3(64), 0, st, pages, npages, first, error, reinterpret_cast<uint32_t*>(scratch),
            scratch + 256);
}

}  // namespace dr
