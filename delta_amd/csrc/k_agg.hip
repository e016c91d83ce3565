// Metadata-only aggregates (dr_state_aggregate): COUNT / MIN / MAX / SUM of typed K5 cache columns, size
// and modificationTime over a selection of the live side, per group. What the reference leaves null in
// DeltaScan(version, files, null, null, null) (D/PartitionFiltering.scala:41, D/stats/DeltaScan.scala:29-52)
// and what a metadata-only count(*) / min / max query reads, answered without exporting a column.
//
// Two kernels. k_agg_tiles: one workgroup per AGG_TILE selection positions loads rows[p] once, then for
// every spec the value and null flag of that row, and reduces by group -- wave shuffles, then the
// workgroup's waves through LDS; a tile that holds group boundaries runs the segmented form of the same
// scan (heads from group_off, found by bisection from the tile's first position). A group that lies
// within the tile is written to the results; a group that goes on beyond the tile leaves one partial
// per tile, which k_agg_combine folds (the workgroup of the tile the group starts in).
//
// Every reduction is over (count, value, selection position) with one combine per class: SUM adds 128
// bits with the carry in registers; MIN / MAX keep the better order key and, between keys equal under
// the order, the smaller selection position. Both are associative and commutative, so the result does
// not depend on how the selection was cut or in which order workgroups ran -- no global atomics. The
// value returned for MIN / MAX is re-read from the winner's row (its own bits, not its order key).
#include "dev_common.h"
#include "kernels.h"
#include "../../include/deltareplay.h"
#include <algorithm>

namespace dr {
namespace dev {

// the combine classes (a template parameter: the shuffle loops hold no per-spec branch)
constexpr int CK_SUM = 0;  // COUNT and SUM: counts and 128-bit sums
constexpr int CK_NUM = 1;  // MIN / MAX over a 128-bit order key (hi signed, lo unsigned)
constexpr int CK_STR = 2;  // MIN / MAX over bytes (an argmin over rows)

__device__ __forceinline__ int agg_class(const AggSpec& s) {
  return (s.fn == DR_AGG_COUNT || s.fn == DR_AGG_SUM) ? CK_SUM : s.kind == AGK_STR ? CK_STR : CK_NUM;
}

__device__ __forceinline__ const uint8_t* agg_bytes(uint64_t addr) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (const uint8_t*)(const __attribute__((address_space(1))) uint8_t*)(addr);
#else
  return reinterpret_cast<const uint8_t*>(addr);
#endif
}

__device__ __forceinline__ AggAcc acc_identity() { return AggAcc{0, 0, 0, -1}; }

__device__ __forceinline__ AggAcc acc_shfl_xor(const AggAcc& a, int m) {
  AggAcc r;
  r.nn = __shfl_xor((long long)a.nn, m, 64);
  r.lo = __shfl_xor((long long)a.lo, m, 64);
  r.hi = __shfl_xor((long long)a.hi, m, 64);
  r.pos = __shfl_xor((long long)a.pos, m, 64);
  return r;
}
__device__ __forceinline__ AggAcc acc_shfl_up(const AggAcc& a, unsigned d) {
  AggAcc r;
  r.nn = __shfl_up((long long)a.nn, d, 64);
  r.lo = __shfl_up((long long)a.lo, d, 64);
  r.hi = __shfl_up((long long)a.hi, d, 64);
  r.pos = __shfl_up((long long)a.pos, d, 64);
  return r;
}

// < 0: a orders before b; 0: equal under the order. STRING / BINARY: unsigned bytes, a proper prefix
// first -- the first 8 bytes (s8, big-endian, zero-padded) decide most pairs without a gather.
template <int K>
__device__ __forceinline__ int acc_cmp(const AggSpec& s, const AggAcc& a, const AggAcc& b) {
  if (K == CK_NUM) {
    if (a.hi != b.hi) return a.hi < b.hi ? -1 : 1;
    if (a.lo != b.lo) return uint64_t(a.lo) < uint64_t(b.lo) ? -1 : 1;
    return 0;
  }
  if (a.lo != b.lo) return uint64_t(a.lo) < uint64_t(b.lo) ? -1 : 1;
  if (a.hi == b.hi) return 0;  // the same row
  const uint32_t la = s.slen[a.hi], lb = s.slen[b.hi], m = la < lb ? la : lb;
  const uint8_t* pa = agg_bytes(s.sptr[a.hi]);
  const uint8_t* pb = agg_bytes(s.sptr[b.hi]);
  for (uint32_t i = 0; i < m; ++i)
    if (pa[i] != pb[i]) return pa[i] < pb[i] ? -1 : 1;
  return la < lb ? -1 : la > lb ? 1 : 0;
}

template <int K>
__device__ __forceinline__ AggAcc acc_combine(const AggSpec& s, const AggAcc& a, const AggAcc& b) {
  AggAcc r;
  if (K == CK_SUM) {
    const uint64_t lo = uint64_t(a.lo) + uint64_t(b.lo);
    r.nn = a.nn + b.nn;
    r.lo = int64_t(lo);
    r.hi = int64_t(uint64_t(a.hi) + uint64_t(b.hi) + (lo < uint64_t(a.lo) ? 1u : 0u));
    r.pos = -1;
    return r;
  }
  bool take_b;
  if (b.pos < 0) {
    take_b = false;
  } else if (a.pos < 0) {
    take_b = true;
  } else {
    int c = acc_cmp<K>(s, a, b);
    if (s.fn == DR_AGG_MAX) c = -c;
    take_b = c > 0 || (c == 0 && b.pos < a.pos);
  }
  // (field by field: a select between the two structs would go through their addresses, in scratch)
  r.nn = a.nn + b.nn;
  r.lo = take_b ? b.lo : a.lo;
  r.hi = take_b ? b.hi : a.hi;
  r.pos = take_b ? b.pos : a.pos;
  return r;
}

// Row `row`'s input of spec s as a reduction element; the identity for a NULL.
template <int K>
__device__ __forceinline__ AggAcc agg_load(const AggSpec& s, uint64_t row, int64_t pos) {
  AggAcc e = acc_identity();
  if (s.isnull && s.isnull[row]) return e;
  e.nn = 1;
  if (K == CK_STR) {
    e.lo = int64_t(static_cast<const uint64_t*>(s.v)[row]);
    e.hi = int64_t(row);
    e.pos = pos;
    return e;
  }
  switch (s.kind) {
    case AGK_I32: e.lo = int64_t(int32_t(static_cast<const uint32_t*>(s.v)[row])); break;
    case AGK_F32: e.lo = fp_key32(static_cast<const uint32_t*>(s.v)[row]); break;
    case AGK_I64: e.lo = static_cast<const int64_t*>(s.v)[row]; break;
    case AGK_F64: e.lo = fp_key64(uint64_t(static_cast<const int64_t*>(s.v)[row])); break;
    case AGK_DEC: e.lo = static_cast<const int64_t*>(s.v)[row]; break;
    default: break;  // AGK_ZERO: COUNT
  }
  e.hi = s.kind == AGK_DEC ? s.hi[row] : e.lo >> 63;
  if (K == CK_NUM) e.pos = pos;
  return e;
}

// Cell (ai, g) of the results. MIN / MAX: the winner's row and that row's own bits.
__device__ __forceinline__ void agg_write(const AggArgs& a, int32_t ai, uint64_t g, const AggAcc& r) {
  const AggSpec& s = a.spec[ai];
  const uint64_t cell = uint64_t(ai) * a.ngroups + g;
  a.nonnull[cell] = r.nn;
  if (s.fn == DR_AGG_COUNT || s.fn == DR_AGG_SUM) {
    a.value_lo[cell] = r.lo;
    a.value_hi[cell] = r.hi;
    return;
  }
  if (r.pos < 0) return;  // no non-NULL input: the zeroed cell and arg_row = -1 stand
  const uint64_t row = a.rows ? uint64_t(a.rows[r.pos]) : uint64_t(r.pos);
  a.arg_row[cell] = int64_t(row);
  int64_t lo = 0, hi = 0;
  switch (s.kind) {
    case AGK_I32: lo = int64_t(int32_t(static_cast<const uint32_t*>(s.v)[row])); hi = lo >> 63; break;
    case AGK_F32: lo = int64_t(static_cast<const uint32_t*>(s.v)[row]); break;
    case AGK_I64: lo = static_cast<const int64_t*>(s.v)[row]; hi = lo >> 63; break;
    case AGK_F64: lo = static_cast<const int64_t*>(s.v)[row]; break;
    case AGK_DEC: lo = static_cast<const int64_t*>(s.v)[row]; hi = s.hi[row]; break;
    default: break;  // AGK_STR: the bytes follow (k_agg_str_copy)
  }
  a.value_lo[cell] = lo;
  a.value_hi[cell] = hi;
}

// The group that holds selection position p, among groups [lo, hi] (group_off[lo] <= p and
// group_off[hi + 1] > p): the g with group_off[g] <= p < group_off[g + 1], whatever empty groups
// share its offsets.
__device__ __forceinline__ uint64_t group_of(const int64_t* off, uint64_t lo, uint64_t hi, uint64_t p) {
  uint64_t a = lo + 1, b = hi + 1;  // the first j with group_off[j] > p is in [a, b]
  while (a < b) {
    const uint64_t m = a + (b - a) / 2;
    if (uint64_t(off[m]) > p) b = m;
    else a = m + 1;
  }
  return a - 1;
}

template <int K>
__device__ __forceinline__ AggAcc wave_reduce(const AggSpec& s, AggAcc v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const AggAcc u = acc_shfl_xor(v, m);
    v = acc_combine<K>(s, v, u);
  }
  return v;
}

// The workgroup's fold of one value per thread, in thread 0 (sh: one slot per wave; free again on return).
template <int K>
__device__ __forceinline__ AggAcc block_reduce(const AggSpec& s, AggAcc v, AggAcc* sh) {
  v = wave_reduce<K>(s, v);
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  if (lane == 0) sh[w] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    for (uint32_t k = 1; k < AGG_BLOCK / 64; ++k) v = acc_combine<K>(s, v, sh[k]);
  __syncthreads();
  return v;
}

// Where a tile's reduction of group g goes: the results when [gs, ge) lies within the tile [p0, p1),
// else the tile's partial -- slot 0 for the segment that holds p0, slot 1 for a later one (which then
// runs to the tile's end; a tile has at most these two open segments).
__device__ __forceinline__ void tile_emit(const AggArgs& a, int32_t ai, uint64_t tile, uint64_t p0, uint64_t p1, uint64_t g,
                                          const AggAcc& v) {
  const uint64_t gs = uint64_t(a.group_off[g]), ge = uint64_t(a.group_off[g + 1]);
  if (gs >= p0 && ge <= p1) agg_write(a, ai, g, v);
  else a.part[(tile * 2 + (gs <= p0 ? 0u : 1u)) * uint64_t(a.naggs) + uint64_t(ai)] = v;
}

constexpr int AGG_ROUNDS = int(AGG_TILE / AGG_BLOCK);

// A tile inside one group: a plain reduction.
template <int K>
__device__ __forceinline__ void tile_plain(const AggArgs& a, int32_t ai, const int64_t (&row)[AGG_ROUNDS], uint64_t tile,
                                           uint64_t p0, uint64_t p1, uint64_t g, AggAcc* sh) {
  const AggSpec& s = a.spec[ai];
  AggAcc acc = acc_identity();
#pragma unroll
  for (int r = 0; r < AGG_ROUNDS; ++r)
    if (row[r] >= 0) acc = acc_combine<K>(s, acc, agg_load<K>(s, uint64_t(row[r]), int64_t(p0 + uint64_t(r) * AGG_BLOCK + threadIdx.x)));
  acc = block_reduce<K>(s, acc, sh);
  if (threadIdx.x == 0) tile_emit(a, ai, tile, p0, p1, g, acc);
}

// A tile with group boundaries: per round of AGG_BLOCK positions a segmented inclusive scan in each
// wave (head flags restart it), then the carry of the waves and rounds before -- back to the nearest
// one that holds a head -- joins every lane in front of its wave's first head. The last lane of a
// segment holds the segment's reduction and emits it.
template <int K>
__device__ __forceinline__ void tile_segmented(const AggArgs& a, int32_t ai, const int64_t (&row)[AGG_ROUNDS],
                                               const uint64_t (&grp)[AGG_ROUNDS], uint32_t heads, uint32_t ends, uint64_t tile,
                                               uint64_t p0, uint64_t p1, AggAcc* sh_tail, uint32_t* sh_head, AggAcc* sh_round) {
  const AggSpec& s = a.spec[ai];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < AGG_ROUNDS; ++r) {
    if (p0 + uint64_t(r) * AGG_BLOCK >= p1) break;  // (the same in every thread)
    AggAcc v = row[r] >= 0 ? agg_load<K>(s, uint64_t(row[r]), int64_t(p0 + uint64_t(r) * AGG_BLOCK + threadIdx.x)) : acc_identity();
    uint32_t f = (heads >> r) & 1u;
#pragma unroll
    for (unsigned d = 1; d < 64; d <<= 1) {
      const AggAcc u = acc_shfl_up(v, d);
      const uint32_t fu = __shfl_up(f, d, 64);
      if (lane >= d) {
        if (!f) v = acc_combine<K>(s, u, v);
        f |= fu;
      }
    }
    if (lane == 63) {
      sh_tail[w] = v;
      sh_head[w] = f;
    }
    __syncthreads();
    if (!f) {  // in front of the wave's first head: the open segment of what came before continues here
      AggAcc carry = acc_identity();
      bool open = true;
      for (int k = int(w) - 1; k >= 0 && open; --k) {
        carry = acc_combine<K>(s, sh_tail[k], carry);
        open = sh_head[k] == 0;
      }
      if (open && r > 0) carry = acc_combine<K>(s, *sh_round, carry);
      v = acc_combine<K>(s, carry, v);
    }
    if (row[r] >= 0 && ((ends >> r) & 1u)) tile_emit(a, ai, tile, p0, p1, grp[r], v);
    __syncthreads();
    if (threadIdx.x == AGG_BLOCK - 1) *sh_round = v;  // read after the next round's barrier
  }
  __syncthreads();  // the next spec's first round writes sh_tail
}

__global__ void __launch_bounds__(AGG_BLOCK) k_agg_tiles(AggArgs a) {
  __shared__ AggAcc sh_tail[AGG_BLOCK / 64];
  __shared__ uint32_t sh_head[AGG_BLOCK / 64];
  __shared__ AggAcc sh_round;
  const uint64_t tile = blockIdx.x, p0 = tile * AGG_TILE, p1 = p0 + AGG_TILE < a.n ? p0 + AGG_TILE : a.n;
  if (p0 >= p1) return;
  const uint64_t g_first = group_of(a.group_off, 0, a.ngroups - 1, p0);
  const uint64_t g_last = group_of(a.group_off, g_first, a.ngroups - 1, p1 - 1);
  int64_t row[AGG_ROUNDS];
#pragma unroll
  for (int r = 0; r < AGG_ROUNDS; ++r) {
    const uint64_t p = p0 + uint64_t(r) * AGG_BLOCK + threadIdx.x;
    row[r] = p < p1 ? (a.rows ? a.rows[p] : int64_t(p)) : -1;
  }
  if (g_first == g_last) {
    for (int32_t ai = 0; ai < a.naggs; ++ai) {
      switch (agg_class(a.spec[ai])) {  // (wave-uniform: the spec, not the lane)
        case CK_SUM: tile_plain<CK_SUM>(a, ai, row, tile, p0, p1, g_first, sh_tail); break;
        case CK_NUM: tile_plain<CK_NUM>(a, ai, row, tile, p0, p1, g_first, sh_tail); break;
        default: tile_plain<CK_STR>(a, ai, row, tile, p0, p1, g_first, sh_tail); break;
      }
    }
    return;
  }
  // each position's group among the tile's, whether it starts its group and whether it ends its segment
  uint64_t grp[AGG_ROUNDS];
  uint32_t heads = 0, ends = 0;
#pragma unroll
  for (int r = 0; r < AGG_ROUNDS; ++r) {
    const uint64_t p = p0 + uint64_t(r) * AGG_BLOCK + threadIdx.x;
    grp[r] = g_first;
    if (p < p1) {
      grp[r] = group_of(a.group_off, g_first, g_last, p);
      if (uint64_t(a.group_off[grp[r]]) == p) heads |= 1u << r;
      if (uint64_t(a.group_off[grp[r] + 1]) == p + 1 || p + 1 == p1) ends |= 1u << r;
    }
  }
  for (int32_t ai = 0; ai < a.naggs; ++ai) {
    switch (agg_class(a.spec[ai])) {
      case CK_SUM: tile_segmented<CK_SUM>(a, ai, row, grp, heads, ends, tile, p0, p1, sh_tail, sh_head, &sh_round); break;
      case CK_NUM: tile_segmented<CK_NUM>(a, ai, row, grp, heads, ends, tile, p0, p1, sh_tail, sh_head, &sh_round); break;
      default: tile_segmented<CK_STR>(a, ai, row, grp, heads, ends, tile, p0, p1, sh_tail, sh_head, &sh_round); break;
    }
  }
}

// A group that goes on beyond the tile it starts in: that tile's workgroup folds the partials the
// group's tiles left, tile by tile across the threads (the starting tile's is its slot 1 when another
// segment holds the tile's first position, every later tile's its slot 0).
template <int K>
__device__ __forceinline__ void combine_group(const AggArgs& a, int32_t ai, uint64_t tile, uint64_t last_tile, bool first_slot1,
                                              uint64_t g, AggAcc* sh) {
  const AggSpec& s = a.spec[ai];
  AggAcc acc = acc_identity();
  for (uint64_t k = tile + threadIdx.x; k <= last_tile; k += AGG_BLOCK) {
    const uint64_t slot = (k == tile && first_slot1) ? 1u : 0u;
    acc = acc_combine<K>(s, acc, a.part[(k * 2 + slot) * uint64_t(a.naggs) + uint64_t(ai)]);
  }
  acc = block_reduce<K>(s, acc, sh);
  if (threadIdx.x == 0) agg_write(a, ai, g, acc);
}

__global__ void __launch_bounds__(AGG_BLOCK) k_agg_combine(AggArgs a) {
  __shared__ AggAcc sh[AGG_BLOCK / 64];
  const uint64_t tile = blockIdx.x, p0 = tile * AGG_TILE, p1 = p0 + AGG_TILE < a.n ? p0 + AGG_TILE : a.n;
  if (p0 >= p1) return;
  const uint64_t g = group_of(a.group_off, 0, a.ngroups - 1, p1 - 1);
  const uint64_t gs = uint64_t(a.group_off[g]), ge = uint64_t(a.group_off[g + 1]);
  if (ge <= p1 || gs < p0) return;  // ends here, or started in an earlier tile (which folds it)
  const uint64_t last_tile = (ge - 1) / AGG_TILE;
  // one workgroup per (tile, spec): a group over the whole selection is one workgroup's fold per spec,
  // and the specs' folds run side by side
  const int32_t ai = int32_t(blockIdx.y);
  switch (agg_class(a.spec[ai])) {
    case CK_SUM: combine_group<CK_SUM>(a, ai, tile, last_tile, gs > p0, g, sh); break;
    case CK_NUM: combine_group<CK_NUM>(a, ai, tile, last_tile, gs > p0, g, sh); break;
    default: combine_group<CK_STR>(a, ai, tile, last_tile, gs > p0, g, sh); break;
  }
}

__device__ __forceinline__ bool agg_str_cell(const AggArgs& a, uint64_t cell, uint64_t* row) {
  const AggSpec& s = a.spec[cell / a.ngroups];
  if (s.kind != AGK_STR || (s.fn != DR_AGG_MIN && s.fn != DR_AGG_MAX) || a.arg_row[cell] < 0) return false;
  *row = uint64_t(a.arg_row[cell]);
  return true;
}

__global__ void __launch_bounds__(256) k_agg_str_len(AggArgs a, uint32_t* len) {
  const uint64_t cell = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (cell >= uint64_t(a.naggs) * a.ngroups) return;
  uint64_t row;
  len[cell] = agg_str_cell(a, cell, &row) ? a.spec[cell / a.ngroups].slen[row] : 0u;
}

__global__ void __launch_bounds__(256) k_agg_str_copy(AggArgs a, const uint64_t* off, uint8_t* bytes) {
  const uint64_t cell = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (cell >= uint64_t(a.naggs) * a.ngroups) return;
  uint64_t row;
  if (!agg_str_cell(a, cell, &row)) return;
  const AggSpec& s = a.spec[cell / a.ngroups];
  const uint8_t* src = agg_bytes(s.sptr[row]);
  const uint32_t n = s.slen[row];
  for (uint32_t i = 0; i < n; ++i) bytes[off[cell] + i] = src[i];
}

}  // namespace dev

static uint32_t agg_tiles(uint64_t n) { return uint32_t((n + AGG_TILE - 1) / AGG_TILE); }

void launch_agg_tiles(const AggArgs& a, hipStream_t st) {
  if (!a.n || !a.naggs) return;
  DR_LAUNCH(dev::k_agg_tiles, dim3(agg_tiles(a.n)), dim3(AGG_BLOCK), 0, st, a);
}

void launch_agg_combine(const AggArgs& a, hipStream_t st) {
  if (!a.n || !a.naggs || a.n <= AGG_TILE) return;  // one tile: every group lies within it
  DR_LAUNCH(dev::k_agg_combine, dim3(agg_tiles(a.n), uint32_t(a.naggs)), dim3(AGG_BLOCK), 0, st, a);
}

void launch_agg_str_len(const AggArgs& a, uint32_t* len, hipStream_t st) {
  const uint64_t cells = uint64_t(a.naggs) * a.ngroups;
  if (!cells) return;
  DR_LAUNCH(dev::k_agg_str_len, dim3(uint32_t((cells + 255) / 256)), dim3(256), 0, st, a, len);
}

void launch_agg_str_copy(const AggArgs& a, const uint64_t* off, uint8_t* bytes, hipStream_t st) {
  const uint64_t cells = uint64_t(a.naggs) * a.ngroups;
  if (!cells) return;
  DR_LAUNCH(dev::k_agg_str_copy, dim3(uint32_t((cells + 255) / 256)), dim3(256), 0, st, a, off, bytes);
}

}  // namespace dr
