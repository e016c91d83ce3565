// Key probe (dr_state_probe_keys): which files of a selection can hold any key of a set, and how many
// files each key can lie in. The reference answers it with a join of the source against the whole target
// (MergeIntoCommand.findTouchedFiles, D/commands/MergeIntoCommand.scala:310); over the typed K5 cache it is
// a range-against-set test per file: lower_bound(lo) and upper_bound(hi) over the distinct sorted keys.
//
// Keys: k_probe_keys_prepare turns each non-NULL key into its order key (filter_plan.h probe_order_key, the
// function the bounds go through as well) beside its caller index; hipcub's radix sort orders the pairs;
// run heads, a scan and k_probe_key_compact leave the distinct keys and a caller-index -> slot map.
//
// Files: k_probe_files, one lane per selection position. The search has two levels: the workgroup stages
// the first key of every segment of `seg` keys in LDS (at most PROBE_TAB entries), bisects that table, and
// finishes inside the one segment the table brackets, in global memory. While the keys fit the table
// (seg == 1) no search leaves LDS. k_probe_files_plain bisects global memory only (the comparison variant).
// A known hit adds 1 to start[a] and to end[b] (probe_count: one add per run of lanes at the same counter):
// integer atomics, so their sums do not depend on the order of arrival, and k_probe_key_files reads a
// key's file count off the two inclusive scans.
#include "dev_common.h"
#include "kernels.h"
#include "../../include/deltareplay.h"
#include <hipcub/device/device_radix_sort.hpp>
#include <algorithm>
#include <stdexcept>

namespace dr {
namespace dev {

__global__ void __launch_bounds__(PROBE_BLOCK) k_probe_key_flags(const uint8_t* key_null, uint64_t n, uint32_t* flag) {
  const uint64_t i = uint64_t(blockIdx.x) * PROBE_BLOCK + threadIdx.x;
  if (i < n) flag[i] = key_null[i] ? 0u : 1u;
}

__global__ void __launch_bounds__(PROBE_BLOCK) k_probe_keys_prepare(const int64_t* keys, const uint8_t* key_null,
                                                                     const uint64_t* pos, uint64_t n, int32_t base,
                                                                     int64_t* enc, uint32_t* idx) {
  const uint64_t i = uint64_t(blockIdx.x) * PROBE_BLOCK + threadIdx.x;
  if (i >= n) return;
  if (key_null && key_null[i]) return;
  const uint64_t o = pos ? pos[i] : i;  // o <= i: within the n entries of enc / idx
  enc[o] = probe_order_key(base, keys[i]);
  idx[o] = uint32_t(i);
}

__global__ void __launch_bounds__(PROBE_BLOCK) k_probe_key_heads(const int64_t* sorted, uint64_t m, uint32_t* head) {
  const uint64_t j = uint64_t(blockIdx.x) * PROBE_BLOCK + threadIdx.x;
  if (j < m) head[j] = (j == 0 || sorted[j] != sorted[j - 1]) ? 1u : 0u;
}

__global__ void __launch_bounds__(PROBE_BLOCK) k_probe_key_compact(const int64_t* sorted, const uint32_t* idx,
                                                                    const uint32_t* head, const uint64_t* hpos, uint64_t m,
                                                                    int64_t* dkeys, uint32_t* slot_of) {
  const uint64_t j = uint64_t(blockIdx.x) * PROBE_BLOCK + threadIdx.x;
  if (j >= m) return;
  // heads up to and including j, less one: the slot of j's run (hpos[j] + head[j] >= 1, as head[0] == 1)
  const uint64_t slot = hpos[j] + head[j] - 1;
  if (head[j]) dkeys[slot] = sorted[j];
  slot_of[idx[j]] = uint32_t(slot);  // idx[j] < nkeys, the map's size
}

// The first index in [lo, hi) whose key is not before x (UPPER: before means <=, else <); hi when every
// key is. Reads keys[lo .. hi) only.
template <bool UPPER, class Keys>
__device__ __forceinline__ uint32_t probe_bisect(Keys keys, uint32_t lo, uint32_t hi, int64_t x) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const int64_t k = keys[mid];
    if (UPPER ? k <= x : k < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// How many distinct keys are before x. Two levels: c = the segments whose first key is before x; the
// answer lies behind the first key of segment c - 1 and not behind the end of that segment.
template <bool LDS, bool UPPER>
__device__ __forceinline__ uint32_t probe_search(const ProbeArgs& a, const int64_t* tab, int64_t x) {
  if (!LDS) return probe_bisect<UPPER>(a.dkeys, 0u, a.ndist, x);
  const uint32_t c = probe_bisect<UPPER>(tab, 0u, a.ntab, x);
  if (c == 0) return 0;
  const uint32_t s = c - 1;  // s * seg < ndist, and (s + 1) * seg < ndist + seg: no 32-bit overflow (ndist < 2^31)
  const uint32_t gl = s * a.seg + 1, ge = (s + 1) * a.seg;
  return probe_bisect<UPPER>(a.dkeys, gl, ge < a.ndist ? ge : a.ndist, x);
}

__device__ __forceinline__ int64_t probe_bound(const ProbeArgs& a, const void* v, uint64_t row) {
  const int64_t w = a.wide ? static_cast<const int64_t*>(v)[row]
                           : a.base == DR_T_FLOAT ? int64_t(static_cast<const uint32_t*>(v)[row])
                                                  : int64_t(int32_t(static_cast<const uint32_t*>(v)[row]));
  return probe_order_key(a.base, w);
}

// ctr[slot] += 1 for every lane with `has`, as one add per run of neighbouring lanes that share a slot: a
// selection in the table's order puts whole waves on one counter, and an add per lane then queues at
// that one address. A lane that has left the loop takes no part in the ballots and so ends a run; the
// sums are what an add per lane gives. Call from where every lane still in the loop arrives.
__device__ __forceinline__ void probe_count(uint32_t* ctr, bool has, uint32_t slot) {
  const uint32_t lane = threadIdx.x & 63u;  // PROBE_BLOCK is a multiple of the wave's 64 lanes
  const uint32_t prev = __shfl_up(slot, 1, 64);  // read only where the lane below takes part (`in`)
  const unsigned long long in = __ballot(has);
  const bool head = has && (lane == 0 || !((in >> (lane - 1)) & 1ull) || prev != slot);
  const unsigned long long stop = __ballot(head) | ~in;  // the lanes a run cannot reach into
  if (head) {
    const unsigned long long above = lane == 63 ? 0ull : stop >> (lane + 1);
    atomicAdd(&ctr[slot], above ? uint32_t(__ffsll(above)) : 64u - lane);  // the run's length, 1..64
  }
}

template <bool LDS>
__device__ __forceinline__ void probe_files(const ProbeArgs& a, int64_t* tab) {
  if (LDS) {
    for (uint32_t t = threadIdx.x; t < a.ntab; t += PROBE_BLOCK) tab[t] = a.dkeys[uint64_t(t) * a.seg];  // t * seg < ndist
    __syncthreads();
  }
  const uint64_t stride = uint64_t(gridDim.x) * PROBE_BLOCK;
  for (uint64_t p = uint64_t(blockIdx.x) * PROBE_BLOCK + threadIdx.x; p < a.n; p += stride) {
    const uint64_t row = a.rows ? uint64_t(a.rows[p]) : p;  // the host checked rows[p] against the side
    const bool lo_n = a.lo_null[row] != 0, hi_n = a.hi_null[row] != 0;
    int64_t h = 0;
    uint32_t first = 0, last = 0;
    if ((lo_n && a.lo_stats) || (hi_n && a.hi_stats)) {
      h = -1;  // a missing statistic: the file cannot be skipped
    } else if (!lo_n && !hi_n) {
      const int64_t lo = probe_bound(a, a.lo_v, row), hi = probe_bound(a, a.hi_v, row);
      if (lo <= hi) {
        first = probe_search<LDS, false>(a, tab, lo);
        last = probe_search<LDS, true>(a, tab, hi);
        if (last > first) h = int64_t(last - first);
      }
    }
    probe_count(a.start, h > 0, first);  // first < last <= ndist: within the ndist + 1 counters
    probe_count(a.end, h > 0, last);
    a.hits[p] = h;
    a.flag[p] = h != 0 ? 1u : 0u;
  }
}

__global__ void __launch_bounds__(PROBE_BLOCK) k_probe_files(ProbeArgs a) {
  __shared__ int64_t tab[PROBE_TAB];
  probe_files<true>(a, tab);
}

__global__ void __launch_bounds__(PROBE_BLOCK) k_probe_files_plain(ProbeArgs a) { probe_files<false>(a, nullptr); }

__global__ void __launch_bounds__(PROBE_BLOCK) k_probe_select(ProbeArgs a, const uint64_t* pos, int64_t* sel, int64_t* sel_hits) {
  const uint64_t p = uint64_t(blockIdx.x) * PROBE_BLOCK + threadIdx.x;
  if (p >= a.n || !a.flag[p]) return;
  const uint64_t o = pos[p];  // below the scan's total, the size of sel / sel_hits
  sel[o] = a.rows ? a.rows[p] : int64_t(p);
  sel_hits[o] = a.hits[p];
}

__global__ void __launch_bounds__(PROBE_BLOCK) k_probe_key_files(const uint32_t* slot_of, const uint64_t* s_scan,
                                                                  const uint64_t* e_scan, uint64_t nkeys, int64_t* key_files) {
  const uint64_t i = uint64_t(blockIdx.x) * PROBE_BLOCK + threadIdx.x;
  if (i >= nkeys) return;
  const uint32_t slot = slot_of[i];
  key_files[i] = slot == PROBE_NO_SLOT ? 0 : int64_t(s_scan[uint64_t(slot) + 1] - e_scan[uint64_t(slot) + 1]);
}

}  // namespace dev

static dim3 probe_grid(uint64_t n) { return dim3(uint32_t((n + PROBE_BLOCK - 1) / PROBE_BLOCK)); }

void launch_probe_key_flags(const uint8_t* key_null, uint64_t n, uint32_t* flag, hipStream_t st) {
  if (n) DR_LAUNCH(dev::k_probe_key_flags, probe_grid(n), dim3(PROBE_BLOCK), 0, st, key_null, n, flag);
}

void launch_probe_keys_prepare(const int64_t* keys, const uint8_t* key_null, const uint64_t* pos, uint64_t n, int32_t base,
                               int64_t* enc, uint32_t* idx, hipStream_t st) {
  if (n) DR_LAUNCH(dev::k_probe_keys_prepare, probe_grid(n), dim3(PROBE_BLOCK), 0, st, keys, key_null, pos, n, base, enc, idx);
}

void launch_probe_sort(void* temp, size_t* temp_bytes, const int64_t* k_in, int64_t* k_out, const uint32_t* v_in,
                       uint32_t* v_out, uint64_t m, hipStream_t st) {
  if (hipcub::DeviceRadixSort::SortPairs(temp, *temp_bytes, k_in, k_out, v_in, v_out, int(m), 0, 64, st) != hipSuccess)
    throw std::runtime_error("key probe radix sort failed");
}

void launch_probe_key_heads(const int64_t* sorted, uint64_t m, uint32_t* head, hipStream_t st) {
  if (m) DR_LAUNCH(dev::k_probe_key_heads, probe_grid(m), dim3(PROBE_BLOCK), 0, st, sorted, m, head);
}

void launch_probe_key_compact(const int64_t* sorted, const uint32_t* idx, const uint32_t* head, const uint64_t* hpos,
                              uint64_t m, int64_t* dkeys, uint32_t* slot_of, hipStream_t st) {
  if (m) DR_LAUNCH(dev::k_probe_key_compact, probe_grid(m), dim3(PROBE_BLOCK), 0, st, sorted, idx, head, hpos, m, dkeys, slot_of);
}

void launch_probe_files(const ProbeArgs& a, bool plain, hipStream_t st) {
  if (!a.n) return;
  const dim3 grid(uint32_t(std::min<uint64_t>((a.n + PROBE_BLOCK - 1) / PROBE_BLOCK, PROBE_GRID)));
  if (plain) DR_LAUNCH(dev::k_probe_files_plain, grid, dim3(PROBE_BLOCK), 0, st, a);
  else DR_LAUNCH(dev::k_probe_files, grid, dim3(PROBE_BLOCK), 0, st, a);
}

void launch_probe_select(const ProbeArgs& a, const uint64_t* pos, int64_t* sel, int64_t* sel_hits, hipStream_t st) {
  if (a.n) DR_LAUNCH(dev::k_probe_select, probe_grid(a.n), dim3(PROBE_BLOCK), 0, st, a, pos, sel, sel_hits);
}

void launch_probe_key_files(const uint32_t* slot_of, const uint64_t* s_scan, const uint64_t* e_scan, uint64_t nkeys,
                            int64_t* key_files, hipStream_t st) {
  if (nkeys) DR_LAUNCH(dev::k_probe_key_files, probe_grid(nkeys), dim3(PROBE_BLOCK), 0, st, slot_of, s_scan, e_scan, nkeys, key_files);
}

}  // namespace dr
