// Selected-rows export (dr_state_export_rows): rows of one side picked by their export positions, in
// the caller's order (any order, duplicates allowed). A side whose columns are not resident is walked
// by k_export over the composed action list (k_rows_compose); a resident side is gathered from its
// columns here -- the scalars and the per-row counts by k_rows_row, the map entries' sources by
// k_rows_entries -- and every string moves through k_gather_bytes (k_util.hip).
#include "dev_common.h"
#include "kernels.h"
#include <algorithm>

namespace dr {
namespace dev {

// sel[i] = side[rows[i]]: the action indices k_export walks (rows validated by the host).
__global__ void __launch_bounds__(256) k_rows_compose(const uint32_t* __restrict__ side, const int64_t* __restrict__ rows,
                                                      uint64_t n, uint32_t* __restrict__ sel) {
  for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += uint64_t(gridDim.x) * blockDim.x)
    sel[i] = side[rows[i]];
}

// One lane per selected row: the scalar columns, the lengths of the row's path and stats with their
// sources, and its partitionValues / tags entry counts (scanned by the host into the output offsets).
__global__ void __launch_bounds__(256) k_rows_row(RowsArgs a) {
  for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < a.n; i += uint64_t(gridDim.x) * blockDim.x) {
    const uint64_t r = uint64_t(a.rows[i]);
    a.o_size[i] = a.size[r];
    a.o_mtime[i] = a.mtime[r];
    a.o_delts[i] = a.delts[r];
    a.o_flags[i] = a.flags[r];
    a.o_efm[i] = a.efm[r];
    a.o_stats_null[i] = a.stats_null[r];
    a.o_pv_null[i] = a.pv_null[r];
    a.o_tags_null[i] = a.tags_null[r];
    const uint64_t p0 = a.path_off[r], s0 = a.stats_off[r];
    a.path_src[i] = reinterpret_cast<uint64_t>(a.path_bytes + p0);
    a.path_len[i] = uint32_t(a.path_off[r + 1] - p0);
    a.stats_src[i] = reinterpret_cast<uint64_t>(a.stats_bytes + s0);
    a.stats_len[i] = uint32_t(a.stats_off[r + 1] - s0);
    a.pv_n[i] = uint32_t(a.pv_entry[r + 1] - a.pv_entry[r]);
    a.tags_n[i] = uint32_t(a.tags_entry[r + 1] - a.tags_entry[r]);
  }
}

// ROWS_G lanes per selected row walk the row's entries of one map (config 4: 4 entries a row, so a
// wave per row would idle 60 lanes): entry e of row rows[i] lands in output slot out_entry[i] + e with
// its key / value source and length and its value-null byte.
constexpr uint32_t ROWS_G = 4;
__global__ void __launch_bounds__(256) k_rows_entries(RowsMapArgs a) {
  const uint32_t gl = threadIdx.x % ROWS_G;
  const uint64_t step = uint64_t(gridDim.x) * (blockDim.x / ROWS_G);
  for (uint64_t i = (uint64_t(blockIdx.x) * blockDim.x + threadIdx.x) / ROWS_G; i < a.n; i += step) {
    const uint64_t r = uint64_t(a.rows[i]);
    const uint64_t s0 = a.entry[r], cnt = a.entry[r + 1] - s0, o0 = a.out_entry[i];
    for (uint64_t e = gl; e < cnt; e += ROWS_G) {
      const uint64_t s = s0 + e, o = o0 + e;
      const int64_t k0 = a.key_off[s], v0 = a.val_off[s];
      a.ksrc[o] = reinterpret_cast<uint64_t>(a.key_bytes + k0);
      a.klen[o] = uint32_t(a.key_off[s + 1] - k0);
      a.vsrc[o] = reinterpret_cast<uint64_t>(a.val_bytes + v0);
      a.vlen[o] = uint32_t(a.val_off[s + 1] - v0);
      a.o_val_null[o] = a.val_null[s];
    }
  }
}

}  // namespace dev

static dim3 rows_grid(uint64_t items) { return dim3(unsigned(std::min<uint64_t>((items + 255) / 256, 1u << 16))); }

void launch_rows_compose(const uint32_t* side, const int64_t* rows, uint64_t n, uint32_t* sel, hipStream_t st) {
  if (n) DR_LAUNCH(dev::k_rows_compose, rows_grid(n), dim3(256), 0, st, side, rows, n, sel);
}

void launch_rows_row(const RowsArgs& a, hipStream_t st) {
  if (a.n) DR_LAUNCH(dev::k_rows_row, rows_grid(a.n), dim3(256), 0, st, a);
}

void launch_rows_entries(const RowsMapArgs& a, hipStream_t st) {
  if (a.n) DR_LAUNCH(dev::k_rows_entries, rows_grid(a.n * dev::ROWS_G), dim3(256), 0, st, a);
}

}  // namespace dr
