// Path lookup (dr_state_lookup_paths): is a given path in a resident state, and at which export
// position? The reference answers this with a host map over the whole of allFiles
// (DeltaCommand.generateCandidateFileMap / getTouchedFile, D/commands/DeltaCommand.scala:96-104,159-168),
// a left-anti join against it (VacuumCommand, D/commands/VacuumCommand.scala:185-206) or a set of the
// removed paths (OptimisticTransaction.checkForConflicts, D/OptimisticTransaction.scala:829-833). Here
// every state can carry an index {replay key -> (side, export position)} over its own survivor lists,
// and a batch of query paths is canonicalised, keyed and probed on the device with the replay's own
// definitions (canon.h, dev_common.h): a query hits exactly the winner the replay would have replaced
// with it.
//
// Exactness does not rest on the 64-bit key. The build never deduplicates -- every survivor claims an
// empty slot of its own, so two survivors that share a key sit in one run -- and a probe walks its run
// to the first empty slot, comparing the bytes (key_equal) of every slot whose key matches.
#include "dev_common.h"
#include "kernels.h"
#include "canon.h"
#include <algorithm>

namespace dr {
namespace dev {

__device__ __forceinline__ unsigned long long lookup_key(uint64_t key, uint64_t key_mask) {
  const uint64_t k = key & key_mask;
  return k ? k : 1;  // 0 marks an empty slot
}

// A device address kept as an integer (ActionArrays::path_ptr), as a pointer the compiler knows to be
// global: the winner's bytes are then read with global loads, not flat ones.
__device__ __forceinline__ const uint8_t* global_bytes(uint64_t addr) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (const uint8_t*)(const __attribute__((address_space(1))) uint8_t*)(addr);
#else
  return reinterpret_cast<const uint8_t*>(addr);
#endif
}

// One lane per survivor of either list: row r of side s claims the first empty slot at or after its
// key's home with a compare-and-swap against 0 (so a slot is never taken twice, and an equal key
// already there is walked past, not merged), then writes (s, r) beside it. The probe runs in a later
// kernel, so the value needs no ordering with the key.
__global__ void __launch_bounds__(256) k_lookup_build(LookupIndexArgs a) {
  const uint64_t n = a.n_live + a.n_tomb;
  for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += uint64_t(gridDim.x) * blockDim.x) {
    const bool t = i >= a.n_live;
    const uint64_t r = t ? i - a.n_live : i;
    const uint32_t x = t ? a.tomb[r] : a.live[r];
    const unsigned long long k = lookup_key(a.key[x], a.key_mask);
    uint64_t s = k & a.cap_mask;
    // (a stale 0 only sends the lane to the compare-and-swap, which decides; slots never return to 0)
    while (a.keys[s] != 0 || atomicCAS(a.keys + s, 0ull, k) != 0) s = (s + 1) & a.cap_mask;
    a.vals[s] = uint32_t(r) | (t ? LOOKUP_TOMB : 0u);
  }
}

// One lane per query: its bytes -> canonical form and key (special queries through their share of the
// arena, every other query is its own canonical form) -> the run of its key -> the bytes of each
// candidate's winner. The chain slot -> survivor list -> path address / length -> path bytes is four
// dependent loads per candidate; the other waves of the CU cover them.
__global__ void __launch_bounds__(256) k_lookup_probe(LookupProbeArgs a) {
  const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const int64_t o0 = a.off[0], o = a.off[i];
  const uint64_t b = uint64_t(o - o0);
  uint32_t m = uint32_t(a.off[i + 1] - o);
  const uint8_t* q = a.blob + b;
  uint64_t key;
  if (path_is_special(q, m)) {
    uint8_t* out = a.arena + 2 * b + 32 * i;  // 2 * (m + 8) + 16 bytes are this query's
    for (uint32_t k = 0; k < m; ++k) out[7 + k] = q[k];
    uint8_t* res;
    key = canon_bytes(out, m, res);
    q = res;
  } else {
    key = path_key(q, m);
  }
  const unsigned long long k = lookup_key(key, a.ix.key_mask);
  uint8_t hit = 0;
  int64_t row = -1;
  for (uint64_t s = k & a.ix.cap_mask;; s = (s + 1) & a.ix.cap_mask) {
    const unsigned long long x = a.ix.keys[s];
    if (x == 0) break;  // load <= 1/2: every run ends
    if (x != k) continue;
    const uint32_t v = a.ix.vals[s];
    const uint32_t r = v & ~LOOKUP_TOMB;
    const uint32_t w = (v & LOOKUP_TOMB) ? a.ix.tomb[r] : a.ix.live[r];
    if (key_equal(q, m, global_bytes(a.path_ptr[w]), a.path_len[w])) {
      hit = (v & LOOKUP_TOMB) ? 2 : 1;
      row = int64_t(r);
      break;
    }
  }
  a.hit[i] = hit;
  a.row[i] = row;
}

}  // namespace dev

void launch_lookup_build(const LookupIndexArgs& a, hipStream_t st) {
  const uint64_t n = a.n_live + a.n_tomb;
  if (n) DR_LAUNCH(dev::k_lookup_build, dim3(unsigned(std::min<uint64_t>((n + 255) / 256, 1u << 16))), dim3(256), 0, st, a);
}

void launch_lookup_probe(const LookupProbeArgs& a, hipStream_t st) {
  if (a.n) DR_LAUNCH(dev::k_lookup_probe, dim3(unsigned((a.n + 255) / 256)), dim3(256), 0, st, a);
}

}  // namespace dr
