// Canonicalisation of one special path (D/Snapshot.scala:317-328), shared by k_canon, the
// small-segment tail kernel (k_json.hip:k_tail_post) and the path lookup (k_lookup.hip).
#pragma once
#include "dev_common.h"
#include "kernels.h"

namespace dr {
namespace dev {

// The canonical form and replay key of the m path bytes at out + 7 (JSON escapes already decoded);
// `out` has room for 2 * (m + 8) + 16 bytes. *res / m receive the canonical string (inside `out`), the
// key bytes (URI-equality form) are written behind it. Shared by the replay (canon_one) and the path
// lookup's queries (k_lookup.hip), so a query is keyed exactly as the action it asks for.
__device__ __forceinline__ uint64_t canon_bytes(uint8_t* out, uint32_t& m, uint8_t*& res) {
  uint8_t* body = out + 7;  // room for a "file://" prefix
  res = body;
  if (m > 0 && body[0] == '/') {
    // Hadoop Path normalisation ('//' collapse, no trailing '/'), then makeQualified on the local
    // filesystem: scheme "file", empty authority -> "file://" + path.
    uint32_t w = 0;
    for (uint32_t k = 0; k < m; ++k) {
      if (body[k] == '/' && w > 0 && body[w - 1] == '/') continue;
      body[w++] = body[k];
    }
    if (w > 1 && body[w - 1] == '/') --w;
    res = out;
    const char pre[7] = {'f', 'i', 'l', 'e', ':', '/', '/'};
    for (int k = 0; k < 7; ++k) out[k] = uint8_t(pre[k]);
    m = w + 7;
  }
  // key bytes (URI-equality form) for hashing, written after the output string
  uint8_t* kb = res + m + 8;
  const uint32_t sk = key_skip(res, m);
  uint32_t kn = 0;
  for (uint32_t k = 0; k < m; ++k) {
    if (sk && (k == 5 || k == 6)) continue;
    kb[kn++] = res[k];
  }
  return path_key(kb, kn);
}

__device__ __forceinline__ void canon_one(const CanonArgs& a, uint64_t i) {

  const uint8_t f = a.act.flags[i];
  if (!(f & F_SPECIAL_PATH)) return;
  const uint8_t* src = reinterpret_cast<const uint8_t*>(a.act.path_ptr[i]);
  const uint32_t n = a.act.path_len[i];
  const uint64_t need = 2ull * (n + 8) + 16;
  const unsigned long long at = atomicAdd(reinterpret_cast<unsigned long long*>(a.arena_fill), (unsigned long long)need);
  if (at + need > a.arena_cap) return;  // host sized the arena from the same counters
  uint8_t* out = a.arena + at;
  uint32_t m;
  uint8_t* body = out + 7;
  if (f & F_PATH_ESCAPED) m = json_unescape(src, n, body);
  else { for (uint32_t k = 0; k < n; ++k) body[k] = src[k]; m = n; }
  uint8_t* res;
  const uint64_t key = canon_bytes(out, m, res);
  a.act.path_ptr[i] = reinterpret_cast<uint64_t>(res);
  a.act.path_len[i] = m;
  if (a.act.path_ref) a.act.path_ref[i] = pack_ref(reinterpret_cast<uint64_t>(res), m);
  a.act.key[i] = key;
}

}  // namespace dev
}  // namespace dr
