// K5: what the predicate planner (pred_plan.cpp, host only) and the evaluators (k_filter.hip) agree
// on -- limits, order keys, the leaf record and the plan's opcodes. No HIP type: g++ compiles it.
#pragma once
#include <cstdint>

namespace dr {

constexpr int PV_MAXC = 16;   // partition columns per predicate
constexpr int PV_STACK = 32;  // k_filter_typed's value stack (lowered program)
// what k_filter_leaf / k_filter_dict hold in LDS (more: k_filter_typed): program ops, leaves, 64-bit
// literal slots, string literals; FD_MAXTAB: the dictionary kernel's leaf-table bytes
constexpr int FL_MAXPROG = 128, FL_MAXLEAF = 64, FL_MAXI64 = 1024, FL_MAXSTR = 256;
constexpr uint32_t FD_MAXTAB = 32768;
constexpr int FL_UCOLS = 4;   // distinct columns a leaf program preloads per tile
constexpr int FL_MAXFN = 4;   // date functions a leaf applies to its column (a longer chain: k_filter_typed)

// Floating-point order keys (SQLOrderingUtil.compareDoubles / compareFloats: -0.0 = 0.0, NaN = NaN,
// NaN above +Infinity): the bits with every NaN canonical and -0.0 turned into +0.0, then the magnitude
// bits of negative values flipped, so the signed integer order of the keys is that order. The device
// applies them when it loads a FLOAT / DOUBLE cache value (the cache keeps the raw bits: the
// checkpoint writer reads them), the host to every literal (pred_plan.cpp). Each is its own inverse on
// canonical values.
#if defined(__HIPCC__)
#define DR_HD __host__ __device__
#else
#define DR_HD
#endif
DR_HD inline int64_t fp_key64(uint64_t bits) {
  if ((bits & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) bits = 0x7ff8000000000000ull;
  if (bits == 0x8000000000000000ull) bits = 0;
  const int64_t k = int64_t(bits);
  return k ^ ((k >> 63) & 0x7fffffffffffffffll);
}
DR_HD inline int64_t fp_key32(uint32_t bits) {
  if ((bits & 0x7fffffffu) > 0x7f800000u) bits = 0x7fc00000u;
  if (bits == 0x80000000u) bits = 0;
  const int32_t k = int32_t(bits);
  return int64_t(k ^ ((k >> 31) & 0x7fffffff));
}
// The 64-bit key of the binary32 value whose 32-bit key is `k32`: the value widened exactly to
// binary64 (a float column compared with a double literal), in integer arithmetic (subnormals
// included, whatever the denormal mode).
DR_HD inline int64_t fp_key_widen(int64_t k32) {
  const int32_t k = int32_t(k32);
  const uint32_t b = uint32_t(k ^ ((k >> 31) & 0x7fffffff));
  const uint64_t sign = uint64_t(b >> 31) << 63;
  int32_t e = int32_t((b >> 23) & 0xffu);
  uint32_t m = b & 0x7fffffu;
  uint64_t d;
  if (e == 255) {
    d = sign | 0x7ff0000000000000ull | (uint64_t(m) << 29);
  } else if (e == 0 && m == 0) {
    d = sign;
  } else {
    if (e == 0) {  // subnormal: normalise
      const int sh = __builtin_clz(m) - 8;
      m = (m << sh) & 0x7fffffu;
      e = 1 - sh;
    }
    d = sign | (uint64_t(e + 896) << 52) | (uint64_t(m) << 29);
  }
  return fp_key64(d);
}
// dr_state_probe_keys: a word in dr_state_stats_column's encoding (a caller's key, a bound widened from
// its cache column) as the int64 the probe sorts, de-duplicates and searches by. FLOAT (the low 32 bits)
// and DOUBLE go through their order keys, so -0.0 and 0.0 are one key and every NaN is the one value
// above +Infinity; every other supported type is a signed integer already. Host (tests) and device
// (k_probe.hip) both call this.
DR_HD inline int64_t probe_order_key(int32_t base, int64_t word) {
  if (base == 7 /* DR_T_FLOAT */) return fp_key32(uint32_t(uint64_t(word)));
  if (base == 8 /* DR_T_DOUBLE */) return fp_key64(uint64_t(word));
  return word;
}
// The kind a leaf evaluates a column as: BINARY as STRING (bytes), TIMESTAMP as LONG (one 64-bit
// integer); FLOAT / DOUBLE through their keys; DECIMAL as two words (w64 unsigned under w64hi).
DR_HD inline int32_t leaf_kind(int32_t type) {
  const int32_t b = type & 0xff;
  return b == 10 /* DR_T_BINARY */ ? 0 /* DR_T_STRING */ : b == 9 /* DR_T_TIMESTAMP */ ? 4 /* DR_T_LONG */ : b;
}

// Leaf form of a predicate (pred_plan.cpp leafify): every leaf compares one partition column with
// literals -- col op lit, col IN (lits), col IS [NOT] NULL, the column possibly under a chain of date
// functions -- and AND / OR / NOT combine their
// three-valued results on a 2-bit-per-entry stack held in one register.
struct FilterLeaf {
  int32_t col;       // predicate column
  int32_t op;        // DR_OP_EQ .. DR_OP_GE, DR_OP_NSEQ, DR_OP_IN, DR_OP_ISNULL, DR_OP_ISNOTNULL,
                     // DR_OP_STARTSWITH .. DR_OP_LIKE (literal `lit`: the needle / like_lane.h's program)
  int32_t lit;       // literal index (comparisons) or first entry of the sorted set (IN)
  int32_t nlit;      // IN: entries in the set
  int32_t lit_null;  // comparisons: the literal is NULL; IN: the list holds a NULL
  int32_t pad;       // IN over integers: 1 = a bitmap (literals [min, words, bits...]); a FLOAT column
                     // against DOUBLE literals: 2 = widen the value's key (fp_key_widen) first
  int32_t slot;      // k_filter_leaf: the preloaded column slot holding `col` (-1: loaded per leaf)
  int32_t ctype;     // leaf_kind of the column's dr_pred_type
  // a function leaf, f(col) op literals: the date functions (date_fn.h) applied to the column's value,
  // innermost first, before the comparison; the literal slots then hold plain integers. An aggregate
  // initialiser that stops before these reads as "no function".
  int32_t nfn;               // 0 .. FL_MAXFN
  int32_t fn[FL_MAXFN], farg[FL_MAXFN];  // DR_OP_YEAR .. DR_OP_TRUNC_DATE and the op's arg
};
enum : int32_t { LEAF_OP_LEAF = 0, LEAF_OP_AND = 1, LEAF_OP_OR = 2, LEAF_OP_NOT = 3 };
// device-only opcodes of the lowered program (pred_plan.cpp lower_program): an IN list is folded
// one element at a time into an accumulator slot above its value
enum : int32_t { FILTER_OP_IN_START = 100, FILTER_OP_IN_STEP = 101, FILTER_OP_IN_END = 102 };

}  // namespace dr
