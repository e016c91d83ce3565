// K5 predicate planner (pred_plan.cpp): everything between a caller's dr_predicate and the arrays the
// evaluators read. Host only and HIP-free, so it also builds and runs without a device
// (tests/native/pred_plan_host.cpp, pred_plan_fuzz.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "common.h"
#include "filter_plan.h"

namespace dr {

inline bool is_pattern_op(int op) { return op >= DR_OP_STARTSWITH && op <= DR_OP_LIKE; }
inline bool is_date_fn(int op) { return op >= DR_OP_YEAR && op <= DR_OP_TRUNC_DATE; }

// Host validation of the postfix program: types, literals, operand indices and stack discipline.
// The only function here that accepts an unchecked program; the others take one it has passed.
void check_program(const dr_predicate& p);
// What check_program asks of column c's source (bits 24..27 of its type, DR_SRC_*): a known one, a type
// the statistic has, a path within stats_json.h's limits. DR_SRC_PARTITION passes as it is.
void check_column_source(const char* name, int32_t type_with_source, int32_t c);

// dr_state_aggregate's host checks (every one DR_E_INVALID_ARG, naming the first offending spec or
// position). check_agg_specs: naggs in 0..DR_AGG_MAX_SPECS, known fn and input, "" and 0 on a built-in
// input, a valid column type, what check_column_source asks (its texts, the spec index as the column),
// SUM over BYTE .. LONG, size and modificationTime only. check_agg_selection: rows within a side of
// `side` files, group_off from 0 to the selection's size and non-decreasing.
void check_agg_specs(const dr_agg_spec* aggs, int32_t naggs);
void check_agg_selection(const int64_t* rows, int64_t nrows, uint64_t side, const int64_t* group_off, int64_t ngroups);

// dr_state_probe_keys' host checks, in this order, each naming the first offender. check_probe_args:
// flags == 0, nrows in 0..2^32 - 1 where rows are given (a key's files are counted in 32 bits), nkeys in 0..2^31 - 1, keys where nkeys > 0, then per bound
// ("lo", then "hi") a name, a valid type code, a supported base type (STRING, BINARY, DECIMAL and BOOLEAN:
// DR_E_UNSUPPORTED) and what check_column_source asks (its texts, "lo" / "hi" in the column's place), and
// last one base type for both. check_probe_rows: rows within a side of `side` files. Everything but the
// unsupported types is DR_E_INVALID_ARG. The order map the probe compares by is filter_plan.h's
// probe_order_key.
void check_probe_args(bool has_rows, int64_t nrows, const char* lo_name, int32_t lo_type, const char* hi_name,
                      int32_t hi_type, const int64_t* keys, int64_t nkeys, uint32_t flags);
void check_probe_rows(const int64_t* rows, int64_t nrows, uint64_t side);

// Literal k as the evaluators compare it: FLOAT / DOUBLE as their order keys (fp_key32 / fp_key64,
// the device's own functions), a DECIMAL's two words, everything else as given.
void literal_words(const dr_predicate& p, int32_t k, int64_t* lo, int64_t* hi);

// A checked program with its LIKE ops compiled (once per call): every non-NULL LIKE pattern is
// replaced by a new literal -- the needle of the cheaper op its shape folds into (no wildcard: EQ,
// `abc%`: STARTSWITH, `%abc`: ENDSWITH, `%abc%`: CONTAINS, `%`: STARTSWITH of the empty string, which
// unlike IS NOT NULL stays NULL for a NULL value under NOT), or the byte program of like_lane.h under
// DR_OP_LIKE. All three evaluators read these bytes. Returns false when the program has no such op.
struct PatternPred {
  dr_predicate p;
  std::vector<dr_pred_op> ops;
  std::vector<int32_t> lit_types;
  std::vector<int64_t> lit_i64, lit_str_off;
  std::vector<uint8_t> lit_null, bytes;
};
bool compile_patterns(const dr_predicate& p, PatternPred& out);

// Lowers the ABI program to the device form. `x e1..en IN(n)` becomes
// `x IN_START e1 IN_STEP .. en IN_STEP IN_END`, so an IN list of any length needs two stack slots
// beyond its value (In.eval semantics are unchanged: true if any element equals, else null if the
// value or any element is null, else false). Returns (opcode, arg) pairs; fails if the lowered
// program still needs more than the device stack.
std::vector<int32_t> lower_program(const dr_predicate& p);

// Leaf form of a program (k_filter_leaf) when every comparison is between one partition column, bare
// or under at most FL_MAXFN date functions, and literals of its kind and the rest is AND / OR / NOT: each leaf is evaluated straight from the typed
// K5 cache, IN lists become sorted sets searched by bisection, and the boolean combination runs on
// a register stack. Returns false (generic interpreter, k_filter_typed) for anything else.
struct LeafPlan {
  std::vector<FilterLeaf> leaves;
  std::vector<int32_t> prog;
  std::vector<int64_t> i64;        // literal slots (FLOAT / DOUBLE: order keys; DECIMAL: the low word)
  std::vector<int64_t> i64hi;      // parallel: a DECIMAL's high word
  std::vector<std::string> str;
};
bool leafify(const dr_predicate& p, LeafPlan& L);

}  // namespace dr
