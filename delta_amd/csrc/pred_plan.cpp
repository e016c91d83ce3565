// K5 predicate planner, host only (pred_plan.h says what each function is for).
#include "pred_plan.h"

#include <algorithm>
#include <cstring>
#include <functional>
#include <utility>

#include "date_fn.h"
#include "like_lane.h"
#include "stats_json.h"

namespace dr {

// Which literals a column may be compared with: a FLOAT, DOUBLE, TIMESTAMP, DECIMAL or BINARY column
// (the type codes from DR_T_FLOAT up) takes literals of its own type only (a decimal's precision and
// scale included), a FLOAT column also a DOUBLE literal (the value is widened), and a literal of one
// of those types fits no other column. STRING, the integer kinds, DATE and BOOLEAN among themselves
// are not checked.
// A column's type as the rules below and the evaluators read it: without its source (DR_SRC_*), which
// says where the engine finds the values and nothing about how they compare.
static int32_t col_type(const dr_predicate& p, int32_t c) { return p.col_types[c] & ~int32_t(DR_SRC_MASK); }
static int32_t col_source(const dr_predicate& p, int32_t c) { return (p.col_types[c] >> DR_SRC_SHIFT) & 0xf; }

// check_column_source with the column given as text: an index for a predicate column or an aggregate
// spec, "lo" / "hi" for a bound of dr_state_probe_keys.
static void check_source_of(const char* name, int32_t type_with_source, const char* c) {
  const int32_t src = (type_with_source >> DR_SRC_SHIFT) & 0xf, base = type_with_source & 0xff;
  if (src == DR_SRC_PARTITION) return;
  if (src > DR_SRC_STATS_NUMRECORDS)
    fail(DR_E_INVALID_ARG, fmt("predicate column %s: unknown source %d (DR_SRC_PARTITION .. DR_SRC_STATS_NUMRECORDS)", c, src));
  if ((src == DR_SRC_STATS_MIN || src == DR_SRC_STATS_MAX) && (base == DR_T_BOOLEAN || base == DR_T_BINARY))
    fail(DR_E_INVALID_ARG, fmt("predicate column %s: %s statistics have no %s (type %d)", c, src == DR_SRC_STATS_MIN ? "minValues" : "maxValues",
                               base == DR_T_BOOLEAN ? "BOOLEAN" : "BINARY", base));
  if ((src == DR_SRC_STATS_NULLCOUNT || src == DR_SRC_STATS_NUMRECORDS) && (type_with_source & ~int32_t(DR_SRC_MASK)) != DR_T_LONG)
    fail(DR_E_INVALID_ARG, fmt("predicate column %s: %s is a LONG, not type %d", c, src == DR_SRC_STATS_NULLCOUNT ? "nullCount" : "numRecords",
                               type_with_source & ~int32_t(DR_SRC_MASK)));
  const size_t len = std::strlen(name);
  if (src == DR_SRC_STATS_NUMRECORDS) {
    if (len) fail(DR_E_INVALID_ARG, fmt("predicate column %s: numRecords takes the name \"\", not a path of %zu bytes", c, len));
    return;
  }
  if (len > size_t(sj::SJ_MAXPATH))
    fail(DR_E_INVALID_ARG, fmt("predicate column %s: a statistics path has at most %d bytes, not %zu", c, sj::SJ_MAXPATH, len));
  int segs = 1;
  for (size_t q = 0; q <= len; ++q) {
    const bool end = q == len || uint8_t(name[q]) == sj::SJ_SEP;
    if (end && (q == 0 || uint8_t(name[q - 1]) == sj::SJ_SEP))
      fail(DR_E_INVALID_ARG, fmt("predicate column %s: segment %d of the statistics path is empty", c, segs - 1));
    if (end && q < len) ++segs;
  }
  if (segs > sj::SJ_MAXSEG)
    fail(DR_E_INVALID_ARG, fmt("predicate column %s: a statistics path has at most %d segments, not %d", c, sj::SJ_MAXSEG, segs));
}

void check_column_source(const char* name, int32_t type_with_source, int32_t c) {
  check_source_of(name, type_with_source, fmt("%d", c).c_str());
}

void check_agg_specs(const dr_agg_spec* aggs, int32_t naggs) {
  if (naggs < 0 || naggs > DR_AGG_MAX_SPECS)
    fail(DR_E_INVALID_ARG, fmt("dr_state_aggregate: naggs = %d is outside 0..%d", naggs, DR_AGG_MAX_SPECS));
  if (naggs && !aggs) fail(DR_E_INVALID_ARG, fmt("dr_state_aggregate: aggs == NULL with naggs = %d", naggs));
  for (int32_t a = 0; a < naggs; ++a) {
    const dr_agg_spec& s = aggs[a];
    if (s.fn < DR_AGG_COUNT || s.fn > DR_AGG_SUM)
      fail(DR_E_INVALID_ARG, fmt("aggregate spec %d: unknown fn %d (DR_AGG_COUNT .. DR_AGG_SUM)", a, s.fn));
    if (s.input < DR_AGG_IN_COLUMN || s.input > DR_AGG_IN_MTIME)
      fail(DR_E_INVALID_ARG, fmt("aggregate spec %d: unknown input %d (DR_AGG_IN_COLUMN .. DR_AGG_IN_MTIME)", a, s.input));
    if (s.input != DR_AGG_IN_COLUMN) {
      if ((s.name && s.name[0]) || s.type_with_source)
        fail(DR_E_INVALID_ARG, fmt("aggregate spec %d: %s takes the name \"\" and the type 0", a,
                                   s.input == DR_AGG_IN_SIZE ? "DR_AGG_IN_SIZE" : "DR_AGG_IN_MTIME"));
      continue;
    }
    if (!s.name) fail(DR_E_INVALID_ARG, fmt("aggregate spec %d: a column input needs a name", a));
    const int32_t t = s.type_with_source & ~int32_t(DR_SRC_MASK), base = t & 0xff;
    bool type_ok = s.type_with_source >= 0 && (base == DR_T_DECIMAL || t <= DR_T_BINARY);
    if (type_ok && base == DR_T_DECIMAL) {
      const int32_t prec = (t >> 8) & 0xff, scale = t >> 16;
      type_ok = prec >= 1 && prec <= 38 && scale <= prec;
    }
    if (!type_ok) fail(DR_E_INVALID_ARG, fmt("aggregate spec %d: no valid column type (code %d)", a, s.type_with_source));
    check_column_source(s.name, s.type_with_source, a);
    if (s.fn == DR_AGG_SUM && (t < DR_T_BYTE || t > DR_T_LONG))
      fail(DR_E_INVALID_ARG, fmt("aggregate spec %d: SUM takes BYTE .. LONG, size and modificationTime, not type %d", a, t));
  }
}

void check_agg_selection(const int64_t* rows, int64_t nrows, uint64_t side, const int64_t* group_off, int64_t ngroups) {
  if (rows && nrows < 0) fail(DR_E_INVALID_ARG, fmt("dr_state_aggregate: nrows = %lld is negative", (long long)nrows));
  if (group_off && ngroups < 0) fail(DR_E_INVALID_ARG, fmt("dr_state_aggregate: ngroups = %lld is negative", (long long)ngroups));
  const uint64_t n = rows ? uint64_t(nrows) : side;
  for (uint64_t i = 0; rows && i < n; ++i)
    if (rows[i] < 0 || uint64_t(rows[i]) >= side)
      fail(DR_E_INVALID_ARG, fmt("dr_state_aggregate: rows[%llu] = %lld is outside [0, %llu)", (unsigned long long)i,
                                 (long long)rows[i], (unsigned long long)side));
  if (!group_off) return;
  if (group_off[0] != 0) fail(DR_E_INVALID_ARG, fmt("dr_state_aggregate: group_off[0] = %lld, not 0", (long long)group_off[0]));
  for (int64_t g = 0; g < ngroups; ++g)
    if (group_off[g + 1] < group_off[g])
      fail(DR_E_INVALID_ARG, fmt("dr_state_aggregate: group_off[%lld] = %lld is below group_off[%lld] = %lld", (long long)(g + 1),
                                 (long long)group_off[g + 1], (long long)g, (long long)group_off[g]));
  if (uint64_t(group_off[ngroups]) != n)
    fail(DR_E_INVALID_ARG, fmt("dr_state_aggregate: group_off[%lld] = %lld, not the selection's %llu rows", (long long)ngroups,
                               (long long)group_off[ngroups], (unsigned long long)n));
}

// One bound of dr_state_probe_keys: `who` is "lo" or "hi".
static void check_probe_bound(const char* who, const char* name, int32_t type_with_source) {
  if (!name) fail(DR_E_INVALID_ARG, fmt("dr_state_probe_keys: %s needs a name", who));
  const int32_t t = type_with_source & ~int32_t(DR_SRC_MASK), base = t & 0xff;
  bool type_ok = type_with_source >= 0 && (base == DR_T_DECIMAL || t <= DR_T_BINARY);
  if (type_ok && base == DR_T_DECIMAL) {
    const int32_t prec = (t >> 8) & 0xff, scale = t >> 16;
    type_ok = prec >= 1 && prec <= 38 && scale <= prec;
  }
  if (!type_ok) fail(DR_E_INVALID_ARG, fmt("dr_state_probe_keys: %s has no valid column type (code %d)", who, type_with_source));
  if (base == DR_T_STRING || base == DR_T_BINARY || base == DR_T_DECIMAL || base == DR_T_BOOLEAN)
    fail(DR_E_UNSUPPORTED, fmt("dr_state_probe_keys: %s is of type %d; STRING, BINARY, DECIMAL and BOOLEAN bounds are not probed", who, base));
  check_source_of(name, type_with_source, who);
}

void check_probe_args(bool has_rows, int64_t nrows, const char* lo_name, int32_t lo_type, const char* hi_name,
                      int32_t hi_type, const int64_t* keys, int64_t nkeys, uint32_t flags) {
  if (flags != 0) fail(DR_E_INVALID_ARG, fmt("dr_state_probe_keys: flags = %u, not 0", flags));
  if (has_rows && nrows < 0) fail(DR_E_INVALID_ARG, fmt("dr_state_probe_keys: nrows = %lld is negative", (long long)nrows));
  if (has_rows && nrows > int64_t(UINT32_MAX))  // the kernel counts a key's files in 32 bits
    fail(DR_E_INVALID_ARG, fmt("dr_state_probe_keys: nrows = %lld is above %u", (long long)nrows, UINT32_MAX));
  if (nkeys < 0 || nkeys > int64_t(INT32_MAX))
    fail(DR_E_INVALID_ARG, fmt("dr_state_probe_keys: nkeys = %lld is outside 0..%d", (long long)nkeys, INT32_MAX));
  if (nkeys && !keys) fail(DR_E_INVALID_ARG, fmt("dr_state_probe_keys: keys == NULL with nkeys = %lld", (long long)nkeys));
  check_probe_bound("lo", lo_name, lo_type);
  check_probe_bound("hi", hi_name, hi_type);
  if ((lo_type & 0xff) != (hi_type & 0xff))
    fail(DR_E_INVALID_ARG, fmt("dr_state_probe_keys: lo is of type %d and hi of type %d; both bounds take one base type",
                               lo_type & 0xff, hi_type & 0xff));
}

void check_probe_rows(const int64_t* rows, int64_t nrows, uint64_t side) {
  for (int64_t i = 0; rows && i < nrows; ++i)
    if (rows[i] < 0 || uint64_t(rows[i]) >= side)
      fail(DR_E_INVALID_ARG, fmt("dr_state_probe_keys: rows[%lld] = %lld is outside [0, %llu)", (long long)i, (long long)rows[i],
                                 (unsigned long long)side));
}

static bool new_pred_type(int32_t t) { return (t & 0xff) >= DR_T_FLOAT; }
static bool lit_fits(int32_t ctype, int32_t ltype) {
  if (!new_pred_type(ctype) && !new_pred_type(ltype)) return true;
  return ctype == ltype || (ctype == DR_T_FLOAT && ltype == DR_T_DOUBLE);
}

// A DECIMAL literal: 16 bytes, little-endian two's complement, in the string bytes.
static void decimal_words(const dr_predicate& p, int32_t k, int64_t* lo, int64_t* hi) {
  uint64_t w[2];
  std::memcpy(w, p.lit_str_bytes + p.lit_str_off[k], 16);
  *lo = int64_t(w[0]);
  *hi = int64_t(w[1]);
}

void literal_words(const dr_predicate& p, int32_t k, int64_t* lo, int64_t* hi) {
  *lo = p.lit_i64[k];
  *hi = 0;
  if (p.lit_null[k]) return;
  const int base = p.lit_types[k] & 0xff;
  if (base == DR_T_FLOAT) *lo = fp_key32(uint32_t(p.lit_i64[k]));
  else if (base == DR_T_DOUBLE) *lo = fp_key64(uint64_t(p.lit_i64[k]));
  else if (base == DR_T_DECIMAL) decimal_words(p, k, lo, hi);
}

// ---- string patterns (DR_OP_STARTSWITH .. DR_OP_LIKE) ------------------------------------------------
static const char* pattern_op_name(int op) {
  return op == DR_OP_STARTSWITH ? "STARTSWITH" : op == DR_OP_ENDSWITH ? "ENDSWITH" : op == DR_OP_CONTAINS ? "CONTAINS" : "LIKE";
}
static std::string pred_op_text(const dr_predicate& p, int32_t k) {
  const int op = p.ops[k].opcode, arg = p.ops[k].arg;
  if (op == DR_OP_COL)
    return fmt("%s column %s of type %d", col_source(p, arg) ? "statistics" : "partition", p.col_names[arg], col_type(p, arg));
  if (op == DR_OP_LIT) return p.lit_null[arg] ? std::string("a NULL literal") : fmt("literal %d of type %d", arg, p.lit_types[arg]);
  return fmt("the result of op %d (opcode %d)", k, op);
}
static lk::LikeCompiled compile_like(const dr_predicate& p, int32_t lit, int32_t escape) {
  const int64_t b = p.lit_str_off[lit], e = p.lit_str_off[lit + 1];
  return lk::like_compile(p.lit_str_bytes + b, size_t(e - b), uint32_t(escape));
}
// Pattern op k over the operands rooted at ops vk (value) and pk (pattern): the value a STRING
// partition column, the pattern a STRING or NULL literal, a LIKE pattern well-formed. The pattern is
// the last operand and, being a literal, a single op: it is op k - 1, where compile_patterns reads it.
static void check_pattern_op(const dr_predicate& p, int32_t k, int32_t vk, int32_t pk) {
  const int op = p.ops[k].opcode;
  const char* name = pattern_op_name(op);
  if (p.ops[vk].opcode != DR_OP_COL || col_type(p, p.ops[vk].arg) != DR_T_STRING)
    fail(DR_E_INVALID_ARG, fmt("predicate op %d (%s): the value must be a STRING partition column, found %s", k, name,
                               pred_op_text(p, vk).c_str()));
  const int32_t l = p.ops[pk].arg;
  if (p.ops[pk].opcode != DR_OP_LIT || (!p.lit_null[l] && p.lit_types[l] != DR_T_STRING))
    fail(DR_E_INVALID_ARG, fmt("predicate op %d (%s): the pattern must be a STRING or NULL literal, found %s", k, name,
                               pred_op_text(p, pk).c_str()));
  if (!p.lit_null[l] && (!p.lit_str_off || p.lit_str_off[l] < 0 || p.lit_str_off[l + 1] < p.lit_str_off[l] ||
                         (p.lit_str_off[l + 1] > p.lit_str_off[l] && !p.lit_str_bytes)))
    fail(DR_E_INVALID_ARG, fmt("predicate op %d (%s): literal %d has no valid bytes", k, name, l));
  if (op != DR_OP_LIKE) return;
  const int32_t esc = p.ops[k].arg;
  if (esc < 1 || esc > 0xFFFF || (esc >= 0xD800 && esc <= 0xDFFF))
    fail(DR_E_INVALID_ARG, fmt("predicate op %d (LIKE): the escape character (arg %d) must be a code point in 1..0xFFFF and no surrogate", k, esc));
  if (p.lit_null[l]) return;
  const lk::LikeCompiled c = compile_like(p, l, esc);
  if (!c.error.empty()) fail(DR_E_INVALID_ARG, fmt("predicate op %d (LIKE): %s", k, c.error.c_str()));
}

bool compile_patterns(const dr_predicate& p, PatternPred& out) {
  bool any = false;
  for (int32_t k = 0; k < p.nops; ++k) any |= p.ops[k].opcode == DR_OP_LIKE && !p.lit_null[p.ops[k - 1].arg];
  if (!any) return false;
  const size_t nl = size_t(p.nlits);
  out.ops.assign(p.ops, p.ops + p.nops);
  out.lit_types.assign(p.lit_types, p.lit_types + nl);
  out.lit_i64.assign(p.lit_i64, p.lit_i64 + nl);
  out.lit_null.assign(p.lit_null, p.lit_null + nl);
  out.lit_str_off.assign(p.lit_str_off, p.lit_str_off + nl + 1);
  if (out.lit_str_off.back() > 0) out.bytes.assign(p.lit_str_bytes, p.lit_str_bytes + out.lit_str_off.back());
  for (int32_t k = 0; k < p.nops; ++k) {
    if (p.ops[k].opcode != DR_OP_LIKE || p.lit_null[p.ops[k - 1].arg]) continue;
    const lk::LikeCompiled c = compile_like(p, p.ops[k - 1].arg, p.ops[k].arg);
    out.ops[size_t(k) - 1].arg = int32_t(out.lit_types.size());
    out.ops[size_t(k)].opcode = c.kind == lk::LIKE_EQ ? DR_OP_EQ : c.kind == lk::LIKE_STARTSWITH ? DR_OP_STARTSWITH
                              : c.kind == lk::LIKE_ENDSWITH ? DR_OP_ENDSWITH : c.kind == lk::LIKE_CONTAINS ? DR_OP_CONTAINS
                              : DR_OP_LIKE;
    out.ops[size_t(k)].arg = 0;
    out.lit_types.push_back(DR_T_STRING);
    out.lit_i64.push_back(0);
    out.lit_null.push_back(0);
    out.bytes.insert(out.bytes.end(), c.text.begin(), c.text.end());
    out.lit_str_off.push_back(int64_t(out.bytes.size()));
  }
  out.p = p;
  out.p.ops = out.ops.data();
  out.p.nlits = int32_t(out.lit_types.size());
  out.p.lit_types = out.lit_types.data();
  out.p.lit_i64 = out.lit_i64.data();
  out.p.lit_null = out.lit_null.data();
  out.p.lit_str_off = out.lit_str_off.data();
  out.p.lit_str_bytes = out.bytes.data();
  return true;
}

// ---- date functions (DR_OP_YEAR .. DR_OP_TRUNC_DATE) -------------------------------------------------
static_assert(int(df::FN_YEAR) == int(DR_OP_YEAR) && int(df::FN_QUARTER) == int(DR_OP_QUARTER) && int(df::FN_MONTH) == int(DR_OP_MONTH) &&
              int(df::FN_DAYOFMONTH) == int(DR_OP_DAYOFMONTH) && int(df::FN_DAYOFWEEK) == int(DR_OP_DAYOFWEEK) &&
              int(df::FN_DAYOFYEAR) == int(DR_OP_DAYOFYEAR) && int(df::FN_WEEKOFYEAR) == int(DR_OP_WEEKOFYEAR) && int(df::FN_TO_DATE) == int(DR_OP_TO_DATE) &&
              int(df::FN_DATE_ADD) == int(DR_OP_DATE_ADD) && int(df::FN_TRUNC_DATE) == int(DR_OP_TRUNC_DATE),
              "date_fn.h's function codes are the ABI's opcodes");
static const char* date_fn_name(int op) {
  static const char* const names[] = {"YEAR", "QUARTER", "MONTH", "DAYOFMONTH", "DAYOFWEEK", "DAYOFYEAR", "WEEKOFYEAR",
                                      "TO_DATE", "DATE_ADD", "TRUNC_DATE"};
  return names[op - DR_OP_YEAR];
}
static int32_t date_fn_operand(int op) { return op == DR_OP_TO_DATE ? DR_T_TIMESTAMP : DR_T_DATE; }
static int32_t date_fn_result(int op) { return op >= DR_OP_TO_DATE ? DR_T_DATE : DR_T_INT; }
static const char* type_name(int32_t t) { return t == DR_T_TIMESTAMP ? "TIMESTAMP" : t == DR_T_DATE ? "DATE" : "INT"; }
static bool int_kind(int32_t t) { return t >= DR_T_BYTE && t <= DR_T_LONG; }
// The static type of op k's value where the date rules need one: a column's, a literal's, a function's
// result; -1 for anything else (a boolean).
static int32_t value_type(const dr_predicate& p, int32_t k) {
  const int op = p.ops[k].opcode, arg = p.ops[k].arg;
  return op == DR_OP_COL ? col_type(p, arg) : op == DR_OP_LIT ? p.lit_types[arg] : is_date_fn(op) ? date_fn_result(op) : -1;
}
// Function op k over the operand rooted at op vk: a column or a function of the operand type, then the arg.
static void check_date_fn(const dr_predicate& p, int32_t k, int32_t vk) {
  const int op = p.ops[k].opcode, arg = p.ops[k].arg, vop = p.ops[vk].opcode;
  const int32_t want = date_fn_operand(op);
  if ((vop != DR_OP_COL && !is_date_fn(vop)) || value_type(p, vk) != want)
    fail(DR_E_INVALID_ARG, fmt("predicate op %d (%s): the operand must be a %s value, found %s", k, date_fn_name(op),
                               type_name(want), pred_op_text(p, vk).c_str()));
  if (op == DR_OP_TRUNC_DATE && (arg < 0 || arg > 3))
    fail(DR_E_INVALID_ARG, fmt("predicate op %d (TRUNC_DATE): the unit (arg %d) must be 0 YEAR, 1 QUARTER, 2 MONTH or 3 WEEK", k, arg));
  if (op != DR_OP_TRUNC_DATE && op != DR_OP_DATE_ADD && arg != 0)
    fail(DR_E_INVALID_ARG, fmt("predicate op %d (%s): takes no argument (arg %d must be 0)", k, date_fn_name(op), arg));
}
// Function result fk (op k compares it) against the value rooted at op ok: a literal of the result's kind
// or NULL; a column or another function result of the same family (integer kinds, or DATE).
static void check_date_fn_peer(const dr_predicate& p, int32_t k, int32_t fk, int32_t ok) {
  const int fop = p.ops[fk].opcode;
  const int32_t rt = date_fn_result(fop), ot = value_type(p, ok);
  auto same_family = [&](int32_t t) { return rt == DR_T_DATE ? t == DR_T_DATE : int_kind(t); };
  if (p.ops[ok].opcode == DR_OP_LIT) {
    const int32_t l = p.ops[ok].arg;
    if (!p.lit_null[l] && !same_family(ot))
      fail(DR_E_INVALID_ARG, fmt("predicate literal %d (type %d) does not fit the result of op %d (%s, type %d)", l, ot, fk,
                                 date_fn_name(fop), rt));
    return;
  }
  if (!same_family(ot))
    fail(DR_E_INVALID_ARG, fmt("predicate op %d: the result of op %d (%s, type %d) does not compare with %s", k, fk,
                               date_fn_name(fop), rt, pred_op_text(p, ok).c_str()));
}

// ---- the program as a tree ---------------------------------------------------------------------------
// The values an op takes off the stack, every opcode listed; -1: no such opcode, or an IN list of a
// negative length.
static int64_t arity(const dr_pred_op& o) {
  switch (o.opcode) {
    case DR_OP_COL: case DR_OP_LIT:
      return 0;
    case DR_OP_ISNULL: case DR_OP_ISNOTNULL: case DR_OP_NOT:
    case DR_OP_YEAR: case DR_OP_QUARTER: case DR_OP_MONTH: case DR_OP_DAYOFMONTH: case DR_OP_DAYOFWEEK:
    case DR_OP_DAYOFYEAR: case DR_OP_WEEKOFYEAR: case DR_OP_TO_DATE: case DR_OP_DATE_ADD: case DR_OP_TRUNC_DATE:
      return 1;
    case DR_OP_EQ: case DR_OP_NE: case DR_OP_LT: case DR_OP_LE: case DR_OP_GT: case DR_OP_GE: case DR_OP_NSEQ:
    case DR_OP_AND: case DR_OP_OR:
    case DR_OP_STARTSWITH: case DR_OP_ENDSWITH: case DR_OP_CONTAINS: case DR_OP_LIKE:
      return 2;
    case DR_OP_IN:
      return o.arg < 0 ? -1 : int64_t(o.arg) + 1;
    default:
      return -1;
  }
}
struct Kids {  // the n ops whose values an op takes, in operand order
  const int32_t* b;
  size_t n;
  int32_t operator[](size_t q) const { return b[q]; }
};
// Postfix -> tree: every op's operands are whole subtrees, named by their last (root) op. It stops at
// the first op that has no arity or finds too few values below it; check_program turns that into
// the error, and a program that passed it has none (bad == nops, left == 1).
struct Tree {
  // one block: at[nops + 1], then kid[nops] (an op is the operand of at most one other), then the
  // stack the walk uses; op k's operands are kid[at[k]] .. kid[at[k + 1])
  std::vector<int32_t> buf;
  int32_t nops;
  int32_t bad;   // the op it stopped at (nops: none)
  size_t left;   // values on the stack there
  Kids kids(int32_t k) const {
    const int32_t* at = buf.data();
    return Kids{at + nops + 1 + at[k], size_t(at[k + 1] - at[k])};
  }
};
static Tree tree_of(const dr_predicate& p) {
  const size_t nops = size_t(p.nops);
  Tree t{std::vector<int32_t>(3 * nops + 1), p.nops, p.nops, 0};
  int32_t *at = t.buf.data(), *kid = at + nops + 1, *stack = kid + nops;
  size_t depth = 0;
  for (int32_t k = 0; k < p.nops; ++k) {
    const int64_t n = arity(p.ops[k]);
    if (n < 0 || int64_t(depth) < n) {
      t.bad = k;
      break;
    }
    depth -= size_t(n);
    std::copy(stack + depth, stack + depth + n, kid + at[k]);
    at[k + 1] = at[k] + int32_t(n);
    stack[depth++] = k;
  }
  t.left = depth;
  return t;
}

void check_program(const dr_predicate& p) {
  if (p.ncols < 0 || p.ncols > PV_MAXC)
    fail(DR_E_UNSUPPORTED, fmt("at most %u partition columns per predicate", unsigned(PV_MAXC)));
  if (p.nops <= 0 || !p.ops) fail(DR_E_INVALID_ARG, "empty predicate program");
  if (p.ncols && (!p.col_names || !p.col_types)) fail(DR_E_INVALID_ARG, "missing partition columns");
  if (p.nlits && (!p.lit_types || !p.lit_i64 || !p.lit_null || !p.lit_str_off))
    fail(DR_E_INVALID_ARG, "missing literals");
  // a type code: STRING .. BINARY bare, DECIMAL | p << 8 | s << 16 with 1 <= p <= 38, s <= p
  auto type_ok = [](int32_t t) {
    if (t < 0) return false;
    if ((t & 0xff) != DR_T_DECIMAL) return t <= DR_T_BINARY;
    const int32_t prec = (t >> 8) & 0xff, scale = t >> 16;
    return prec >= 1 && prec <= 38 && scale <= prec;
  };
  for (int32_t c = 0; c < p.ncols; ++c) {
    if (p.col_types[c] < 0 || !type_ok(col_type(p, c)) || !p.col_names[c])
      fail(DR_E_UNSUPPORTED, "unsupported partition column type");
    check_column_source(p.col_names[c], p.col_types[c], c);
  }
  for (int32_t k = 0; k < p.nlits; ++k) {
    if (p.lit_null[k]) continue;
    const int32_t t = p.lit_types[k];
    if (!type_ok(t)) fail(DR_E_INVALID_ARG, fmt("predicate literal %d has no valid type (code %d)", k, t));
    if ((t & 0xff) != DR_T_DECIMAL) continue;
    if (!p.lit_str_bytes || p.lit_str_off[k] < 0 || p.lit_str_off[k + 1] - p.lit_str_off[k] != 16)
      fail(DR_E_INVALID_ARG, fmt("decimal literal %d must be 16 bytes (little-endian two's complement)", k));
    int64_t lo, hi;
    decimal_words(p, k, &lo, &hi);
    // (assembled unsigned: shifting a negative high word left is undefined)
    const __int128 v = __int128(((unsigned __int128)uint64_t(hi) << 64) | uint64_t(lo));
    unsigned __int128 lim = 1;
    for (int32_t d = 0; d < ((t >> 8) & 0xff); ++d) lim *= 10;
    if ((v < 0 ? (unsigned __int128)0 - (unsigned __int128)v : (unsigned __int128)v) >= lim)
      fail(DR_E_INVALID_ARG, fmt("decimal literal %d does not fit precision %d", k, (t >> 8) & 0xff));
  }
  // a literal compared with a column must be of a kind the column takes (lit_fits)
  auto fits = [&](int32_t ck, int32_t lk) {
    if (p.ops[ck].opcode != DR_OP_COL || p.ops[lk].opcode != DR_OP_LIT) return;
    const int32_t c = p.ops[ck].arg, l = p.ops[lk].arg;
    if (!p.lit_null[l] && !lit_fits(col_type(p, c), p.lit_types[l]))
      fail(DR_E_INVALID_ARG, fmt("predicate literal %d (type %d) does not fit partition column %s (type %d)", l,
                                 p.lit_types[l], p.col_names[c], col_type(p, c)));
  };
  // op by op, so that the first fault in program order is the one reported: its indices, its place in
  // the tree, then its operands
  const Tree t = tree_of(p);
  for (int32_t k = 0; k < p.nops; ++k) {
    const int op = p.ops[k].opcode, arg = p.ops[k].arg;
    if (op == DR_OP_COL && (arg < 0 || arg >= p.ncols)) fail(DR_E_INVALID_ARG, "predicate column index out of range");
    if (op == DR_OP_LIT && (arg < 0 || arg >= p.nlits)) fail(DR_E_INVALID_ARG, "predicate literal index out of range");
    if (k == t.bad)
      fail(DR_E_INVALID_ARG, op == DR_OP_IN ? "predicate stack underflow (IN)"
                             : arity(p.ops[k]) < 0 ? fmt("unknown predicate opcode %d", op) : "predicate stack underflow");
    const Kids ch = t.kids(k);
    if (is_pattern_op(op)) check_pattern_op(p, k, ch[0], ch[1]);
    if (is_date_fn(op)) check_date_fn(p, k, ch[0]);
    // an INT or a DATE is no boolean: a function result goes under a comparison, IN, IS [NOT] NULL or
    // another function, not under AND / OR / NOT
    if (op == DR_OP_AND || op == DR_OP_OR || op == DR_OP_NOT)
      for (size_t q = 0; q < ch.n; ++q)
        if (is_date_fn(p.ops[ch[q]].opcode))
          fail(DR_E_INVALID_ARG, fmt("predicate op %d (%s): the operand must be a boolean, found the result of op %d (%s, type %d)", k,
                                     op == DR_OP_AND ? "AND" : op == DR_OP_OR ? "OR" : "NOT", ch[q],
                                     date_fn_name(p.ops[ch[q]].opcode), date_fn_result(p.ops[ch[q]].opcode)));
    // a function result on either side of a comparison, or as the value or an element of an IN
    auto peers = [&](int32_t ak, int32_t bk) {
      if (is_date_fn(p.ops[ak].opcode)) check_date_fn_peer(p, k, ak, bk);
      else if (is_date_fn(p.ops[bk].opcode)) check_date_fn_peer(p, k, bk, ak);
    };
    if (op >= DR_OP_EQ && op <= DR_OP_NSEQ) {
      fits(ch[0], ch[1]);
      fits(ch[1], ch[0]);
      peers(ch[0], ch[1]);
    } else if (op == DR_OP_IN) {
      for (size_t q = 1; q < ch.n; ++q) {
        fits(ch[0], ch[q]);
        peers(ch[0], ch[q]);
      }
    }
  }
  if (t.left != 1) fail(DR_E_INVALID_ARG, "predicate program must leave one value");
  const int last = p.ops[p.nops - 1].opcode;  // nor is one the program's value
  if (is_date_fn(last))
    fail(DR_E_INVALID_ARG, fmt("predicate program must leave a boolean, op %d (%s) leaves a value of type %d", p.nops - 1,
                               date_fn_name(last), date_fn_result(last)));
}

std::vector<int32_t> lower_program(const dr_predicate& p) {
  const Tree t = tree_of(p);
  std::vector<int32_t> out;
  int depth = 0, max_depth = 0;
  auto put = [&](int32_t op, int32_t arg, int delta) {
    out.push_back(op);
    out.push_back(arg);
    depth += delta;
    max_depth = std::max(max_depth, depth);
  };
  std::function<void(int32_t)> emit = [&](int32_t k) {
    const int op = p.ops[k].opcode, arg = p.ops[k].arg;
    const Kids ch = t.kids(k);
    if (op == DR_OP_IN) {
      emit(ch[0]);
      put(FILTER_OP_IN_START, 0, +1);
      for (size_t q = 1; q < ch.n; ++q) {
        emit(ch[q]);
        put(FILTER_OP_IN_STEP, 0, -1);
      }
      put(FILTER_OP_IN_END, 0, -1);
      return;
    }
    for (size_t q = 0; q < ch.n; ++q) emit(ch[q]);
    put(op, arg, 1 - int(ch.n));
  };
  emit(p.nops - 1);
  if (max_depth > PV_STACK) fail(DR_E_UNSUPPORTED, "predicate program too deep");
  return out;
}

bool leafify(const dr_predicate& p, LeafPlan& L) {
  const Tree t = tree_of(p);
  auto is_col = [&](int32_t k) { return p.ops[k].opcode == DR_OP_COL; };
  // chain(col): a column under at most FL_MAXFN date functions (none: the bare column); `f` gets the
  // column and the functions, innermost first
  auto is_chain = [&](int32_t k, FilterLeaf& f) {
    int32_t n = 0;
    for (int32_t q = k; is_date_fn(p.ops[q].opcode); q = t.kids(q)[0]) ++n;
    if (n > FL_MAXFN) return false;
    f.nfn = n;
    for (; is_date_fn(p.ops[k].opcode); k = t.kids(k)[0]) {
      f.fn[--n] = p.ops[k].opcode;
      f.farg[n] = p.ops[k].arg;
    }
    f.col = p.ops[k].arg;
    return is_col(k);
  };
  auto is_lit = [&](int32_t k) { return p.ops[k].opcode == DR_OP_LIT; };
  auto is_str = [](int32_t t) { return leaf_kind(t) == DR_T_STRING; };
  // string (and binary) columns with literals of bytes, others numeric; the new types by lit_fits
  auto kind_ok = [&](int32_t col, int32_t lit) {
    return is_str(col_type(p, col)) == is_str(p.lit_types[lit]) && lit_fits(col_type(p, col), p.lit_types[lit]);
  };
  // a FLOAT column's literal as the leaf compares it: a DOUBLE literal's key as it is (the leaf widens
  // the value, pad = 2), and then a FLOAT literal's key widened like the value
  auto fp_word = [&](int32_t lit, bool widen) {
    int64_t lo, hi;
    literal_words(p, lit, &lo, &hi);
    return widen && p.lit_types[lit] == DR_T_FLOAT ? fp_key_widen(lo) : lo;
  };
  auto slot = [&](int32_t lit) {
    int64_t lo, hi;
    literal_words(p, lit, &lo, &hi);
    L.i64.push_back(lo);
    L.i64hi.push_back(hi);
    if (is_str(p.lit_types[lit]))
      L.str.emplace_back(reinterpret_cast<const char*>(p.lit_str_bytes) + p.lit_str_off[lit],
                         size_t(p.lit_str_off[lit + 1] - p.lit_str_off[lit]));
    else L.str.emplace_back();
    return int32_t(L.i64.size() - 1);
  };
  int depth = 0, max_depth = 0;
  std::function<bool(int32_t)> emit = [&](int32_t k) -> bool {
    const int op = p.ops[k].opcode;
    const Kids ch = t.kids(k);
    auto push_leaf = [&](const FilterLeaf& f) {
      L.prog.push_back(LEAF_OP_LEAF);
      L.prog.push_back(int32_t(L.leaves.size()));
      L.leaves.push_back(f);
      max_depth = std::max(max_depth, ++depth);
      return true;
    };
    switch (op) {
      case DR_OP_AND: case DR_OP_OR:
        if (!emit(ch[0]) || !emit(ch[1])) return false;
        L.prog.push_back(op == DR_OP_AND ? LEAF_OP_AND : LEAF_OP_OR);
        L.prog.push_back(0);
        --depth;
        return true;
      case DR_OP_NOT:
        if (!emit(ch[0])) return false;
        L.prog.push_back(LEAF_OP_NOT);
        L.prog.push_back(0);
        return true;
      case DR_OP_ISNULL: case DR_OP_ISNOTNULL: {
        FilterLeaf f{};
        if (!is_chain(ch[0], f)) return false;
        f.op = op;
        return push_leaf(f);
      }
      case DR_OP_EQ: case DR_OP_NE: case DR_OP_LT: case DR_OP_LE: case DR_OP_GT: case DR_OP_GE: case DR_OP_NSEQ: {
        FilterLeaf f{};
        int32_t l;
        f.op = op;
        if (is_lit(ch[1]) && is_chain(ch[0], f)) {
          l = p.ops[ch[1]].arg;
        } else if (is_lit(ch[0]) && is_chain(ch[1], f)) {
          l = p.ops[ch[0]].arg;
          f.op = op == DR_OP_LT ? DR_OP_GT : op == DR_OP_GT ? DR_OP_LT : op == DR_OP_LE ? DR_OP_GE
               : op == DR_OP_GE ? DR_OP_LE : op;
        } else {
          return false;
        }
        const int32_t c = f.col;
        // a function result: an integer against an integer literal, whatever the column (check_program)
        if (!f.nfn && !p.lit_null[l] && !kind_ok(c, l)) return false;
        const bool widen = !f.nfn && !p.lit_null[l] && col_type(p, c) == DR_T_FLOAT && p.lit_types[l] == DR_T_DOUBLE;
        f.lit = slot(l);
        f.lit_null = p.lit_null[l] ? 1 : 0;
        f.pad = widen ? 2 : 0;
        return push_leaf(f);
      }
      case DR_OP_STARTSWITH: case DR_OP_ENDSWITH: case DR_OP_CONTAINS: case DR_OP_LIKE: {
        // check_program: a STRING column and a STRING or NULL literal (LIKE: compiled, compile_patterns)
        const int32_t l = p.ops[ch[1]].arg;
        if (p.lit_null[l]) {  // NULL whatever the value; its type field may hold anything
          L.i64.push_back(0);
          L.i64hi.push_back(0);
          L.str.emplace_back();
          return push_leaf(FilterLeaf{p.ops[ch[0]].arg, op, int32_t(L.i64.size() - 1), 0, 1, 0});
        }
        return push_leaf(FilterLeaf{p.ops[ch[0]].arg, op, slot(l), 0, 0, 0});
      }
      case DR_OP_IN: {
        FilterLeaf f{};
        if (!is_chain(ch[0], f)) return false;
        f.op = DR_OP_IN;
        const int32_t c = f.col;
        // a function result is a 32-bit integer: a sorted set or a bitmap, like an INT column's
        const int kind = f.nfn ? DR_T_INT : leaf_kind(col_type(p, c));
        const bool str = kind == DR_T_STRING;
        bool has_null = false, widen = false;
        std::vector<int64_t> iv;
        std::vector<std::pair<int64_t, uint64_t>> dv;  // decimals: (high signed, low unsigned)
        std::vector<std::string> sv;
        for (size_t q = 1; q < ch.n; ++q)  // a FLOAT column with a DOUBLE element: all in binary64
          widen |= !f.nfn && is_lit(ch[q]) && !p.lit_null[p.ops[ch[q]].arg] && col_type(p, c) == DR_T_FLOAT &&
                   p.lit_types[p.ops[ch[q]].arg] == DR_T_DOUBLE;
        for (size_t q = 1; q < ch.n; ++q) {
          if (!is_lit(ch[q])) return false;
          const int32_t l = p.ops[ch[q]].arg;
          if (p.lit_null[l]) { has_null = true; continue; }
          if (!f.nfn && !kind_ok(c, l)) return false;
          if (str) {
            sv.emplace_back(reinterpret_cast<const char*>(p.lit_str_bytes) + p.lit_str_off[l],
                            size_t(p.lit_str_off[l + 1] - p.lit_str_off[l]));
          } else if (kind == DR_T_DECIMAL) {
            int64_t lo, hi;
            literal_words(p, l, &lo, &hi);
            dv.emplace_back(hi, uint64_t(lo));
          } else {
            iv.push_back(fp_word(l, widen));  // FLOAT / DOUBLE: the key, so the set is sorted by key
          }
        }
        if (kind == DR_T_DECIMAL) {  // sorted as 128-bit values
          std::sort(dv.begin(), dv.end());
          dv.erase(std::unique(dv.begin(), dv.end()), dv.end());
          const int32_t first = int32_t(L.i64.size());
          for (const auto& d : dv) {
            L.i64.push_back(int64_t(d.second));
            L.i64hi.push_back(d.first);
            L.str.emplace_back();
          }
          f.lit = first;
          f.nlit = int32_t(dv.size());
          f.lit_null = has_null ? 1 : 0;
          return push_leaf(f);
        }
        std::sort(iv.begin(), iv.end());
        iv.erase(std::unique(iv.begin(), iv.end()), iv.end());
        std::sort(sv.begin(), sv.end());  // bytewise (std::string compares as unsigned char)
        sv.erase(std::unique(sv.begin(), sv.end()), sv.end());
        const int32_t first = int32_t(L.i64.size());
        const size_t m = str ? sv.size() : iv.size();
        // an integer set spanning < 2^16 values: a bitmap, one word read per file instead of a
        // binary search (pad = 1; literals [min, words, bits...])
        const bool fp = kind == DR_T_FLOAT || kind == DR_T_DOUBLE;  // the bitmap: one-word integer kinds only
        if (!str && !fp && m >= 8 && uint64_t(iv.back()) - uint64_t(iv.front()) < 65536) {
          const uint64_t span = uint64_t(iv.back()) - uint64_t(iv.front()) + 1, nw = (span + 63) / 64;
          std::vector<uint64_t> bits(nw, 0);
          for (int64_t x : iv) {
            const uint64_t d = uint64_t(x) - uint64_t(iv.front());
            bits[d >> 6] |= uint64_t(1) << (d & 63);
          }
          L.i64.push_back(iv.front());
          L.i64.push_back(int64_t(nw));
          for (uint64_t w : bits) L.i64.push_back(int64_t(w));
          L.i64hi.resize(L.i64.size(), 0);
          L.str.resize(L.i64.size());
          f.lit = first;
          f.nlit = int32_t(m);
          f.lit_null = has_null ? 1 : 0;
          f.pad = 1;
          return push_leaf(f);
        }
        for (size_t q = 0; q < m; ++q) {
          L.i64.push_back(str ? 0 : iv[q]);
          L.i64hi.push_back(0);
          L.str.push_back(str ? sv[q] : std::string());
        }
        f.lit = first;
        f.nlit = int32_t(m);
        f.lit_null = has_null ? 1 : 0;
        f.pad = widen ? 2 : 0;
        return push_leaf(f);
      }
      default:
        return false;
    }
  };
  return emit(p.nops - 1) && max_depth <= 32;
}

}  // namespace dr
