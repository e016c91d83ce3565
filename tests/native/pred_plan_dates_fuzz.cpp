// Stand-alone fuzz of delta_amd/csrc/pred_plan.cpp with the date functions, for a sanitizer build
// (tests/test_pred_plan_dates.py builds it with -fsanitize=address,undefined and runs it): pred_plan_fuzz.cpp's
// generator, which also wraps columns in chains of DR_OP_YEAR .. DR_OP_TRUNC_DATE (mostly well-typed, any
// length, any arg) and damages programs with opcodes up to and beyond DR_OP_TRUNC_DATE. Each program ends in
// a dr::Error or in plans whose every leaf, chain, literal and program index is in range.
#include "../../delta_amd/csrc/pred_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

using namespace dr;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return uint32_t((rng_state >> 11) % n);
}
static bool one_in(uint32_t n) { return rnd(n) == 0; }

static const int32_t kTypes[] = {DR_T_STRING, DR_T_BYTE, DR_T_SHORT, DR_T_INT, DR_T_LONG, DR_T_DATE, DR_T_BOOLEAN, DR_T_FLOAT,
                                 DR_T_DOUBLE, DR_T_TIMESTAMP, DR_T_BINARY, DR_T_DECIMAL | 12 << 8 | 2 << 16,
                                 DR_T_DECIMAL | 38 << 8 | 10 << 16};
static const int64_t kValues[] = {0, 1, -1, 7, 63, 64, 65535, 65536, INT64_MIN, INT64_MAX, 0x7ff8000000000001ll, 0x3ff8000000000000ll,
                                  int64_t(0x8000000000000000ull), 0x7fc00000, 0x80000000ll, 0x00000001, 0x3fc00000, int64_t(0xfff0000000000000ull)};
static const char* kPatterns[] = {"", "abc", "abc%", "%abc", "%abc%", "%", "a_c%d", "_", "a\\%", "abc\\", "a\\bc", "\xC3\xA9_%",
                                  "\xff", "%\xC3", "a#_b", "#", "%a%b%c%d%e%f%g%h%i%j%k%l%m%n%o%p%q%r%s%t%u%v%w%x%y%z%"};

struct Gen {
  std::vector<dr_pred_op> ops;
  std::vector<int32_t> col_types, lit_types;
  std::vector<std::string> names, lit_bytes;
  std::vector<int64_t> lit_i64;
  std::vector<uint8_t> lit_null;

  int32_t column() {
    if (col_types.empty() || (col_types.size() < 20 && one_in(3))) {
      col_types.push_back(kTypes[rnd(13)]);
      names.push_back("c" + std::to_string(col_types.size()));
    }
    return int32_t(rnd(uint32_t(col_types.size())));
  }
  int32_t literal(int32_t type) {
    if (one_in(8)) type = kTypes[rnd(13)];
    lit_types.push_back(type);
    lit_null.push_back(one_in(6));
    lit_i64.push_back(one_in(3) ? kValues[rnd(18)] : int64_t(rnd(40)) - 8 + (one_in(4) ? 65500 : 0));
    std::string b;
    if ((type & 0xff) == DR_T_DECIMAL) {
      b.assign(16, one_in(2) ? '\0' : '\xff');  // small, of either sign; now and then beyond any precision
      b[0] = char(rnd(256));
      if (one_in(3)) b[8] = char(rnd(256));
      if (one_in(10)) b[15] = char(rnd(256));
    } else if (one_in(2)) {
      b = kPatterns[rnd(17)];
    } else {
      for (uint32_t n = rnd(12); n; --n) b.push_back(char(one_in(4) ? rnd(256) : "abc%_\\#"[rnd(7)]));
    }
    lit_bytes.push_back(b);
    return int32_t(lit_types.size() - 1);
  }
  void col_op() { ops.push_back(dr_pred_op{DR_OP_COL, column()}); }
  void lit_op(int32_t type) { ops.push_back(dr_pred_op{DR_OP_LIT, literal(type)}); }
  void expr(int depth) {
    const uint32_t pick = depth <= 0 ? rnd(5) : rnd(9);
    if (pick < 5) {
      col_op();
      const size_t c = size_t(ops.back().arg);
      int32_t type = col_types[c];
      if (pick != 2 && one_in(5)) {  // a chain of date functions, mostly over a DATE column and mostly well-typed
        if (!one_in(4)) col_types[c] = DR_T_DATE;
        for (uint32_t n = 1 + rnd(one_in(6) ? 6 : 3); n; --n) {
          const int fn = one_in(5) ? DR_OP_YEAR + int(rnd(10)) : DR_OP_DATE_ADD + int(rnd(2));
          ops.push_back(dr_pred_op{fn, fn == DR_OP_DATE_ADD ? int32_t(rng_state) : one_in(8) ? int32_t(rnd(7)) - 2 : int32_t(rnd(4)) * (fn == DR_OP_TRUNC_DATE)});
        }
        if (one_in(2)) ops.push_back(dr_pred_op{DR_OP_YEAR + int(rnd(7)), 0});
        type = ops.back().opcode >= DR_OP_TO_DATE ? DR_T_DATE : DR_T_INT;
      }
      if (pick == 0) {
        ops.push_back(dr_pred_op{one_in(2) ? int32_t(DR_OP_ISNULL) : int32_t(DR_OP_ISNOTNULL), 0});
      } else if (pick == 1) {
        const uint32_t n = one_in(5) ? 8 + rnd(12) : rnd(5);
        for (uint32_t q = 0; q < n; ++q) one_in(30) ? expr(depth - 1) : lit_op(type == DR_T_FLOAT && one_in(4) ? int32_t(DR_T_DOUBLE) : type);
        ops.push_back(dr_pred_op{DR_OP_IN, int32_t(n)});
      } else if (pick == 2) {
        if (type != DR_T_STRING && !one_in(4)) {  // mostly a STRING column, as the pattern ops require
          col_types[c] = DR_T_STRING;
        }
        lit_op(DR_T_STRING);
        const int op = DR_OP_STARTSWITH + int(rnd(4));
        const int32_t escapes[] = {'\\', '#', 0xE9, 0, 0xD800, 0x10000, -1};
        ops.push_back(dr_pred_op{op, op == DR_OP_LIKE ? escapes[one_in(6) ? rnd(7) : rnd(3)] : int32_t(rnd(3))});
      } else {
        lit_op(type);
        if (one_in(3)) std::swap(ops[ops.size() - 1], ops[ops.size() - 2]);
        ops.push_back(dr_pred_op{DR_OP_EQ + int(rnd(7)), 0});
      }
    } else if (pick == 5) {
      expr(depth - 1);
      ops.push_back(dr_pred_op{DR_OP_NOT, 0});
    } else {
      expr(depth - 1);
      expr(depth - 1);
      ops.push_back(dr_pred_op{pick == 6 ? int(DR_OP_OR) : pick == 7 ? int(DR_OP_AND) : DR_OP_EQ + int(rnd(7)), 0});
    }
  }
  void damage() {
    dr_pred_op& o = ops[rnd(uint32_t(ops.size()))];
    switch (rnd(7)) {
      case 0: o.opcode = int32_t(rnd(33)) - 2; break;
      case 1: o.opcode = int32_t(rng_state); break;
      case 2: o.arg = int32_t(rnd(40)) - 4; break;
      case 3: o.arg = one_in(2) ? INT32_MAX : INT32_MIN; break;
      case 4: ops.erase(ops.begin() + rnd(uint32_t(ops.size()))); break;
      case 5: ops.insert(ops.begin() + rnd(uint32_t(ops.size())), dr_pred_op{int32_t(rnd(30)), int32_t(rnd(6))}); break;
      default:
        if (!lit_types.empty()) lit_types[rnd(uint32_t(lit_types.size()))] = one_in(2) ? int32_t(rng_state >> 8) : int32_t(rnd(14) | rnd(40) << 8 | rnd(40) << 16);
        else col_types[rnd(uint32_t(col_types.size()))] = int32_t(rnd(14)) - 1;
    }
  }
};

template <typename T>
static std::unique_ptr<T[]> exact(const std::vector<T>& v) {
  std::unique_ptr<T[]> p(new T[v.size()]);
  std::copy(v.begin(), v.end(), p.get());
  return p;
}

// `bad` when a lowered / leaf program does not stay within `limit` slots or does not end with one value
static bool walk(int* depth, int delta, int limit) {
  *depth += delta;
  return *depth < 1 || *depth > limit;
}
#define REQUIRE(x)                                                                   \
  do {                                                                               \
    if (!(x)) {                                                                      \
      std::fprintf(stderr, "round %u: %s\n", round_no, #x);                          \
      return 1;                                                                      \
    }                                                                                \
  } while (0)

static uint32_t round_no = 0, accepted = 0, leafified = 0, lowered = 0, folded = 0;

static int run(Gen& g) {
  const int32_t ncols = int32_t(g.col_types.size()), nlits = int32_t(g.lit_types.size());
  std::vector<const char*> name_ptrs;
  for (const std::string& n : g.names) name_ptrs.push_back(n.c_str());
  std::vector<int64_t> off(1, 0);
  std::vector<uint8_t> bytes;
  for (const std::string& b : g.lit_bytes) {
    bytes.insert(bytes.end(), b.begin(), b.end());
    off.push_back(int64_t(bytes.size()));
  }
  auto ops = exact(g.ops);
  auto names = exact(name_ptrs);
  auto col_types = exact(g.col_types), lit_types = exact(g.lit_types);
  auto lit_i64 = exact(g.lit_i64), lit_off = exact(off);
  auto lit_null = exact(g.lit_null), lit_bytes = exact(bytes);
  dr_predicate p{};
  p.nops = int32_t(g.ops.size());
  p.ops = ops.get();
  p.ncols = ncols;
  p.col_names = names.get();
  p.col_types = col_types.get();
  p.nlits = nlits;
  p.lit_types = lit_types.get();
  p.lit_i64 = lit_i64.get();
  p.lit_null = lit_null.get();
  p.lit_str_off = lit_off.get();
  p.lit_str_bytes = lit_bytes.get();
  try {
    check_program(p);
  } catch (const Error& e) {
    REQUIRE(e.status == DR_E_INVALID_ARG || e.status == DR_E_UNSUPPORTED);
    return 0;
  }
  ++accepted;
  PatternPred compiled;
  const bool any = compile_patterns(p, compiled);
  const dr_predicate& q = any ? compiled.p : p;
  folded += any;
  REQUIRE(q.nops == p.nops && q.nlits >= p.nlits && q.ncols == p.ncols);
  for (int32_t k = 0; k < q.nlits; ++k) REQUIRE(q.lit_str_off[k] >= 0 && q.lit_str_off[k] <= q.lit_str_off[k + 1]);
  REQUIRE(!any || size_t(q.lit_str_off[q.nlits]) == compiled.bytes.size());
  for (int32_t k = 0; k < q.nops; ++k) {
    const dr_pred_op o = q.ops[k];
    REQUIRE(o.opcode >= DR_OP_COL && o.opcode <= DR_OP_TRUNC_DATE);
    REQUIRE(o.opcode != DR_OP_COL || (o.arg >= 0 && o.arg < q.ncols));
    REQUIRE(o.opcode != DR_OP_LIT || (o.arg >= 0 && o.arg < q.nlits));
  }
  LeafPlan L;
  if (leafify(q, L)) {
    ++leafified;
    const size_t slots = L.i64.size();
    REQUIRE(L.i64hi.size() == slots && L.str.size() == slots && L.prog.size() % 2 == 0);
    int depth = 0;
    for (size_t k = 0; k < L.prog.size(); k += 2) {
      const int32_t op = L.prog[k];
      REQUIRE(op >= LEAF_OP_LEAF && op <= LEAF_OP_NOT);
      REQUIRE(op != LEAF_OP_LEAF || (L.prog[k + 1] >= 0 && size_t(L.prog[k + 1]) < L.leaves.size()));
      REQUIRE(!walk(&depth, op == LEAF_OP_LEAF ? 1 : op == LEAF_OP_NOT ? 0 : -1, 32));
    }
    REQUIRE(depth == 1);
    for (const FilterLeaf& f : L.leaves) {
      REQUIRE(f.col >= 0 && f.col < q.ncols && f.op >= DR_OP_EQ && f.op <= DR_OP_LIKE && f.lit >= 0 && f.nlit >= 0);
      REQUIRE(f.op != DR_OP_AND && f.op != DR_OP_OR && f.op != DR_OP_NOT);
      REQUIRE(f.nfn >= 0 && f.nfn <= FL_MAXFN);
      for (int32_t n = 0; n < f.nfn; ++n) REQUIRE(is_date_fn(f.fn[n]) && (f.fn[n] != DR_OP_TRUNC_DATE || (f.farg[n] >= 0 && f.farg[n] <= 3)));
      REQUIRE(!f.nfn || (f.pad != 2 && !is_pattern_op(f.op)));
      size_t width = f.op == DR_OP_ISNULL || f.op == DR_OP_ISNOTNULL ? 0 : f.op == DR_OP_IN ? size_t(f.nlit) : 1;
      if (f.pad == 1) {
        REQUIRE(f.op == DR_OP_IN && size_t(f.lit) + 2 <= slots && L.i64[size_t(f.lit) + 1] >= 1 && L.i64[size_t(f.lit) + 1] <= 1024);
        width = 2 + size_t(L.i64[size_t(f.lit) + 1]);
      }
      REQUIRE(size_t(f.lit) + width <= slots);
    }
  }
  try {
    const std::vector<int32_t> low = lower_program(q);
    ++lowered;
    REQUIRE(low.size() % 2 == 0);
    int depth = 0;
    for (size_t k = 0; k < low.size(); k += 2) {
      const int32_t op = low[k], arg = low[k + 1];
      REQUIRE((op >= DR_OP_COL && op <= DR_OP_TRUNC_DATE && op != DR_OP_IN) || (op >= FILTER_OP_IN_START && op <= FILTER_OP_IN_END));
      REQUIRE(op != DR_OP_COL || (arg >= 0 && arg < q.ncols));
      REQUIRE(op != DR_OP_LIT || (arg >= 0 && arg < q.nlits));
      const int delta = op == DR_OP_COL || op == DR_OP_LIT || op == FILTER_OP_IN_START ? 1
                      : op == DR_OP_ISNULL || op == DR_OP_ISNOTNULL || op == DR_OP_NOT || is_date_fn(op) ? 0 : -1;
      REQUIRE(!walk(&depth, delta, PV_STACK));
    }
    REQUIRE(depth == 1);
  } catch (const Error& e) {
    REQUIRE(e.status == DR_E_UNSUPPORTED);
  }
  for (int32_t k = 0; k < q.nlits; ++k) {
    int64_t lo, hi;
    literal_words(q, k, &lo, &hi);
  }
  return 0;
}

int main(int argc, char** argv) {
  const uint32_t rounds = argc > 1 ? uint32_t(std::atoi(argv[1])) : 200000;
  for (round_no = 0; round_no < rounds; ++round_no) {
    Gen g;
    if (one_in(50)) {  // ops with no expression behind them at all
      g.column();
      g.literal(DR_T_INT);
      for (uint32_t n = rnd(12); n; --n) g.ops.push_back(dr_pred_op{int32_t(rnd(31)) - 1, int32_t(rnd(8)) - 2});
    } else {
      g.expr(one_in(20) ? 9 : int(rnd(5)));
      if (one_in(40)) {  // IN lists nested beyond the device stack
        const uint32_t n = 10 + rnd(10);
        for (uint32_t k = 0; k < n; ++k) g.col_op();
        g.lit_op(DR_T_INT);
        for (uint32_t k = 0; k < n; ++k) g.ops.push_back(dr_pred_op{DR_OP_IN, 1});
        g.ops.push_back(dr_pred_op{DR_OP_AND, 0});
      }
      if (!one_in(3))
        for (uint32_t n = 1 + rnd(3); n && !g.ops.empty(); --n) g.damage();
    }
    if (run(g)) return 1;
  }
  // the fuzz does get past check_program, into both plans and into the LIKE compiler
  if (accepted < rounds / 5 || leafified < rounds / 20 || lowered < rounds / 5 || folded < rounds / 200) {
    std::fprintf(stderr, "too few programs accepted: %u accepted, %u leafified, %u lowered, %u with a LIKE compiled\n", accepted,
                 leafified, lowered, folded);
    return 1;
  }
  std::printf("pred_plan fuzz ok: %u rounds, %u accepted, %u leafified, %u lowered, %u with a LIKE compiled\n", rounds, accepted,
              leafified, lowered, folded);
  return 0;
}
