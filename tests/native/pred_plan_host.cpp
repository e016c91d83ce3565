// Host build of the K5 predicate planner (delta_amd/csrc/pred_plan.cpp) for tests/test_pred_plan.py:
// the dr_predicate that predicates.lower_program builds goes through the functions dr_filter calls,
// and what they make comes back as JSON text.
#include "../../delta_amd/csrc/pred_plan.h"

#include <cstring>

using namespace dr;

namespace {

struct Json {
  std::string s;
  template <typename It>
  void ints(const char* key, It b, It e) {
    s += fmt("\"%s\": [", key);
    for (It i = b; i != e; ++i) s += (i == b ? "" : ", ") + std::to_string((long long)*i);
    s += "]";
  }
  void hex(const uint8_t* b, size_t n) {
    s += '"';
    for (size_t k = 0; k < n; ++k) s += fmt("%02x", b[k]);
    s += '"';
  }
};

int give(const std::string& text, char* out, uint32_t cap) {
  if (text.size() + 1 > cap) return -1;
  std::memcpy(out, text.c_str(), text.size() + 1);
  return 0;
}

}  // namespace

extern "C" {

// filter_plan.h's values that the tests name, so that a change there fails them instead of passing by.
void pp_constants(int32_t out[9]) {
  const int32_t v[9] = {PV_MAXC, PV_STACK, LEAF_OP_LEAF, LEAF_OP_AND, LEAF_OP_OR, LEAF_OP_NOT, FILTER_OP_IN_START,
                        FILTER_OP_IN_STEP, FILTER_OP_IN_END};
  std::memcpy(out, v, sizeof v);
}

// check_program's verdict: 0, or the status with the message in msg.
int pp_check(const dr_predicate* p, char* msg, uint32_t cap) {
  try {
    check_program(*p);
  } catch (const Error& e) {
    give(e.what(), msg, cap);
    return e.status;
  }
  msg[0] = 0;
  return 0;
}

// The plan of a program that passes check_program, as one JSON object: the program and literals
// after compile_patterns, lower_program's pairs (or its status and message) and, when leafify takes
// the program, the flat LeafPlan (`leaf`: null otherwise). Returns 0, check_program's status, or -1
// when `out` is too small.
int pp_plan(const dr_predicate* given, char* out, uint32_t cap) {
  try {
    check_program(*given);
  } catch (const Error& e) {
    return e.status;
  }
  PatternPred compiled;
  const bool folded = compile_patterns(*given, compiled);
  const dr_predicate& p = folded ? compiled.p : *given;
  Json j;
  j.s = fmt("{\"compiled\": %s, \"ops\": [", folded ? "true" : "false");
  for (int32_t k = 0; k < p.nops; ++k) j.s += fmt("%s[%d, %d]", k ? ", " : "", p.ops[k].opcode, p.ops[k].arg);
  j.s += "], ";
  j.ints("lit_types", p.lit_types, p.lit_types + p.nlits);
  j.s += ", ";
  j.ints("lit_i64", p.lit_i64, p.lit_i64 + p.nlits);
  j.s += ", ";
  j.ints("lit_null", p.lit_null, p.lit_null + p.nlits);
  j.s += ", \"lit_bytes\": [";
  for (int32_t k = 0; k < p.nlits; ++k) {
    j.s += k ? ", " : "";
    j.hex(p.lit_str_bytes + p.lit_str_off[k], size_t(p.lit_str_off[k + 1] - p.lit_str_off[k]));
  }
  j.s += "], \"words\": [";
  for (int32_t k = 0; k < p.nlits; ++k) {
    int64_t lo, hi;
    literal_words(p, k, &lo, &hi);
    j.s += fmt("%s[%lld, %lld]", k ? ", " : "", (long long)lo, (long long)hi);
  }
  j.s += "], ";
  try {
    const std::vector<int32_t> low = lower_program(p);
    j.ints("lowered", low.begin(), low.end());
  } catch (const Error& e) {
    j.s += fmt("\"lowered\": null, \"lower_status\": %d, \"lower_error\": \"%s\"", e.status, e.what());
  }
  LeafPlan L;
  if (!leafify(p, L)) {
    j.s += ", \"leaf\": null}";
    return give(j.s, out, cap);
  }
  j.s += ", \"leaf\": {\"leaves\": [";
  for (size_t k = 0; k < L.leaves.size(); ++k) {
    const FilterLeaf& f = L.leaves[k];
    j.s += fmt("%s{\"col\": %d, \"op\": %d, \"lit\": %d, \"nlit\": %d, \"lit_null\": %d, \"pad\": %d}", k ? ", " : "", f.col, f.op,
               f.lit, f.nlit, f.lit_null, f.pad);
  }
  j.s += "], ";
  j.ints("prog", L.prog.begin(), L.prog.end());
  j.s += ", ";
  j.ints("i64", L.i64.begin(), L.i64.end());
  j.s += ", ";
  j.ints("i64hi", L.i64hi.begin(), L.i64hi.end());
  j.s += ", \"str\": [";
  for (size_t k = 0; k < L.str.size(); ++k) {
    j.s += k ? ", " : "";
    j.hex(reinterpret_cast<const uint8_t*>(L.str[k].data()), L.str[k].size());
  }
  j.s += "]}}";
  return give(j.s, out, cap);
}

}  // extern "C"
