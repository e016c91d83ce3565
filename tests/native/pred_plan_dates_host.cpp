// Host build of the K5 predicate planner (delta_amd/csrc/pred_plan.cpp) for tests/test_pred_plan_dates.py:
// like pred_plan_host.cpp, with the function chain of every leaf (FilterLeaf's appended fields) in
// the JSON text.
#include "../../delta_amd/csrc/pred_plan.h"

#include <cstring>

using namespace dr;

namespace {

template <typename It>
std::string ints(const char* key, It b, It e) {
  std::string s = fmt("\"%s\": [", key);
  for (It i = b; i != e; ++i) s += (i == b ? "" : ", ") + std::to_string((long long)*i);
  return s + "]";
}

}  // namespace

extern "C" {

// what the tests name of filter_plan.h and of FilterLeaf's layout: an aggregate initialiser of the
// first six fields must leave "no function"
void ppd_constants(int32_t out[3]) {
  const FilterLeaf six{7, DR_OP_EQ, 1, 2, 3, 4};
  out[0] = FL_MAXFN;
  out[1] = six.nfn;
  out[2] = int32_t(sizeof(FilterLeaf));
}

// check_program's verdict: 0, or the status with the message in msg.
int ppd_check(const dr_predicate* p, char* msg, uint32_t cap) {
  msg[0] = 0;
  try {
    check_program(*p);
  } catch (const Error& e) {
    std::strncpy(msg, e.what(), cap - 1);
    msg[cap - 1] = 0;
    return e.status;
  }
  return 0;
}

// The plan of a program that passes check_program: lower_program's pairs and, when leafify takes the
// program, its leaves with their chains (`leaf`: null otherwise). Returns 0, check_program's status,
// or -1 when `out` is too small.
int ppd_plan(const dr_predicate* p, char* out, uint32_t cap) {
  try {
    check_program(*p);
  } catch (const Error& e) {
    return e.status;
  }
  std::string s = "{";
  try {
    const std::vector<int32_t> low = lower_program(*p);
    s += ints("lowered", low.begin(), low.end());
  } catch (const Error& e) {
    s += "\"lowered\": null";
  }
  LeafPlan L;
  if (!leafify(*p, L)) {
    s += ", \"leaf\": null}";
  } else {
    s += ", \"leaf\": {\"leaves\": [";
    for (size_t k = 0; k < L.leaves.size(); ++k) {
      const FilterLeaf& f = L.leaves[k];
      s += fmt("%s{\"col\": %d, \"op\": %d, \"lit\": %d, \"nlit\": %d, \"lit_null\": %d, \"pad\": %d, \"fns\": [", k ? ", " : "", f.col,
               f.op, f.lit, f.nlit, f.lit_null, f.pad);
      for (int32_t q = 0; q < f.nfn; ++q) s += fmt("%s[%d, %d]", q ? ", " : "", f.fn[q], f.farg[q]);
      s += "]}";
    }
    s += "], " + ints("prog", L.prog.begin(), L.prog.end()) + ", " + ints("i64", L.i64.begin(), L.i64.end()) + "}}";
  }
  if (s.size() + 1 > cap) return -1;
  std::memcpy(out, s.c_str(), s.size() + 1);
  return 0;
}

}  // extern "C"
