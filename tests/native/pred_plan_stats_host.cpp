// Stand-alone driver of delta_amd/csrc/pred_plan.cpp over predicate columns with a source (DR_SRC_*),
// built by tests/test_pred_plan_stats.py with -fsanitize=address,undefined and run as it is. Every case
// is one line of stdin: `ncols {type name-as-hex|-}... nops {opcode arg}... nlits {type i64}...`; the
// answer is one line `status|text|leafified leaves nprog|lowered ops`.
#include "../../delta_amd/csrc/pred_plan.h"

#include <cstdio>
#include <iostream>
#include <sstream>

using namespace dr;

static std::string unhex(const std::string& h) {
  std::string out;
  if (h == "-") return out;
  for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back(char(std::stoi(h.substr(i, 2), nullptr, 16)));
  return out;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    int ncols = 0, nops = 0, nlits = 0;
    in >> ncols;
    std::vector<int32_t> types(size_t(ncols) + 1);
    std::vector<std::string> names(size_t(ncols) + 1);
    std::vector<const char*> name_ptrs(size_t(ncols) + 1);
    for (int c = 0; c < ncols; ++c) {
      std::string h;
      in >> types[size_t(c)] >> h;
      names[size_t(c)] = unhex(h);
    }
    for (int c = 0; c < ncols; ++c) name_ptrs[size_t(c)] = names[size_t(c)].c_str();
    in >> nops;
    std::vector<dr_pred_op> ops(size_t(nops) + 1);
    for (int k = 0; k < nops; ++k) in >> ops[size_t(k)].opcode >> ops[size_t(k)].arg;
    in >> nlits;
    std::vector<int32_t> lt(size_t(nlits) + 1);
    std::vector<int64_t> li(size_t(nlits) + 1), lo(size_t(nlits) + 2, 0);
    std::vector<uint8_t> ln(size_t(nlits) + 1, 0), bytes(1, 0);
    for (int k = 0; k < nlits; ++k) in >> lt[size_t(k)] >> li[size_t(k)];
    dr_predicate p{nops, ops.data(), ncols, name_ptrs.data(), types.data(), nlits, lt.data(), li.data(), ln.data(), lo.data(), bytes.data()};
    try {
      check_program(p);
      LeafPlan L;
      const bool leaf = leafify(p, L);
      const std::vector<int32_t> low = lower_program(p);
      printf("0||%d %zu %zu|%zu\n", leaf ? 1 : 0, leaf ? L.leaves.size() : size_t(0), leaf ? L.prog.size() / 2 : size_t(0), low.size() / 2);
    } catch (const Error& e) {
      printf("%d|%s||\n", int(e.status), e.what());
    }
  }
  return 0;
}
