// Stand-alone driver of dr_state_aggregate's host checks (delta_amd/csrc/pred_plan.cpp: check_agg_specs,
// check_agg_selection) and of check_column_source as a predicate column meets it, built by
// tests/test_agg_plan.py with -fsanitize=address,undefined and run as it is. Every case is one line of stdin:
//   S naggs {fn input type name}...      name as hex, `-` for "", `0` for a NULL pointer; naggs < 0 or
//                                        `S n null`: aggs == NULL with naggs = n
//   R side hasrows nrows {row}... hasgroups ngroups {offset}...   (max(ngroups, 0) + 1 offsets)
//   C type name c                        check_column_source(name, type, c)
// The answer is one line `status|text`.
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
    std::string kind;
    in >> kind;
    try {
      if (kind == "S") {
        int naggs = 0;
        in >> naggs;
        std::vector<std::string> tok;
        for (std::string t; in >> t;) tok.push_back(t);
        if (!tok.empty() && tok[0] == "null") {
          check_agg_specs(nullptr, naggs);
        } else {
          const size_t n = tok.size() / 4;  // (as many as the line holds: naggs itself may be out of range)
          std::vector<dr_agg_spec> specs(n + 1);
          std::vector<std::string> names(n + 1);
          std::vector<bool> null_name(n + 1, false);
          for (size_t a = 0; a < n; ++a) {
            specs[a].fn = std::stoi(tok[4 * a]);
            specs[a].input = std::stoi(tok[4 * a + 1]);
            specs[a].type_with_source = std::stoi(tok[4 * a + 2]);
            const std::string& h = tok[4 * a + 3];
            null_name[a] = h == "0";
            names[a] = null_name[a] ? std::string() : unhex(h);
          }
          for (size_t a = 0; a < n; ++a) specs[a].name = null_name[a] ? nullptr : names[a].c_str();
          check_agg_specs(specs.data(), naggs);
        }
      } else if (kind == "R") {
        unsigned long long side = 0;
        int hasrows = 0, hasgroups = 0;
        long long nrows = 0, ngroups = 0;
        in >> side >> hasrows >> nrows;
        std::vector<int64_t> rows(nrows > 0 ? size_t(nrows) : 0);
        for (auto& r : rows) in >> r;
        in >> hasgroups >> ngroups;
        std::vector<int64_t> off((ngroups > 0 ? size_t(ngroups) : 0) + 1);
        for (auto& o : off) in >> o;
        rows.push_back(0);  // (never empty: data() of an empty vector may be a null pointer, which means "all")
        check_agg_selection(hasrows ? rows.data() : nullptr, nrows, side, hasgroups ? off.data() : nullptr, ngroups);
      } else if (kind == "C") {
        int32_t type = 0, c = 0;
        std::string h;
        in >> type >> h >> c;
        const std::string name = unhex(h);
        check_column_source(name.c_str(), type, c);
      } else {
        printf("-1|unknown case %s\n", kind.c_str());
        continue;
      }
      printf("0|\n");
    } catch (const Error& e) {
      printf("%d|%s\n", int(e.status), e.what());
    }
  }
  return 0;
}
