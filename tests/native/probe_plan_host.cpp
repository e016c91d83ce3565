// Stand-alone driver of dr_state_probe_keys' host side (delta_amd/csrc/pred_plan.cpp: check_probe_args,
// check_probe_rows; delta_amd/csrc/filter_plan.h: probe_order_key, the function the kernel calls as well),
// built by tests/test_probe_plan.py with -fsanitize=address,undefined and run as it is. One case a line:
//   A hasrows nrows lo_type lo_name hi_type hi_name haskeys nkeys flags    names as hex, `-` for "", `0` for NULL
//   R side nrows {row}...
//   K base word                                                             the order key of an int64 word
// The answer is one line `status|text`; K answers `0|key`.
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
      if (kind == "A") {
        int hasrows = 0, haskeys = 0;
        long long nrows = 0, nkeys = 0;
        int32_t lo_type = 0, hi_type = 0;
        unsigned flags = 0;
        std::string lo_h, hi_h;
        in >> hasrows >> nrows >> lo_type >> lo_h >> hi_type >> hi_h >> haskeys >> nkeys >> flags;
        const std::string lo = lo_h == "0" ? std::string() : unhex(lo_h), hi = hi_h == "0" ? std::string() : unhex(hi_h);
        const int64_t one_key = 0;  // never read: the checks look at the pointer alone
        check_probe_args(hasrows != 0, nrows, lo_h == "0" ? nullptr : lo.c_str(), lo_type, hi_h == "0" ? nullptr : hi.c_str(),
                         hi_type, haskeys ? &one_key : nullptr, nkeys, flags);
      } else if (kind == "R") {
        unsigned long long side = 0;
        long long nrows = 0;
        in >> side >> nrows;
        std::vector<int64_t> rows(nrows > 0 ? size_t(nrows) : 0);
        for (auto& r : rows) in >> r;
        rows.push_back(0);  // never empty
        check_probe_rows(rows.data(), nrows, side);
      } else if (kind == "K") {
        int32_t base = 0;
        long long word = 0;
        in >> base >> word;
        printf("0|%lld\n", (long long)probe_order_key(base, word));
        continue;
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
