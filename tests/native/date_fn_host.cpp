// Host build of the K5 date functions for tests/test_date_fn.py: date_fn.h is included first and alone,
// so this file also shows that g++ compiles the header with nothing before it.
#include "../../delta_amd/csrc/date_fn.h"

extern "C" {

// out[i] = date_fn(fn, arg, in[i])
void dfh_apply(int32_t fn, int32_t arg, const int64_t* in, int64_t* out, int64_t n) {
  for (int64_t i = 0; i < n; ++i) out[i] = dr::df::date_fn(fn, arg, in[i]);
}

// year, month, day, day of the year and leap flag of civil_from_days(days[i]), five values per day
void dfh_civil(const int64_t* days, int64_t* out, int64_t n) {
  for (int64_t i = 0; i < n; ++i) {
    const dr::df::Civil c = dr::df::civil_from_days(days[i]);
    out[5 * i] = c.year;
    out[5 * i + 1] = c.month;
    out[5 * i + 2] = c.day;
    out[5 * i + 3] = c.doy;
    out[5 * i + 4] = c.leap;
  }
}

}  // extern "C"
