// K5 date functions (DR_OP_YEAR .. DR_OP_TRUNC_DATE of include/deltareplay.h): Spark 3.1's Year,
// Quarter, Month, DayOfMonth, DayOfWeek, DayOfYear, WeekOfYear, Cast(timestamp AS date), DateAdd and
// TruncDate as pure integer functions of a day count (days since 1970-01-01 in the proleptic
// Gregorian calendar of java.time.LocalDate.ofEpochDay) or of microseconds since the epoch (UTC).
// One source for the three evaluators of k_filter.hip and for the host (tests/native/date_fn_host.cpp):
// no HIP type, g++ compiles it alone. Every function is total; 64-bit arithmetic throughout, exact for
// every int32 day count (about +-5.8 M years), no table and no loop per year.
#pragma once
#include <cstdint>

#include "filter_plan.h"

namespace dr {
namespace df {

// the function codes are the ABI's opcodes (pred_plan.cpp asserts it)
enum : int32_t { FN_YEAR = 19, FN_QUARTER = 20, FN_MONTH = 21, FN_DAYOFMONTH = 22, FN_DAYOFWEEK = 23, FN_DAYOFYEAR = 24,
                 FN_WEEKOFYEAR = 25, FN_TO_DATE = 26, FN_DATE_ADD = 27, FN_TRUNC_DATE = 28 };
enum : int32_t { TRUNC_YEAR = 0, TRUNC_QUARTER = 1, TRUNC_MONTH = 2, TRUNC_WEEK = 3 };
constexpr int64_t MICROS_PER_DAY = 86400000000ll;

DR_HD inline int64_t floor_div(int64_t a, int64_t b) { return a / b - ((a % b != 0) && ((a % b < 0) != (b < 0))); }
DR_HD inline int64_t floor_mod(int64_t a, int64_t b) { return a - floor_div(a, b) * b; }

struct Civil {
  int64_t year;
  int32_t month, day;  // 1..12, 1..31
  int32_t doy;         // 1..366, from 1 January
  int32_t leap;        // the year has a 29 February
};

// The date of a day count: eras of 400 years (146 097 days) from 0000-03-01, the year beginning in
// March so that the leap day is its last.
DR_HD inline Civil civil_from_days(int64_t days) {
  const int64_t z = days + 719468;
  const int64_t era = floor_div(z, 146097);
  const int64_t doe = z - era * 146097;                                        // [0, 146096]
  const int64_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;   // [0, 399]
  const int64_t dom = doe - (365 * yoe + yoe / 4 - yoe / 100);                 // day of the March year, [0, 365]
  const int64_t mp = (5 * dom + 2) / 153;                                      // [0, 11], 0 = March
  Civil c;
  c.day = int32_t(dom - (153 * mp + 2) / 5 + 1);
  c.month = int32_t(mp < 10 ? mp + 3 : mp - 9);
  c.year = yoe + era * 400 + (c.month <= 2);
  c.leap = (c.year % 4 == 0 && c.year % 100 != 0) || c.year % 400 == 0;
  // January and February close the March year (from its day 306)
  c.doy = int32_t(dom >= 306 ? dom - 305 : dom + 60 + c.leap);
  return c;
}

DR_HD inline int64_t year(int64_t days) { return civil_from_days(days).year; }
DR_HD inline int64_t quarter(int64_t days) { return (civil_from_days(days).month - 1) / 3 + 1; }
DR_HD inline int64_t month(int64_t days) { return civil_from_days(days).month; }
DR_HD inline int64_t day_of_month(int64_t days) { return civil_from_days(days).day; }
DR_HD inline int64_t day_of_year(int64_t days) { return civil_from_days(days).doy; }
// Sunday = 1 .. Saturday = 7 (1970-01-01 was a Thursday)
DR_HD inline int64_t day_of_week(int64_t days) { return floor_mod(days + 4, 7) + 1; }
// The Monday on or before
DR_HD inline int64_t trunc_week(int64_t days) { return days - floor_mod(days + 3, 7); }
// ISO-8601: a week belongs to the year of its Thursday, and is that Thursday's week of the year
DR_HD inline int64_t week_of_year(int64_t days) { return (civil_from_days(trunc_week(days) + 3).doy - 1) / 7 + 1; }
// Cast(timestamp AS date), zone UTC
DR_HD inline int64_t to_date(int64_t micros) { return floor_div(micros, MICROS_PER_DAY); }
// Int + Int, non-ANSI: wraps
DR_HD inline int64_t date_add(int64_t days, int32_t n) { return int64_t(int32_t(uint32_t(days) + uint32_t(n))); }
// The first day of the year / quarter / month, the Monday on or before; `unit` outside 0..3 (refused
// by check_program) reads as WEEK
DR_HD inline int64_t trunc_date(int64_t days, int32_t unit) {
  if (unit != TRUNC_YEAR && unit != TRUNC_QUARTER && unit != TRUNC_MONTH) return trunc_week(days);
  const Civil c = civil_from_days(days);
  if (unit == TRUNC_MONTH) return days - (c.day - 1);
  if (unit == TRUNC_YEAR) return days - (c.doy - 1);
  // 1 January, 1 April, 1 July, 1 October as days of the year
  const int32_t q = (c.month - 1) / 3;
  const int32_t first = q == 0 ? 1 : (q == 1 ? 91 : q == 2 ? 182 : 274) + c.leap;
  return days - (c.doy - first);
}

// Function `fn` (an opcode DR_OP_YEAR .. DR_OP_TRUNC_DATE) with its op's `arg` on a non-NULL value: a day
// count, for FN_TO_DATE microseconds. Any other code gives the value back.
DR_HD inline int64_t date_fn(int32_t fn, int32_t arg, int64_t v) {
  switch (fn) {
    case FN_YEAR: return year(v);
    case FN_QUARTER: return quarter(v);
    case FN_MONTH: return month(v);
    case FN_DAYOFMONTH: return day_of_month(v);
    case FN_DAYOFWEEK: return day_of_week(v);
    case FN_DAYOFYEAR: return day_of_year(v);
    case FN_WEEKOFYEAR: return week_of_year(v);
    case FN_TO_DATE: return to_date(v);
    case FN_DATE_ADD: return date_add(v, arg);
    case FN_TRUNC_DATE: return trunc_date(v, arg);
    default: return v;
  }
}

}  // namespace df
}  // namespace dr
