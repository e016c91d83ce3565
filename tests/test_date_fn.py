"""The K5 date functions (delta_amd/csrc/date_fn.h), host build, held to Python's datetime.date -- like
java.time.LocalDate a proleptic Gregorian calendar, with the same ISO-8601 week rule -- for years
1..9999, and beyond them to the calendar's exact period of 400 years = 146,097 days = 0 mod 7."""
import ctypes as C
import datetime as dt
import os
import random
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "delta_amd", "csrc", "date_fn.h")
SRC = os.path.join(ROOT, "tests", "native", "date_fn_host.cpp")
LIB = os.path.join(ROOT, "build", "libdatefn_host.so")
YEAR, QUARTER, MONTH, DAYOFMONTH, DAYOFWEEK, DAYOFYEAR, WEEKOFYEAR, TO_DATE, DATE_ADD, TRUNC = range(19, 29)
TY, TQ, TM, TW = 0, 1, 2, 3
EPOCH_ORD = dt.date(1970, 1, 1).toordinal()
MIN_DAY, MAX_DAY = dt.date.min.toordinal() - EPOCH_ORD, dt.date.max.toordinal() - EPOCH_ORD
PERIOD = 146097
# (fn, arg) in the order of `expected_row`
FUNCS = [(YEAR, 0), (QUARTER, 0), (MONTH, 0), (DAYOFMONTH, 0), (DAYOFWEEK, 0), (DAYOFYEAR, 0), (WEEKOFYEAR, 0),
         (TRUNC, TY), (TRUNC, TQ), (TRUNC, TM), (TRUNC, TW)]


@pytest.fixture(scope="module")
def lib():
    deps = [SRC, HDR, os.path.join(ROOT, "delta_amd", "csrc", "filter_plan.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in deps):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O2", "-fPIC", "-shared", "-o", LIB, SRC])
    return C.CDLL(LIB)


def apply(lib, fn, arg, values):
    a = np.ascontiguousarray(values, dtype=np.int64)
    out = np.empty_like(a)
    lib.dfh_apply(C.c_int32(fn), C.c_int32(arg), a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                  C.c_int64(len(a)))
    return out


def expected_row(days):
    """The eleven values of FUNCS for a day count within datetime's range, from datetime alone."""
    d = dt.date.fromordinal(days + EPOCH_ORD)
    q = (d.month - 1) // 3 + 1
    jan1 = dt.date(d.year, 1, 1).toordinal()
    return (d.year, q, d.month, d.day, d.isoweekday() % 7 + 1, d.toordinal() - jan1 + 1, d.isocalendar()[1],
            jan1 - EPOCH_ORD, dt.date(d.year, 3 * q - 2, 1).toordinal() - EPOCH_ORD,
            dt.date(d.year, d.month, 1).toordinal() - EPOCH_ORD, days - d.weekday())


def check_days(lib, days):
    days = np.asarray(days, dtype=np.int64)
    want = np.array([expected_row(int(x)) for x in days], dtype=np.int64)
    for k, (fn, arg) in enumerate(FUNCS):
        got = apply(lib, fn, arg, days)
        bad = np.nonzero(got != want[:, k])[0]
        assert bad.size == 0, (fn, arg, int(days[bad[0]]), int(got[bad[0]]), int(want[bad[0], k]))


def test_every_day_of_1896_to_2104(lib):
    """The century rules of 1900, 2000 and 2100 and every leap pattern."""
    lo, hi = dt.date(1896, 1, 1).toordinal() - EPOCH_ORD, dt.date(2104, 12, 31).toordinal() - EPOCH_ORD
    check_days(lib, np.arange(lo, hi + 1))


def test_forty_days_around_every_new_year(lib):
    """Every ISO week-1 / week-52 / week-53 boundary of the years 1..9999."""
    days = set()
    for y in range(1, 10000):
        j = dt.date(y, 1, 1).toordinal() - EPOCH_ORD
        days.update(range(max(j - 40, MIN_DAY), min(j + 40, MAX_DAY) + 1))
    check_days(lib, sorted(days))


def test_period_rule_beyond_datetime(lib):
    """Outside 0001..9999: the values at `days` and at `days - 146097 k` agree, the year being 400 k and a
    truncation 146097 k further on."""
    rng = random.Random(20241)
    days = [rng.randrange(-2 * 10 ** 9 + 1, -719163) for _ in range(2000)] + \
           [rng.randrange(2932897 + 1, 2 * 10 ** 9) for _ in range(2000)]
    assert all(not MIN_DAY <= x <= MAX_DAY for x in days)
    mid = dt.date(4000, 1, 1).toordinal() - EPOCH_ORD  # shifted near here: truncations stay within range
    ks = [(x - mid) // PERIOD for x in days]
    base = [x - PERIOD * k for x, k in zip(days, ks)]
    assert all(MIN_DAY + 400 < b < MAX_DAY - 400 for b in base)
    k = np.array(ks, dtype=np.int64)
    shift = {YEAR: 400 * k, TRUNC: PERIOD * k}
    for fn, arg in FUNCS:
        got, near = apply(lib, fn, arg, days), apply(lib, fn, arg, base)
        assert np.array_equal(got, near + shift.get(fn, 0)), (fn, arg)
    check_days(lib, base)


# days, date, year, quarter, month, day, dow, doy, week, trunc Y, trunc Q, trunc M, trunc W
ANCHORS = [
    (0, "1970-01-01", 1970, 1, 1, 1, 5, 1, 1, 0, 0, 0, -3),
    (-1, "1969-12-31", 1969, 4, 12, 31, 4, 365, 1, -365, -92, -31, -3),
    (11016, "2000-02-29", 2000, 1, 2, 29, 3, 60, 9, 10957, 10957, 10988, 11015),
    (-25508, "1900-03-01", 1900, 1, 3, 1, 5, 60, 9, -25567, -25567, -25508, -25511),
    (18627, "2020-12-31", 2020, 4, 12, 31, 5, 366, 53, 18262, 18536, 18597, 18624),
    (18630, "2021-01-03", 2021, 1, 1, 3, 1, 3, 53, 18628, 18628, 18628, 18624),
    (18631, "2021-01-04", 2021, 1, 1, 4, 2, 4, 1, 18628, 18628, 18628, 18631),
    (17896, "2018-12-31", 2018, 4, 12, 31, 2, 365, 1, 17532, 17805, 17866, 17896),
    (20819, "2027-01-01", 2027, 1, 1, 1, 6, 1, 53, 20819, 20819, 20819, 20815),
    (-141432, "1582-10-10", 1582, 4, 10, 10, 1, 283, 40, -141714, -141441, -141441, -141438),
    (-719162, "0001-01-01", 1, 1, 1, 1, 2, 1, 1, -719162, -719162, -719162, -719162),
    (2932896, "9999-12-31", 9999, 4, 12, 31, 6, 365, 52, 2932532, 2932805, 2932866, 2932892),
]


def test_anchors(lib):
    for row in ANCHORS:
        days, text, want = row[0], row[1], row[2:]
        y, m, d = (int(x) for x in text.split("-"))
        assert dt.date(y, m, d).toordinal() - EPOCH_ORD == days, text
        assert expected_row(days) == want, text
        got = tuple(int(apply(lib, fn, arg, [days])[0]) for fn, arg in FUNCS)
        assert got == want, text


def test_civil_from_days(lib):
    days = np.array([r[0] for r in ANCHORS] + [MIN_DAY, MAX_DAY, -2 ** 31, 2 ** 31 - 1], dtype=np.int64)
    out = np.empty(5 * len(days), dtype=np.int64)
    lib.dfh_civil(days.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_int64(len(days)))
    out = out.reshape(-1, 5)
    for x, (y, m, d, doy, leap) in zip(days[:-2], out[:-2]):
        w = dt.date.fromordinal(int(x) + EPOCH_ORD)
        assert (y, m, d) == (w.year, w.month, w.day) and doy == w.timetuple().tm_yday
        assert bool(leap) == (w.year % 4 == 0 and (w.year % 100 != 0 or w.year % 400 == 0))
    # the ends of the int32 range (java.time.LocalDate.ofEpochDay(Integer.MIN_VALUE / MAX_VALUE))
    assert tuple(out[-2][:3]) == (-5877641, 6, 23) and tuple(out[-1][:3]) == (5881580, 7, 11)


def test_to_date_floors(lib):
    micros = [-1, 0, 86_399_999_999, 86_400_000_000, -86_400_000_001, -86_400_000_000, 2 ** 63 - 1, -2 ** 63]
    want = [-1, 0, 0, 1, -2, -1, (2 ** 63 - 1) // 86_400_000_000, (-2 ** 63) // 86_400_000_000]
    assert apply(lib, TO_DATE, 0, micros).tolist() == want


def test_date_add_wraps_at_32_bits(lib):
    assert apply(lib, DATE_ADD, 1, [2 ** 31 - 1, 0, -1]).tolist() == [-2 ** 31, 1, 0]
    assert apply(lib, DATE_ADD, -1, [-2 ** 31, 0]).tolist() == [2 ** 31 - 1, -1]
    assert apply(lib, DATE_ADD, -2 ** 31, [0, -1]).tolist() == [-2 ** 31, 2 ** 31 - 1]
    assert apply(lib, DATE_ADD, 7, [18627]).tolist() == [18634]
