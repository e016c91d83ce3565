"""Partition-pruning corpus for the date functions of K5 (DR_OP_YEAR .. DR_OP_TRUNC_DATE): one table of
415 live files partitioned by `dt date`, `ts timestamp` and `k integer`, whose dates sit where a
calendar function goes wrong -- the epoch and the day before, century years, both sides of the ISO
year boundaries, 29 February, year 0001 and year 9999, NULL and text that casts to NULL -- and whose
timestamps straddle midnight UTC on both sides of the epoch.

The oracle has no such functions, so the expected values come from here: every function is computed
from Python's datetime.date (a proleptic Gregorian calendar, like java.time.LocalDate, with the same
ISO-8601 week rule) and the predicate tree is walked with Spark's three-valued logic. Nothing here
calls the device or reads date_fn.h."""
import datetime as dt
import json
import os

from delta_amd.testing import synth as S
from oracle import delta_oracle as O

PTYPES = {"dt": "date", "ts": "timestamp", "k": "integer"}
SCHEMA = {"type": "struct", "fields": [{"name": "id", "type": "long", "nullable": True, "metadata": {}}] + [
    {"name": c, "type": t, "nullable": True, "metadata": {}} for c, t in PTYPES.items()]}
METADATA = {"id": "filter-dates-corpus", "format": {"provider": "parquet", "options": {}},
            "schemaString": json.dumps(SCHEMA, separators=(",", ":")), "partitionColumns": list(PTYPES),
            "configuration": {}, "createdTime": 1600000000000}
PROTOCOL = {"minReaderVersion": 1, "minWriterVersion": 2}
EPOCH_ORD = dt.date(1970, 1, 1).toordinal()
MICROS_PER_DAY = 86_400_000_000

ANCHORS = ["1970-01-01", "1969-12-31", "2000-02-29", "1900-03-01", "2020-12-31", "2021-01-03", "2021-01-04", "2018-12-31",
           "2027-01-01", "1582-10-10", "0001-01-01", "9999-12-31"]


def _dates():
    out = []
    for a in ANCHORS:  # each anchor and its neighbours
        o = dt.date.fromisoformat(a).toordinal()
        out += [dt.date.fromordinal(x).isoformat() for x in (o - 1, o, o + 1) if dt.date.min.toordinal() <= x <= dt.date.max.toordinal()]
    for y in (2015, 2018, 2020, 2026):  # both sides of the ISO year boundary y / y + 1
        o = dt.date(y + 1, 1, 1).toordinal()
        out += [dt.date.fromordinal(x).isoformat() for x in range(o - 5, o + 5)]
    out += ["2000-02-29", "2024-02-29", "2024-03-01", "2024-03-15", "2024-03-31", "2024-04-01", "2023-02-28", "2100-02-28", "2100-03-01",
            "0001-06-15", "9999-06-15", "2024-3-7", " 2024-07-04 ",
            None, "2024-02-30", "not-a-date", ""]  # NULL, and text that casts to NULL
    seen, uniq = set(), []
    for v in out:
        if v not in seen:
            seen.add(v)
            uniq.append(v)
    return uniq


DT_VALUES = _dates()
TS_VALUES = [
    "1970-01-01 00:00:00", "1969-12-31 23:59:59.999999", "1970-01-01 23:59:59.999999", "1970-01-02 00:00:00",
    "1969-12-31 00:00:00", "1969-12-30 23:59:59.999999", "1970-01-01 00:00:00.000001", "2024-02-29 23:59:59.999999",
    "2024-03-01 00:00:00", "2024-03-01 00:30:00+01:00", "2020-12-31 23:59:59", "2021-01-01 00:00:00", "2021-01-03 12:00:00",
    "1900-02-28 23:59:59.5", "1900-03-01 00:00:00", "0001-01-01 00:00:00", "9999-12-31 23:59:59.999999", None, "yesterday",
]
N_ADDS = 440  # adds written; every 9th of the first half is removed again
N_LIVE = 415


def _pv(i):
    return {"dt": DT_VALUES[i % len(DT_VALUES)], "ts": TS_VALUES[(i * 7 + 3) % len(TS_VALUES)], "k": str(i % 13)}


def _add(i):
    return {"path": "f-%05d.parquet" % i, "partitionValues": _pv(i), "size": 100 + i, "modificationTime": 1600000000000 + i,
            "dataChange": True, "stats": None}


def live_indices():
    removed = set(range(0, N_ADDS // 2, 9))
    return [i for i in range(N_ADDS) if i not in removed]


def live_files():
    return [_add(i) for i in live_indices()]


def build(table_dir, checkpoint=False):
    """Returns the _delta_log path of the table. v0: protocol, metadata, the first half of the adds;
    v1: removes every 9th of those and adds most of the rest; v2: the last 30 adds. With `checkpoint`, a
    checkpoint of the v1 state: its files' values are then read from the checkpoint's partitionValues
    map column, the last 30 from JSON."""
    log = os.path.join(table_dir, "_delta_log")
    os.makedirs(log, exist_ok=True)
    n, h = N_ADDS, N_ADDS // 2
    removed = list(range(0, h, 9))
    assert len(live_indices()) == n - len(removed) == N_LIVE
    line = lambda a: json.dumps(a, separators=(",", ":"))  # noqa: E731
    with open(os.path.join(log, "%020d.json" % 0), "w", encoding="utf-8") as f:
        f.write(line({"protocol": PROTOCOL}) + "\n" + line({"metaData": METADATA}) + "\n")
        for i in range(h):
            f.write(line({"add": _add(i)}) + "\n")
    with open(os.path.join(log, "%020d.json" % 1), "w", encoding="utf-8") as f:
        for i in removed:
            f.write(line({"remove": {"path": "f-%05d.parquet" % i, "deletionTimestamp": 1600000001000, "dataChange": True}}) + "\n")
        for i in range(h, n - 30):
            f.write(line({"add": _add(i)}) + "\n")
    with open(os.path.join(log, "%020d.json" % 2), "w", encoding="utf-8") as f:
        for i in range(n - 30, n):
            f.write(line({"add": _add(i)}) + "\n")
    if checkpoint:
        live = [_add(i) for i in live_indices() if i < n - 30]
        S.write_checkpoint_records(os.path.join(log, "%020d.checkpoint.parquet" % 1), PROTOCOL, METADATA, live,
                                   row_group_size=150, use_dictionary=True)
        with open(os.path.join(log, "_last_checkpoint"), "w") as f:
            f.write('{"version":1,"size":%d}\n' % (len(live) + 2))
    return log


# ---- the functions, from datetime -------------------------------------------------------------------------
PERIOD = 146097  # days in 400 years, a multiple of 7: the calendar repeats exactly


def _date(days):
    """(date, k): the date of `days - PERIOD * k`, k = 0 within datetime's years 1..9999; beyond them the
    day is moved by whole periods, which changes the year by 400 k, a truncation by PERIOD * k and
    nothing else."""
    k = 0
    if not dt.date.min.toordinal() <= days + EPOCH_ORD <= dt.date.max.toordinal():
        k = (days - _days(dt.date(4000, 1, 1))) // PERIOD
    return dt.date.fromordinal(days - PERIOD * k + EPOCH_ORD), k


def _days(d):
    return d.toordinal() - EPOCH_ORD


def _wrap32(x):
    return (x + 2 ** 31) % 2 ** 32 - 2 ** 31


TRUNC_UNITS = {"year": "Y", "yyyy": "Y", "yy": "Y", "quarter": "Q", "month": "M", "mm": "M", "mon": "M", "week": "W"}


def date_function(op, v, arg=None):
    """One function on a non-NULL value: a day count, for to_date microseconds."""
    if op == "to_date":
        return v // MICROS_PER_DAY  # floor
    if op == "date_add":
        return _wrap32(v + arg)
    if op == "date_sub":
        return _wrap32(v - arg)
    d, k = _date(v)
    if op == "year":
        return d.year + 400 * k
    if op == "quarter":
        return (d.month - 1) // 3 + 1
    if op == "month":
        return d.month
    if op == "dayofmonth":
        return d.day
    if op == "dayofweek":
        return d.isoweekday() % 7 + 1  # Sunday = 1 .. Saturday = 7
    if op == "dayofyear":
        return d.timetuple().tm_yday
    if op == "weekofyear":
        return d.isocalendar()[1]
    if op == "trunc":
        unit = TRUNC_UNITS[arg.lower()]
        if unit == "W":
            return v - d.weekday()  # the Monday on or before
        first = dt.date(d.year, 1 if unit == "Y" else d.month if unit == "M" else 3 * ((d.month - 1) // 3) + 1, 1)
        return _days(first) + PERIOD * k
    raise ValueError(op)


FUNCTIONS = ("year", "quarter", "month", "dayofmonth", "dayofweek", "dayofyear", "weekofyear", "to_date", "date_add", "date_sub",
             "trunc")


def evaluate(expr, pv, schema=PTYPES):
    """Three-valued evaluation of a predicate tree over one file's partitionValues (None is NULL)."""
    op = expr[0]
    if op == "col":
        field = next(f for f in schema if f.lower() == expr[1].strip("`").lower())
        return O.cast_string((pv or {}).get(field), schema[field])
    if op == "lit":
        if expr[2] is None:
            return None
        if expr[1] == "date":
            return _days(dt.date.fromisoformat(expr[2])) if isinstance(expr[2], str) else int(expr[2])
        return expr[2]
    if op in FUNCTIONS:
        a = evaluate(expr[1], pv, schema)
        return None if a is None else date_function(op, a, *expr[2:])
    if op in ("=", "!=", "<", "<=", ">", ">="):
        a, b = evaluate(expr[1], pv, schema), evaluate(expr[2], pv, schema)
        if a is None or b is None:
            return None
        return {"=": a == b, "!=": a != b, "<": a < b, "<=": a <= b, ">": a > b, ">=": a >= b}[op]
    if op == "<=>":
        a, b = evaluate(expr[1], pv, schema), evaluate(expr[2], pv, schema)
        return a == b  # None == None: both NULL
    if op in ("isnull", "isnotnull"):
        return (evaluate(expr[1], pv, schema) is None) == (op == "isnull")
    if op == "in":
        a = evaluate(expr[1], pv, schema)
        vals = [evaluate(x, pv, schema) for x in expr[2]]
        if a is None:
            return None
        return True if a in [v for v in vals if v is not None] else (None if None in vals else False)
    if op == "not":
        a = evaluate(expr[1], pv, schema)
        return None if a is None else (not a)
    a, b = evaluate(expr[1], pv, schema), evaluate(expr[2], pv, schema)
    if op == "and":
        return False if (a is False or b is False) else (None if (a is None or b is None) else True)
    if op == "or":
        return True if (a is True or b is True) else (None if (a is None or b is None) else False)
    raise ValueError(op)


def expected(files, preds, schema=PTYPES):
    """The files `preds` (ANDed) select: those where every conjunct is TRUE."""
    return [f for f in files if all(evaluate(e, f["partitionValues"], schema) is True for e in preds)]


# ---- the predicates ---------------------------------------------------------------------------------------
C = lambda n: ("col", n)  # noqa: E731
L = lambda t, v: ("lit", t, v)  # noqa: E731
INT = lambda v: L("integer", v)  # noqa: E731
DATE = lambda v: L("date", v)  # noqa: E731
K = lambda op, v: (op, C("k"), INT(v))  # noqa: E731
DT, TS = C("dt"), C("ts")

# every function with the literal type of its result, a value it takes on the corpus (for = and <) and an
# IN list; the eight-element lists are bitmaps in the leaf plan, the shorter ones sorted sets
INT_FUNCS = [
    (("year", DT), INT, 2020, [2020, 1, 9999, 1969]),
    (("quarter", DT), INT, 4, [1, 4]),
    (("month", DT), INT, 3, [1, 2, 3, 5, 7, 8, 10, 12]),
    (("dayofmonth", DT), INT, 31, [1, 29, 31]),
    (("dayofweek", DT), INT, 5, [1, 7]),
    (("dayofyear", DT), INT, 60, [1, 60, 365, 366]),
    (("weekofyear", DT), INT, 53, [1, 52, 53]),
]
DATE_FUNCS = [
    (("to_date", TS), DATE, "1969-12-31", ["1970-01-01", "2024-02-29", "0001-01-01"]),
    (("date_add", DT, 7), DATE, "2021-01-07", ["2021-01-07", "2000-03-07", "1970-01-07"]),
    (("date_sub", DT, 1), DATE, "2020-12-31", ["1969-12-31", "2024-02-29", "1900-02-28"]),
    (("trunc", DT, "YEAR"), DATE, "2021-01-01", ["2021-01-01", "1970-01-01", "1969-01-01"]),
    (("trunc", DT, "quarter"), DATE, "2020-10-01", ["2020-10-01", "2024-01-01"]),
    (("trunc", DT, "MM"), DATE, "2024-03-01", ["2024-%02d-01" % m for m in range(1, 9)]),
    (("trunc", DT, "week"), DATE, "2020-12-28", ["2020-12-28", "1969-12-29", "2018-12-31"]),
]


def _per_function(f, lit, v, vals):
    return [
        [("=", f, lit(v))],
        [("<", f, lit(v))],
        [("in", f, [lit(x) for x in vals])],
        [("in", f, [lit(x) for x in vals] + [lit(None)])],
        [("<=>", f, lit(None))],
        [("isnull", f)],
        [(">=", lit(v), f)],                          # the function on the right of a literal
        [("not", ("=", f, lit(v)))],                  # a NULL value stays NULL under NOT
        [("not", ("in", f, [lit(vals[0]), lit(None)]))],
        [("and", ("!=", f, lit(v)), K("<", 6))],
        [("or", (">", f, lit(v)), ("in", C("k"), [INT(0), INT(12)]))],
    ]


FIVE = ("year", ("date_add", ("trunc", ("date_add", ("to_date", TS), 1), "yy"), -1))  # the generic path
PREDICATES = [p for spec in INT_FUNCS + DATE_FUNCS for p in _per_function(*spec)] + [
    [("=", ("year", ("to_date", TS)), INT(1969))],
    [("in", ("year", ("to_date", TS)), [INT(1970), INT(2024), INT(1)])],
    [("=", ("trunc", ("date_add", DT, -1), "WEEK"), DATE("2020-12-28"))],
    [("<", ("trunc", ("date_add", DT, -1), "WEEK"), DATE("1970-01-01"))],
    [("=", ("dayofweek", ("to_date", TS)), INT(4))],
    [("=", ("year", DT), INT(2024)), ("=", ("month", DT), INT(3))],           # WHERE year(dt) = 2024 AND month(dt) = 3
    [(">=", ("date_add", DT, 7), DATE("2024-03-08")), K("!=", 4)],
    [("=", ("weekofyear", DT), L("long", 1)), ("isnotnull", ("quarter", DT))],
    [("<=>", ("year", DT), ("lit", "short", 1970))],
    [("or", ("isnull", ("year", DT)), ("=", ("year", ("to_date", ("col", "TS"))), INT(9999)))],
    [("=", ("year", ("date_add", ("trunc", ("date_add", DT, 1), "yy"), -1)), INT(2020))],   # four functions: still a leaf
    # the generic path: five functions, a function against a column, against another function
    [("=", FIVE, INT(1969))],
    [("not", ("in", FIVE, [INT(2023), INT(None)]))],
    [("=", ("month", DT), C("k"))],
    [("<", C("k"), ("dayofweek", DT))],
    [("=", ("year", DT), ("year", ("to_date", TS)))],
    [("<=>", ("trunc", DT, "MM"), DT)],
    [("and", ("=", ("month", DT), C("k")), ("=", ("quarter", DT), INT(1)))],
]
