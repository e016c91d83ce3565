"""Partition-pruning corpus over the later partition types -- timestamp, double, float,
decimal(12,2), decimal(38,10) and binary, beside an integer column: one table of 2,113 live files
(two 1,024-file leaf tiles, one 64-file mask word, and one more file) whose values exercise the
casts' edges, and predicates over every comparison, <=>, IN and AND / OR / NOT for each type.

Expected results are the oracle's (`O.filter_file_list`). Python's float comparisons are not
Spark's for NaN, so predicates that read a float / double column -- the table holds NaN rows -- are
evaluated by `spark_eval`, a restatement of the same tree walk with
SQLOrderingUtil.compareDoubles over `O.cast_string` values; nothing else uses it.

A second, small table (`build_years`) holds timestamps whose years Python's datetime cannot hold
(negative, zero, above 9999). The oracle reads those as NULL; Spark and the device do not. Their
expected microseconds come from `cast_timestamp_any_year`, which moves the year by a multiple of
400 into the oracle's range (the proleptic Gregorian calendar repeats every 146,097 days)."""
import json
import os

from delta_amd.testing import synth as S
from oracle import delta_oracle as O

PTYPES = {"ts": "timestamp", "d": "double", "f": "float", "m": "decimal(12,2)", "w": "decimal(38,10)",
          "b": "binary", "part": "integer"}
SCHEMA = {"type": "struct", "fields": [{"name": "id", "type": "long", "nullable": True, "metadata": {}}] + [
    {"name": c, "type": t, "nullable": True, "metadata": {}} for c, t in PTYPES.items()]}
METADATA = {"id": "filter-types-corpus", "format": {"provider": "parquet", "options": {}},
            "schemaString": json.dumps(SCHEMA, separators=(",", ":")), "partitionColumns": list(PTYPES),
            "configuration": {}, "createdTime": 1600000000000}
PROTOCOL = {"minReaderVersion": 1, "minWriterVersion": 2}
N_LIVE = 2113

# zone offsets (two spellings of one instant), fractions (truncated to microseconds), a date and a
# year alone, a time before the epoch, NULL, uncastable text, an impossible date
TS = ["2020-03-01 00:00:00", "2020-03-01T12:30:00.123456", "2020-03-01 12:30:00+02:00", "2020-03-01 10:30:00Z",
      "2019-12-31 23:59:59.999999", "2020-03-01", "2020", None, "not a ts", "2020-02-30 00:00:00",
      " 2020-03-02 01:02:03 ", "1969-12-31 23:59:59-00:30", "2020-03-01 12:30:00.5"]
# NaN and -NaN, the infinities (1e400 overflows to one), both zeros, the smallest subnormal and
# another, more than 19 digits and a hexadecimal significand (converted by the host), d / f suffixes
D = ["1.5", "-1.5", "NaN", "-NaN", "Infinity", "-Infinity", "-0.0", "0.0", "1e400", "4.9e-324", "1e-310",
     "3.14159265358979323846264338", "0x1.8p1", "2.5d", "7f", None, "abc"]
# 0.1 and 16777217 are not binary32 values (the nearest differs from the double), 1e-46 underflows
# to 0, 1e-40 is a binary32 subnormal, 3.4028236e38 rounds past the largest finite value
F = ["0.1", "16777217", "1.5f", "3.4028236e38", "-0.0", "NaN", "1e-46", "1e-40", "2.5", None, "x"]
# HALF_UP at scale 2 (12.345 -> 12.35, -12.345 -> -12.35, -0.005 -> -0.01), overflow of precision 12
# (after rounding, and outright): NULL
M = ["12.345", "12.344", "-12.345", "9999999999.99", "9999999999.995", "1e13", "0", None, "abc", "-0.005"]
# unscaled 2^64 and 2^65 (low words equal, high words differ), 2^63 and 2^63 - 1 (the low word's top
# bit: a signed low-word compare would misplace it), negatives, 38 digits, overflow of precision 38
W = ["-1", "1", "1844674407.3709551616", "3689348814.7419103232", "922337203.6854775808", "922337203.6854775807",
     "-1844674407.3709551616", "1234567890123456789012345678.0123456789", "99999999999999999999999999999.5", None]
# values sharing an 8-byte prefix (one of them the prefix itself), bytes >= 0x80
B = ["prefix12A", "prefix12B", "prefix12", "prefix12é", "é", "", None, "ÿzz", "abc"]


def _pv(i):
    # strides coprime with the list lengths: every value of every column occurs
    return {"ts": TS[i % len(TS)], "d": D[(i * 3 + 1) % len(D)], "f": F[(i * 5 + 2) % len(F)],
            "m": M[(i * 7) % len(M)], "w": W[(i * 3 + 2) % len(W)], "b": B[(i * 5 + 1) % len(B)],
            "part": str(i % 5)}


def _add(i):
    return {"path": "f-%05d.parquet" % i, "partitionValues": _pv(i), "size": 100 + i,
            "modificationTime": 1600000000000 + i, "dataChange": True, "stats": None}


def _line(a):
    return json.dumps(a, separators=(",", ":"), ensure_ascii=bool(len(str(a)) % 2))  # mix raw / \\u escapes


N_ADDS = 2238  # adds written; every 9th of the first half is removed again


def live_indices():
    """The `_add` indices of the table's live files, as `build` leaves them."""
    removed = set(range(0, N_ADDS // 2, 9))
    return [i for i in range(N_ADDS) if i not in removed]


def build(table_dir, checkpoint=False):
    """Returns the _delta_log path of the N_LIVE-file table. v0: protocol, metadata, the first half
    of the adds; v1: removes every 9th of those and adds most of the rest; v2: the last 30 adds.
    With `checkpoint`, a checkpoint of the v1 state: its files' values are then read from the
    checkpoint's partitionValues map column, the last 30 from JSON."""
    log = os.path.join(table_dir, "_delta_log")
    os.makedirs(log, exist_ok=True)
    n = N_ADDS
    h = n // 2
    removed = list(range(0, h, 9))
    assert len(live_indices()) == n - len(removed) == N_LIVE
    with open(os.path.join(log, "%020d.json" % 0), "w") as f:
        for a in [{"protocol": PROTOCOL}, {"metaData": METADATA}] + [{"add": _add(i)} for i in range(h)]:
            f.write(_line(a) + "\n")
    with open(os.path.join(log, "%020d.json" % 1), "w") as f:
        for i in removed:
            f.write(_line({"remove": {"path": "f-%05d.parquet" % i, "deletionTimestamp": 1600000001000,
                                      "dataChange": True}}) + "\n")
        for i in range(h, n - 30):
            f.write(_line({"add": _add(i)}) + "\n")
    with open(os.path.join(log, "%020d.json" % 2), "w") as f:
        for i in range(n - 30, n):
            f.write(_line({"add": _add(i)}) + "\n")
    if checkpoint:
        live = [_add(i) for i in live_indices() if i < n - 30]
        S.write_checkpoint_records(os.path.join(log, "%020d.checkpoint.parquet" % 1), PROTOCOL, METADATA, live,
                                   row_group_size=700, use_dictionary=True)
        with open(os.path.join(log, "_last_checkpoint"), "w") as f:
            f.write('{"version":1,"size":%d}\n' % (len(live) + 2))
    return log


C = lambda n: ("col", n)  # noqa: E731
L = lambda t, v: ("lit", t, v)  # noqa: E731
T = lambda s: L("timestamp", O.cast_string(s, "timestamp"))  # noqa: E731  (microseconds)
DBL = lambda v: L("double", v)  # noqa: E731
FLT = lambda v: L("float", v)  # noqa: E731
M2 = lambda u: L("decimal(12,2)", u)  # noqa: E731  (unscaled)
W10 = lambda u: L("decimal(38,10)", u)  # noqa: E731
BIN = lambda b: L("binary", b)  # noqa: E731
NAN, INF = float("nan"), float("inf")
_US = O.cast_string("2020-03-02 01:02:03", "timestamp")

PREDICATES = [
    # timestamp: microseconds, compared as int64
    [("=", C("ts"), T("2020-03-01 10:30:00Z"))],
    [("!=", C("ts"), T("2020-03-01 10:30:00Z"))],
    [("<", C("ts"), T("2020-03-01"))],
    [("<=", C("ts"), T("2020-03-01"))],
    [(">", C("ts"), T("2020-03-01 12:30:00.123456"))],
    [(">=", C("ts"), T("2020-03-01 12:30:00.123456"))],
    [("<", T("2020-01-01"), C("ts"))],
    [("<=>", C("ts"), L("timestamp", None))],
    [("<=>", C("ts"), T("1970-01-01 00:29:59"))],
    [("isnull", C("TS"))],
    [("in", C("ts"), [T("2020-03-01"), T("2020"), T("2021-01-01")])],
    [("in", C("ts"), [T("2020-03-01"), L("timestamp", None)])],
    [("not", ("in", C("ts"), [T("2020-03-01"), T("2020-03-01 12:30:00.5")]))],
    [("in", C("ts"), [L("timestamp", _US - 4 + k) for k in range(9)])],            # the bitmap form
    [("in", C("ts"), [L("timestamp", _US + k * 10 ** 9) for k in range(-5, 5)])],  # a sorted set of 10
    [(">=", C("ts"), T("2020-03-01")), ("<", C("ts"), T("2020-03-02"))],
    [("and", (">=", C("ts"), T("2020-03-01")), ("=", C("part"), L("integer", 3)))],
    [("or", ("<", C("ts"), T("1970-01-01")), ("not", ("!=", C("part"), L("integer", 1))))],
    # decimal(12,2): the unscaled value
    [("=", C("m"), M2(1235))],
    [("!=", C("m"), M2(1235))],
    [("<", C("m"), M2(0))],
    [("<=", C("m"), M2(-1235))],
    [(">", C("m"), M2(1234))],
    [(">=", C("m"), M2(999999999999))],
    [("<=>", C("m"), M2(None))],
    [("in", C("m"), [M2(1234), M2(-1235), M2(None)])],
    [("in", C("m"), [M2(k) for k in range(-4, 6)])],
    [("and", ("not", ("<", C("m"), M2(-1))), ("in", C("part"), [L("integer", 0), L("integer", 2)]))],
    # decimal(38,10): 128 bits
    [("=", C("w"), W10(1 << 64))],
    [("!=", C("w"), W10(-(10 ** 10)))],
    [("<", C("w"), W10(1 << 64))],
    [(">", C("w"), W10((1 << 63) - 1))],
    [(">=", C("w"), W10(1 << 65))],
    [("<=", C("w"), W10(-(1 << 64)))],
    [(">", C("w"), W10(-(1 << 64)))],
    [("<=>", C("w"), W10(None))],
    [("in", C("w"), [W10(1 << 64), W10(1 << 65), W10(-(10 ** 10))])],
    [("in", C("w"), [W10(1 << 63), W10(None)])],
    [("in", C("w"), [W10((1 << 63) + k) for k in range(-1, 8)] + [W10(10 ** 38 - 1), W10(-(10 ** 38) + 1)])],
    [("or", ("<", C("w"), W10(0)), ("=", C("part"), L("integer", 4)))],
    # binary: unsigned bytes
    [("=", C("b"), BIN(b"prefix12A"))],
    [("!=", C("b"), BIN(b"prefix12A"))],
    [("<", C("b"), BIN(b"prefix12B"))],
    [("<=", C("b"), BIN(b"prefix12"))],
    [(">", C("b"), BIN(b"prefix12"))],
    [(">=", C("b"), BIN("é".encode("utf-8")))],
    [("<=>", C("b"), BIN(None))],
    [("in", C("b"), [BIN(b"prefix12B"), BIN("prefix12é".encode("utf-8")), BIN(b""), BIN(None)])],
    [("in", C("b"), [BIN(b"prefix12" + bytes([k])) for k in range(60, 70)])],
    [("and", ("isnotnull", C("b")), ("not", ("=", C("part"), L("integer", 0))))],
    # double: compareDoubles
    [("=", C("d"), DBL(1.5))],
    [("!=", C("d"), DBL(1.5))],
    [("<", C("d"), DBL(0.0))],
    [("<=", C("d"), DBL(0.0))],
    [("=", C("d"), DBL(-0.0))],
    [(">", C("d"), DBL(1e308))],
    [(">=", C("d"), DBL(NAN))],
    [("=", C("d"), DBL(NAN))],
    [("<", C("d"), DBL(NAN))],
    [(">", C("d"), DBL(INF))],
    [("=", C("d"), DBL(3.0))],
    [(">", C("d"), DBL(3.14)), ("<", C("d"), DBL(3.15))],
    [("=", C("d"), DBL(5e-324))],
    [("<", DBL(0.0), C("d")), ("<", C("d"), DBL(1e-300))],
    [("<=>", C("d"), DBL(None))],
    [("<=>", C("d"), DBL(NAN))],
    [("in", C("d"), [DBL(1.5), DBL(NAN), DBL(-0.0)])],
    [("in", C("d"), [DBL(2.5), DBL(None)])],
    [("in", C("d"), [DBL(float(k)) for k in range(-3, 8)])],
    [("not", (">", C("d"), DBL(0.0)))],
    [("or", ("=", C("d"), DBL(-INF)), ("and", (">=", C("d"), DBL(7.0)), ("=", C("part"), L("integer", 2))))],
    # float: compareFloats, and a double literal against the exactly widened value
    [("=", C("f"), FLT(1.5))],
    [("!=", C("f"), FLT(1.5))],
    [("<=", C("f"), FLT(-0.0))],
    [("<", C("f"), FLT(2.0 ** -126))],
    [("=", C("f"), FLT(NAN))],
    [(">", C("f"), FLT(3.0))],
    [(">=", C("f"), FLT(2.5))],
    [(">", C("f"), DBL(0.1))],
    [(">=", C("f"), DBL(0.1)), ("<", C("f"), DBL(0.2))],
    [("=", C("f"), DBL(16777216.0))],
    [("<", C("f"), DBL(16777216.5)), (">", C("f"), DBL(2.5))],
    [(">", C("f"), DBL(1e39))],
    [("<=>", C("f"), FLT(None))],
    [("in", C("f"), [FLT(1.5), DBL(0.1), FLT(2.5)])],
    [("in", C("f"), [FLT(float(k) / 2) for k in range(-2, 9)])],
    [("and", ("not", ("<", C("f"), FLT(1.0))), ("<", C("part"), L("integer", 3)))],
]


def compare_doubles(x, y):
    """SQLOrderingUtil.compareDoubles / compareFloats: equal when x == y (-0.0 and 0.0 are), else
    java.lang.Double.compare, where NaN equals NaN and is above everything else."""
    if x == y:
        return 0
    xn, yn = x != x, y != y
    if xn or yn:
        return 0 if (xn and yn) else (1 if xn else -1)
    return -1 if x < y else 1


def _cmp(a, b):
    if isinstance(a, float) and isinstance(b, float):
        return compare_doubles(a, b)
    return 0 if a == b else (-1 if a < b else 1)


def spark_eval(expr, pv, schema, cast=O.cast_string):
    """O.eval_predicate's tree walk with comparisons by compare_doubles (three-valued: None is NULL);
    `cast` is the column cast (the oracle's, or cast_timestamp_any_year for the years table)."""
    op = expr[0]
    if op == "col":
        field = next(f for f in schema if f.lower() == expr[1].strip("`").lower())
        return cast((pv or {}).get(field), schema[field])
    if op == "lit":
        return O.eval_predicate(expr, pv, schema)
    if op in ("=", "!=", "<", "<=", ">", ">="):
        a, b = spark_eval(expr[1], pv, schema, cast), spark_eval(expr[2], pv, schema, cast)
        if a is None or b is None:
            return None
        c = _cmp(a, b)
        return {"=": c == 0, "!=": c != 0, "<": c < 0, "<=": c <= 0, ">": c > 0, ">=": c >= 0}[op]
    if op == "<=>":
        a, b = spark_eval(expr[1], pv, schema, cast), spark_eval(expr[2], pv, schema, cast)
        return (a is None and b is None) or (a is not None and b is not None and _cmp(a, b) == 0)
    if op == "in":
        a = spark_eval(expr[1], pv, schema, cast)
        if a is None:
            return None
        vals = [spark_eval(l, pv, schema, cast) for l in expr[2]]
        if any(v is not None and _cmp(a, v) == 0 for v in vals):
            return True
        return None if any(v is None for v in vals) else False
    if op in ("isnull", "isnotnull"):
        return (spark_eval(expr[1], pv, schema, cast) is None) == (op == "isnull")
    if op == "not":
        a = spark_eval(expr[1], pv, schema, cast)
        return None if a is None else (not a)
    a, b = spark_eval(expr[1], pv, schema, cast), spark_eval(expr[2], pv, schema, cast)
    if op == "and":
        return False if (a is False or b is False) else (None if (a is None or b is None) else True)
    if op == "or":
        return True if (a is True or b is True) else (None if (a is None or b is None) else False)
    raise ValueError(op)


def _reads_fp(expr, schema):
    if expr[0] == "col":
        return schema.get(next((c for c in schema if c.lower() == expr[1].strip("`").lower()), None)) in ("float", "double")
    if expr[0] == "lit":
        return expr[1] in ("float", "double")
    if expr[0] == "in":
        return _reads_fp(expr[1], schema) or any(_reads_fp(l, schema) for l in expr[2])
    return any(_reads_fp(a, schema) for a in expr[1:])


def expected(schema, files, preds):
    """The files `preds` (ANDed) select: the oracle's filter_file_list. A predicate that reads a float
    or double column goes through spark_eval instead, because both columns of the table hold NaN
    rows, so every such predicate compares some NaN, where Python's comparisons are not Spark's
    (a float / double literal occurs only against those columns). Every other predicate is the
    oracle's alone."""
    if not any(_reads_fp(e, schema) for e in preds):
        return O.filter_file_list(schema, files, preds)
    return [f for f in files if all(spark_eval(e, f["partitionValues"], schema) is True for e in preds)]


# ---- timestamps beyond datetime's years -----------------------------------------------------------
YEARS_TYPES = {"ts": "timestamp", "part": "integer"}
YEARS_TS = ["-0044-03-15 10:00:00", "-0001-01-01 00:00:00", "0000-02-29 12:00:00", "-0001-02-29 00:00:00",
            "+12345-06-07 08:09:10.5", "10000-01-01 00:00:00Z", "-290000-01-01", "0001-01-01 00:00:00",
            "9999-12-31 23:59:59.999999", "1970-01-01 00:00:00", "2020-03-01 00:00:00", None, "-044-03-15"]
N_YEARS = 130


def _years_add(i):
    return {"path": "y-%04d.parquet" % i, "partitionValues": {"ts": YEARS_TS[i % len(YEARS_TS)], "part": str(i % 3)},
            "size": 10 + i, "modificationTime": 1600000000000 + i % 7, "dataChange": True, "stats": None}


def build_years(table_dir):
    """A table of N_YEARS files over YEARS_TS; returns its _delta_log path."""
    log = os.path.join(table_dir, "_delta_log")
    os.makedirs(log, exist_ok=True)
    schema = {"type": "struct", "fields": [{"name": c, "type": t, "nullable": True, "metadata": {}}
                                           for c, t in YEARS_TYPES.items()]}
    md = dict(METADATA, id="filter-years", schemaString=json.dumps(schema), partitionColumns=list(YEARS_TYPES))
    with open(os.path.join(log, "%020d.json" % 0), "w") as f:
        for a in [{"protocol": PROTOCOL}, {"metaData": md}] + [{"add": _years_add(i)} for i in range(N_YEARS)]:
            f.write(_line(a) + "\n")
    return log


def cast_timestamp_any_year(s, typ):
    """O.cast_string, and for a timestamp whose year lies outside 1..9999 (which the oracle reads as
    NULL, Spark as a proleptic Gregorian date) the oracle's value of the same text with the year
    moved by a multiple of 400 into 2000..2399, moved back by 146,097 days per 400 years."""
    import re
    v = O.cast_string(s, typ)
    if v is not None or s is None or typ != "timestamp":
        return v
    m = re.match(r"([\x00-\x20]*)([+-]?)(\d{4,6})(.*)\Z", s, re.S)
    if not m:
        return None
    y = int(m.group(3)) * (-1 if m.group(2) == "-" else 1)
    if 1 <= y <= 9999:
        return None
    y2 = y % 400 + 2000
    v = O.cast_string("%s%04d%s" % (m.group(1), y2, m.group(4)), typ)
    return None if v is None else v + (y - y2) // 400 * 146097 * 86400 * 10 ** 6


def TY(s):
    return L("timestamp", cast_timestamp_any_year(s, "timestamp"))


YEARS_PREDICATES = [
    [("<", C("ts"), TY("1970-01-01 00:00:00"))],
    [("<", C("ts"), TY("-0001-01-01 00:00:00"))],
    [("<=", C("ts"), TY("-0001-01-01 00:00:00"))],
    [("=", C("ts"), TY("-0044-03-15 10:00:00"))],
    [("!=", C("ts"), TY("0000-02-29 12:00:00"))],
    [(">", C("ts"), TY("9999-12-31 23:59:59.999999"))],
    [(">=", C("ts"), TY("+12345-06-07 08:09:10.5"))],
    [("<=>", C("ts"), L("timestamp", None))],
    [("isnotnull", C("ts"))],
    [("in", C("ts"), [TY("-290000-01-01"), TY("10000-01-01 00:00:00"), TY("2020-03-01")])],
    [("not", ("in", C("ts"), [TY("-0044-03-15 10:00:00"), TY("0001-01-01")]))],
    [("and", ("<", C("ts"), TY("0001-01-01 00:00:00")), ("=", C("part"), L("integer", 1)))],
    [("or", (">", C("ts"), TY("10000-01-01")), ("<", C("ts"), TY("-100000-01-01")))],
]


def expected_years(schema, files, preds):
    """The files of the years table that `preds` select, by spark_eval over cast_timestamp_any_year."""
    return [f for f in files if all(spark_eval(e, f["partitionValues"], schema, cast_timestamp_any_year) is True
                                    for e in preds)]
