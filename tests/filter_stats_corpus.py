"""Data-skipping corpus for K5's statistics columns (DR_SRC_STATS_* of include/deltareplay.h): one table
of 399 live files whose `add.stats` strings are steered -- absent, JSON null, `{}`, missing members,
nested struct columns, escaped keys and values, repeated keys at every level, the wrong token kind for
every type, -0, the int64 extremes and one past them, doubles with exponents and more than 19 digits,
NaN and the infinities, strings that share their first 8 bytes, malformed JSON, and one string of
70 000 bytes whose wanted members lie behind offset 65 535 -- between ordinary writer-shaped ones.

The expected values come from here: Python's json.loads with hooks that keep every number's text, the
conversions of delta_amd/predicates.py (the host restatements of the casts) and a walk of the predicate
tree with Spark's three-valued logic. Nothing here calls the device or reads stats_json.h."""
import datetime as dt
import json
import os
import re
import struct

from delta_amd import _native as N
from delta_amd import predicates as P
from delta_amd.testing import synth as S

MIN, MAX, NULLCOUNT, NUMRECORDS = N.DR_SRC_STATS_MIN, N.DR_SRC_STATS_MAX, N.DR_SRC_STATS_NULLCOUNT, N.DR_SRC_STATS_NUMRECORDS
GROUP = {MIN: "minValues", MAX: "maxValues", NULLCOUNT: "nullCount", NUMRECORDS: "numRecords"}
# the data columns (path -> type) and the one partition column
DTYPES = {("id",): "long", ("b",): "byte", ("sh",): "short", ("i",): "integer", ("f",): "float", ("d",): "double",
          ("dec",): "decimal(12,2)", ("dt",): "date", ("ts",): "timestamp", ("s",): "string", ("n", "x"): "integer",
          ("n", "y", "z"): "string", ('we"ird',): "string"}
_F = lambda name, t: {"name": name, "type": t, "nullable": True, "metadata": {}}  # noqa: E731
_ST = lambda fields: {"type": "struct", "fields": fields}  # noqa: E731
SCHEMA = _ST([_F(p[0], t) for p, t in DTYPES.items() if len(p) == 1] +
             [_F("n", _ST([_F("x", "integer"), _F("y", _ST([_F("z", "string")]))])), _F("p", "integer")])
METADATA = {"id": "filter-stats-corpus", "format": {"provider": "parquet", "options": {}},
            "schemaString": json.dumps(SCHEMA, separators=(",", ":")), "partitionColumns": ["p"],
            "configuration": {}, "createdTime": 1600000000000}
PROTOCOL = {"minReaderVersion": 1, "minWriterVersion": 2}
N_ADDS, N_CKPT, N_TAIL, REMOVED = 400, 200, 20, 3
N_LIVE = N_ADDS - 1

I64_MAX, I64_MIN = 2 ** 63 - 1, -2 ** 63
LONG_PAD = "x" * 70000

# ---- the steered statistics: raw strings (None: the add has no stats) ---------------------------------
STEERED = [
    None, "null", "{}", "", "   ", "[]", "5", '"{}"', "{", '{"numRecords":3', '{"numRecords":3}}', '{"numRecords":3} x',
    '{"numRecords":3,}', '{numRecords:3}', '{"numRecords":03}', '{"numRecords":3,"minValues":{"id":1.}}',
    '{"numRecords":3,"minValues":{"s":"a\\x"}}', '{"numRecords":3,"minValues":{"s":"tab\there"}}', '{"numRecords":tru}',
    # missing members
    '{"numRecords":10}', '{"numRecords":10,"maxValues":{"id":9},"nullCount":{"id":0}}', '{"minValues":{"id":4},"maxValues":{"id":9}}',
    '{"numRecords":10,"minValues":{},"maxValues":{},"nullCount":{}}', '{"numRecords":10,"minValues":null,"maxValues":7,"nullCount":[1]}',
    # whitespace wherever JSON allows it
    ' {\t"numRecords" :\n5 , "minValues" : { "id" : 2 , "s" : "b" } ,\r\n "maxValues":{ "id":8,"s":"y" } , "nullCount" : { "id" : 1 } } ',
    # nested columns, a non-object on the path
    '{"numRecords":4,"minValues":{"n":{"x":-3,"y":{"z":"k"}}},"maxValues":{"n":{"x":12,"y":{"z":"kz"}}},"nullCount":{"n":{"x":1,"y":{"z":4}}}}',
    '{"numRecords":4,"minValues":{"n":5},"maxValues":{"n":{"x":{"deep":1},"y":"flat"}},"nullCount":{"n":[{"x":1}]}}',
    '{"numRecords":4,"minValues":{"n.x":1,"n":{"y":{"z":"only"}}},"maxValues":{"n":{"y":{"z":null}}}}',
    # escaped keys, and values with \\" \\\\ and \\u00e9
    '{"numRecords":2,"minValues":{"we\\"ird":"a\\"b","s":"back\\\\slash"},"maxValues":{"we\\u0022ird":"caf\\u00e9","s":"caf\\u00e9"}}',
    '{"numRecords":2,"minValues":{"\\u0069d":5,"\\u0073":"\\u0061bc"},"maxValues":{"i\\u0064":6,"s":"\\ud83d\\ude00 pair"}}',
    '{"numRecords":2,"minValues":{"s":"}{\\"}{"},"skip":"}{","also":{"a":"\\"}","b":[1,{"c":"]"}]},"maxValues":{"s":"~"}}',
    # repeated keys at every level: the last one holds
    '{"numRecords":1,"numRecords":7,"minValues":{"id":1,"id":2},"maxValues":{"id":3},"maxValues":{"id":4,"id":5}}',
    '{"numRecords":7,"minValues":{"id":1},"minValues":{"s":"later"},"maxValues":{"id":9},"maxValues":5}',
    '{"numRecords":7,"minValues":{"n":{"x":1},"n":{"y":{"z":"q"}}},"maxValues":{"n":{"x":1,"x":2}},"nullCount":{"id":0,"id":null}}',
    # the wrong token kind for every type
    '{"numRecords":"3","minValues":{"id":"1","b":1.0,"sh":1e2,"i":true,"f":"1.5","d":"x","dec":"1.00","dt":20200101,"ts":0,"s":5},'
    '"maxValues":{"id":[1],"b":{},"sh":null,"i":"7","f":false,"d":{"v":1},"dec":null,"dt":null,"ts":"never","s":null},"nullCount":{"id":"0","s":1.5}}',
    # out of range for the narrow kinds; -0; the int64 extremes and one past them
    '{"numRecords":0,"minValues":{"b":-129,"sh":-32769,"i":-2147483649,"id":-9223372036854775809},'
    '"maxValues":{"b":128,"sh":32768,"i":2147483648,"id":9223372036854775808}}',
    '{"numRecords":-0,"minValues":{"b":-128,"sh":-32768,"i":-2147483648,"id":-9223372036854775808,"d":-0,"f":-0.0},'
    '"maxValues":{"b":127,"sh":32767,"i":2147483647,"id":9223372036854775807,"d":-0.0,"f":0},"nullCount":{"id":-0}}',
    # doubles: exponents, more than 19 digits (left to the host), NaN and the infinities as strings
    '{"numRecords":5,"minValues":{"d":4.9e-324,"f":1.17549435e-38},"maxValues":{"d":1.7976931348623157e308,"f":3.4028235e38}}',
    '{"numRecords":5,"minValues":{"d":0.1234567890123456789012345,"f":0.1234567890123456789012345},'
    '"maxValues":{"d":123456789012345678901234567890,"f":16777217}}',
    '{"numRecords":5,"minValues":{"d":1e23,"f":1e10},"maxValues":{"d":2.2250738585072011e-308,"f":1E-2}}',
    '{"numRecords":5,"minValues":{"d":"-Infinity","f":"-Infinity"},"maxValues":{"d":"NaN","f":"Infinity"}}',
    '{"numRecords":5,"minValues":{"d":"nan","f":"+Infinity"},"maxValues":{"d":"Infinity ","f":"inf"}}',
    '{"numRecords":5,"minValues":{"d":1e400,"f":1e39,"dec":1e3},"maxValues":{"d":-1e400,"f":-1e-60,"dec":12345678901.005}}',
    '{"numRecords":5,"minValues":{"dec":-0.005,"id":12},"maxValues":{"dec":9999999999.994,"id":12}}',
    # dates and timestamps: the writer's form, an escaped one, the lenient forms, nonsense
    '{"numRecords":6,"minValues":{"dt":"1969-12-31","ts":"1969-12-31T23:59:59.999Z"},"maxValues":{"dt":"2024-02-29","ts":"2024-02-29T12:00:00.123+01:00"}}',
    '{"numRecords":6,"minValues":{"dt":"2020\\u002d01-01","ts":"2020-01-01T00:00:00.000\\u005a"},"maxValues":{"dt":"2020-1-1","ts":"2020-01-01 00:00:00"}}',
    '{"numRecords":6,"minValues":{"dt":"2023-02-29","ts":"2023-02-29T00:00:00.000Z"},"maxValues":{"dt":"","ts":""}}',
    # strings that share their first 8 bytes
    '{"numRecords":9,"minValues":{"s":"prefix00-a"},"maxValues":{"s":"prefix00-b"},"nullCount":{"s":0}}',
    '{"numRecords":9,"minValues":{"s":"prefix00-b"},"maxValues":{"s":"prefix00-c"},"nullCount":{"s":9}}',
    '{"numRecords":9,"minValues":{"s":"prefix00"},"maxValues":{"s":"prefix00-"},"nullCount":{"s":3}}',
    '{"numRecords":9,"minValues":{"s":""},"maxValues":{"s":"prefix00-a\\u0000"},"nullCount":{"s":null}}',
    # the wanted members behind offset 65 535
    '{"numRecords":70,"pad":"%s","minValues":{"id":65536,"s":"far"},"maxValues":{"id":70000,"s":"farther"},"nullCount":{"id":2}}' % LONG_PAD,
]


def _regular(i):
    """What a writer leaves for file i: every column, millisecond timestamps."""
    lo, n = 1000 * (i % 37) - 5000, 50 + i % 7
    ms = 1600000000000 + 86400000 * (i % 29)
    ts = lambda m: "2020-09-%02dT%02d:26:40.%03dZ" % (13 + (m // 86400000) % 15, 12 + m % 3, m % 1000)  # noqa: E731
    mn = {"id": lo, "b": i % 100 - 50, "sh": lo // 4, "i": lo * 3, "f": (i % 16) / 4.0, "d": lo / 8.0, "dec": lo / 100.0,
          "dt": "2021-%02d-%02d" % (1 + i % 12, 1 + i % 28), "ts": ts(ms), "s": "name-%04d" % (i % 50),
          "n": {"x": i % 9, "y": {"z": "z%02d" % (i % 20)}}, 'we"ird': "w%d" % (i % 4)}
    mx = {"id": lo + 999, "b": i % 100 - 40, "sh": lo // 4 + 9, "i": lo * 3 + 99, "f": (i % 16) / 4.0 + 1.5, "d": lo / 8.0 + 0.125,
          "dec": lo / 100.0 + 7.25, "dt": "2021-%02d-%02d" % (1 + i % 12, 1 + i % 28 + (i % 3 == 0)), "ts": ts(ms + 999 * (i % 2)),
          "s": "name-%04d~" % (i % 50 + i % 3), "n": {"x": i % 9 + 2, "y": {"z": "z%02d" % (i % 20 + 1)}}, 'we"ird': "w%d" % (i % 4 + 1)}
    nc = {"id": 0, "b": i % 2, "sh": 0, "i": 0, "f": 0, "d": 0, "dec": 0, "dt": n if i % 11 == 0 else 0, "ts": 0, "s": i % 5,
          "n": {"x": 0, "y": {"z": n if i % 13 == 0 else 1}}, 'we"ird': 0}
    return json.dumps({"numRecords": n, "minValues": mn, "maxValues": mx, "nullCount": nc}, separators=(",", ":"))


ALL_STATS = STEERED + [_regular(i) for i in range(113 - len(STEERED))]
assert len(ALL_STATS) == 113 and len(STEERED) < 80  # 113 is coprime to the halves: every string on both sides


def _add(i):
    return {"path": "f-%05d.parquet" % i, "partitionValues": {"p": str(i % 5)}, "size": 100 + i, "modificationTime": 1600000000000 + i,
            "dataChange": True, "stats": ALL_STATS[i % len(ALL_STATS)]}


def live_files():
    return [_add(i) for i in range(N_ADDS) if i != REMOVED]


def build(table_dir, checkpoint):
    """The _delta_log path. v0: protocol, metadata, the first 200 adds (with `checkpoint`, also a checkpoint
    of v0 written by pyarrow: their stats are then read from its add.stats column); v1: 180 adds; v2: the
    last 20 and one remove -- the commit a test applies with dr_state_apply on top of the v1 state."""
    log = os.path.join(table_dir, "_delta_log")
    os.makedirs(log, exist_ok=True)
    line = lambda a: json.dumps(a, separators=(",", ":"))  # noqa: E731
    cuts = [(0, N_CKPT), (N_CKPT, N_ADDS - N_TAIL), (N_ADDS - N_TAIL, N_ADDS)]
    for v, (lo, hi) in enumerate(cuts):
        with open(os.path.join(log, "%020d.json" % v), "w", encoding="utf-8") as f:
            if v == 0:
                f.write(line({"protocol": PROTOCOL}) + "\n" + line({"metaData": METADATA}) + "\n")
            if v == 2:
                f.write(line({"remove": {"path": "f-%05d.parquet" % REMOVED, "deletionTimestamp": 1600000001000, "dataChange": True}}) + "\n")
            for i in range(lo, hi):
                f.write(line({"add": _add(i)}) + "\n")
    if checkpoint:
        adds = [_add(i) for i in range(N_CKPT)]
        S.write_checkpoint_records(os.path.join(log, "%020d.checkpoint.parquet" % 0), PROTOCOL, METADATA, adds, row_group_size=70)
        with open(os.path.join(log, "_last_checkpoint"), "w") as f:
            f.write('{"version":0,"size":%d}\n' % (len(adds) + 2))
    return log


# ---- the expected values ------------------------------------------------------------------------------
class Num(str):
    """A JSON number, kept as its text."""


def _refuse(name):
    raise ValueError(name)


def parse_stats(s):
    """The statistics object, or None when there is none: no stats, no well-formed JSON, no object."""
    if s is None:
        return None
    try:
        v = json.loads(s, parse_int=Num, parse_float=Num, parse_constant=_refuse)
    except ValueError:
        return None
    return v if isinstance(v, dict) else None


def token(stats, source, path):
    """The JSON value at (source, path); `KeyError` stands for absent."""
    v = parse_stats(stats)
    for key in (GROUP[source],) + tuple(path):
        if not isinstance(v, dict) or key not in v:
            raise KeyError(key)
        v = v[key]
    return v


def _signed64(u):
    return u - (1 << 64) if u >= 1 << 63 else u


def _bits(x, typ):
    return struct.unpack("<I", struct.pack("<f", x))[0] if typ == "float" else _signed64(P.double_bits(x))


def typed(stats, source, path, typ):
    """(value as dr_state_stats_column reports it, value as the evaluator compares it), or None for NULL.
    Integer kinds, date days and timestamp micros are both; float / double: (bits, order key); decimal:
    (None, unscaled); string: (None, UTF-8 bytes)."""
    try:
        v = token(stats, source, path)
    except KeyError:
        return None
    if typ in P._INT_BITS:
        if not isinstance(v, Num) or not re.fullmatch(r"-?[0-9]+", v):
            return None
        x, b = int(v), P._INT_BITS[typ]
        return (x, x) if -(1 << (b - 1)) <= x < (1 << (b - 1)) else None
    if typ in ("float", "double"):
        if not (isinstance(v, Num) or (isinstance(v, str) and v in ("NaN", "Infinity", "-Infinity"))):
            return None
        x = P.java_parse_fp(str(v), typ == "float")
        bits = _bits(x, typ)
        return bits, P.fp_order_key(bits % (1 << 64) if typ == "double" else bits, 32 if typ == "float" else 64)
    if typ.startswith("decimal"):
        p, s = (int(g) for g in re.fullmatch(r"decimal\((\d+),(\d+)\)", typ).groups())
        d = P.decimal_value(str(v), p, s) if isinstance(v, Num) else None
        return None if d is None else (None, int(d.scaleb(s)))
    if isinstance(v, Num) or not isinstance(v, str):
        return None
    if typ == "date":
        x = P._date_days(v)
    elif typ == "timestamp":
        x = P.timestamp_micros(v)
    else:
        return None, v.encode("utf-8", "surrogatepass")
    return None if x is None else (x, x)


def _literal(typ, v):
    if v is None:
        return None
    if typ in ("float", "double"):
        return P.fp_order_key(P._lit(typ, v), 32 if typ == "float" else 64)
    if typ.startswith("decimal"):
        return int.from_bytes(P._lit(typ, v), "little", signed=True)
    return P._lit(typ, v)  # ints, days, micros, UTF-8 bytes


def evaluate(expr, add):
    """Three-valued evaluation of a predicate tree over one AddFile (None is NULL)."""
    op = expr[0]
    if op == "stats":
        t = typed(add["stats"], expr[1], expr[2], expr[3])
        return None if t is None else t[1]
    if op == "col":  # the partition column
        return int(add["partitionValues"]["p"])
    if op == "lit":
        return _literal(expr[1], expr[2])
    if op in ("=", "!=", "<", "<=", ">", ">="):
        a, b = evaluate(expr[1], add), evaluate(expr[2], add)
        if a is None or b is None:
            return None
        return {"=": a == b, "!=": a != b, "<": a < b, "<=": a <= b, ">": a > b, ">=": a >= b}[op]
    if op in ("isnull", "isnotnull"):
        return (evaluate(expr[1], add) is None) == (op == "isnull")
    if op in ("startswith", "like", "year", "to_date"):
        a = evaluate(expr[1], add)
        if a is None:
            return None
        if op == "year":
            return (dt.date(1970, 1, 1) + dt.timedelta(days=a)).year
        if op == "to_date":
            return a // 86_400_000_000
        pat = evaluate(expr[2], add)
        if op == "startswith":
            return a.startswith(pat)
        rx = "".join(".*" if ch == "%" else "." if ch == "_" else re.escape(ch) for ch in pat.decode("utf-8"))
        return re.fullmatch(rx, a.decode("utf-8", "surrogatepass"), re.S) is not None
    if op == "in":
        a, vals = evaluate(expr[1], add), [evaluate(x, add) for x in expr[2]]
        if a is None:
            return None
        return True if a in [v for v in vals if v is not None] else (None if None in vals else False)
    if op == "not":
        a = evaluate(expr[1], add)
        return None if a is None else (not a)
    a, b = evaluate(expr[1], add), evaluate(expr[2], add)
    if op == "and":
        return False if (a is False or b is False) else (None if (a is None or b is None) else True)
    if op == "or":
        return True if (a is True or b is True) else (None if (a is None or b is None) else False)
    raise ValueError(op)


def expected(files, preds):
    return [f for f in files if all(evaluate(e, f) is True for e in preds)]


# ---- the predicates -----------------------------------------------------------------------------------
C = lambda n: ("col", n)  # noqa: E731
L = lambda t, v: ("lit", t, v)  # noqa: E731
ST = lambda src, path, typ: ("stats", src, tuple(path), typ)  # noqa: E731
TYPE_OF = {".".join(p): t for p, t in DTYPES.items()}

# data filters, rewritten by delta_amd/skipping.py: every row of its table, over every type
DATA_FILTERS = [
    ("=", C("id"), L("long", 12)), ("<", C("id"), L("long", -4000)), ("<=", C("id"), L("long", I64_MIN)),
    (">", C("id"), L("long", 30000)), (">=", C("id"), L("long", I64_MAX)), ("!=", C("id"), L("long", 12)),
    ("in", C("id"), [L("long", 2), L("long", 65536), L("long", 7), L("long", -5000)]),
    ("isnull", C("id")), ("isnotnull", C("id")), ("isnull", C("dt")), ("isnotnull", C("n.y.z")), ("isnotnull", C("s")),
    ("=", C("b"), L("byte", -128)), (">", C("b"), L("byte", 40)), ("<", C("sh"), L("short", -32000)), (">=", C("i"), L("integer", 2147483647)),
    ("=", C("f"), L("float", 0.0)), (">", C("f"), L("float", 3.0)), ("<", C("f"), L("float", float("-inf"))),
    ("=", C("d"), L("double", float("nan"))), (">=", C("d"), L("double", 1e300)), ("<", C("d"), L("double", -600.0)),
    ("<=", C("d"), L("double", 0.0)), ("!=", C("d"), L("double", 0.0)),
    ("=", C("dec"), L("decimal(12,2)", 0)), (">", C("dec"), L("decimal(12,2)", 999999999998)), ("<", C("dec"), L("decimal(12,2)", -4500)),
    ("=", C("dt"), L("date", "2020-01-01")), ("<", C("dt"), L("date", "1970-01-01")), (">=", C("dt"), L("date", "2021-12-01")),
    ("=", C("ts"), L("timestamp", "2020-09-14 12:26:40.5")), (">", C("ts"), L("timestamp", "2020-09-27 14:26:40.998")),
    ("<=", C("ts"), L("timestamp", "1969-12-31 23:59:59.999")), (">=", C("ts"), L("timestamp", I64_MIN + 5)),
    ("=", C("s"), L("string", "prefix00-b")), ("<", C("s"), L("string", "prefix00-a")), (">", C("s"), L("string", "prefix00-b")),
    (">=", C("s"), L("string", "café")), ("=", C("s"), L("string", '}{"}{')), ("<=", C("s"), L("string", "")),
    ("in", C("s"), [L("string", "name-0003"), L("string", "far"), L("string", "\U0001F600 pair")]),
    ("=", C("n.x"), L("integer", 2)), (">", C("n.y.z"), L("string", "z15")), ("=", C('we"ird'), L("string", 'a"b')),
    ("not", ("<", C("id"), L("long", 25000))), ("not", ("or", ("=", C("id"), L("long", 12)), (">", C("f"), L("float", 1.0)))),
    ("not", ("and", ("isnull", C("s")), ("not", ("=", C("i"), L("integer", 0))))),
    ("and", (">=", C("id"), L("long", 1000)), ("<", C("id"), L("long", 2000))),
    ("and", ("like", C("s"), L("string", "a%")), (">", C("id"), L("long", 20000))),   # the LIKE side is dropped
    ("or", ("=", C("id"), L("long", 65536)), ("=", C("s"), L("string", "later"))),
]
# these rewrite to TRUE: a partition column under OR, LIKE alone, a NULL literal, <=>
TRUE_FILTERS = [
    ("or", ("=", C("p"), L("integer", 1)), (">", C("d"), L("double", 3500.0))),
    ("like", C("s"), L("string", "a%")), ("=", C("id"), L("long", None)), ("<=>", C("id"), L("long", 1)),
]
# written over the statistics columns directly, partition columns mixed in
ID_MIN, ID_MAX, NREC = ST(MIN, ["id"], "long"), ST(MAX, ["id"], "long"), ST(NUMRECORDS, [], "long")
DIRECT = [
    [("=", NREC, L("long", 7))], [("isnull", NREC)], [(">", NREC, L("long", 0)), ("=", C("p"), L("integer", 2))],
    [("<", ST(NULLCOUNT, ["s"], "long"), NREC)], [("=", ST(NULLCOUNT, ["n", "y", "z"], "long"), NREC)],
    [("<=", ID_MIN, ID_MAX)], [("=", ID_MIN, ID_MAX), ("in", C("p"), [L("integer", 0), L("integer", 2), L("integer", 4)])],
    [("in", ID_MIN, [L("long", I64_MIN), L("long", 2), L("long", 65536), L("long", None)])],
    [("not", ("in", ST(MAX, ["s"], "string"), [L("string", "prefix00-b"), L("string", "y")]))],
    [("isnotnull", ST(MIN, ["d"], "double")), ("isnull", ST(MAX, ["f"], "float"))],
    [("startswith", ST(MIN, ["s"], "string"), L("string", "prefix00-"))], [("like", ST(MAX, ["s"], "string"), L("string", "%f_"))],
    [("=", ("year", ST(MIN, ["dt"], "date")), L("integer", 2020))],
    [("<", ("to_date", ST(MIN, ["ts"], "timestamp")), L("date", "1970-01-01"))],
    [("or", ("=", C("p"), L("integer", 3)), ("=", ST(MIN, ["b"], "byte"), L("byte", -128)))],
    [("=", ST(MAX, ["dec"], "decimal(12,2)"), L("decimal(12,2)", 999999999999))],
]


def predicates():
    """Every predicate as a list of conjuncts over statistics and partition columns."""
    from delta_amd import skipping as K
    schema = K.data_schema(METADATA)
    out = []
    for f in DATA_FILTERS:
        r = K.rewrite(f, schema, ["p"])
        assert r is not None, f
        out.append([r])
    for f in TRUE_FILTERS:
        assert K.rewrite(f, schema, ["p"]) is None, f
    # a partition conjunct beside a rewritten one
    out.append([("=", C("p"), L("integer", 1)), K.rewrite(DATA_FILTERS[0], schema, ["p"])])
    return out + DIRECT
