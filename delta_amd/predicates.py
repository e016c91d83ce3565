"""Partition-pruning predicates: the host side of K5 (`dr_filter`).

Mirrors the reference's metadata-predicate handling:
  split_metadata_and_data_predicates <- DeltaTableUtils.splitMetadataAndDataPredicates /
                                        isPredicatePartitionColumnsOnly (D/DeltaTable.scala:198-294)
  build_program                      <- DeltaLog.rewritePartitionFilters + filterFileList
                                        (D/DeltaLog.scala:500-547): every partition column becomes
                                        Cast(partitionValues[col] AS partitionSchema(col).type), the
                                        filters are ANDed
  partition_schema                   <- Metadata.partitionSchema (D/actions/actions.scala:370-373)

Expressions are nested tuples (the oracle's format): ("col", name), ("lit", type, value),
(op, a, b) for = != < <= > >= <=>, ("in", a, [lits]), ("isnull", a), ("isnotnull", a),
("and", a, b), ("or", a, b), ("not", a), and the string patterns ("startswith", col, lit),
("endswith", col, lit), ("contains", col, lit), ("like", col, lit[, escape]) -- Catalyst's StartsWith /
EndsWith / Contains / Like over a string partition column and a string (or NULL) literal; the escape
is one character, Spark's default "\\". The date functions: ("year", e), ("quarter", e), ("month", e),
("dayofmonth", e), ("dayofweek", e), ("dayofyear", e), ("weekofyear", e) over a date, ("to_date", e)
over a timestamp (Cast(ts AS date), session zone UTC), ("date_add", e, n) / ("date_sub", e, n) with n
an int in the int32 range (no expression) and ("trunc", e, fmt) with fmt one of YEAR | YYYY | YY,
QUARTER, MONTH | MM | MON, WEEK in any case -- Catalyst's Year .. WeekOfYear, DateAdd / DateSub and
TruncDate; e is a partition column of the operand's type or another of these functions, so they nest,
and the result compares with integer literals (year .. weekofyear) or date literals. Types: "string", "byte", "short", "integer", "long",
"date", "boolean", "float", "double", "timestamp", "binary", "decimal(p,s)" ("decimal" is
decimal(10,0)). The program is evaluated on the GPU; nothing here evaluates it.

Literal values of the later types: "double" a float; "float" a float that binary32 holds exactly;
"timestamp" microseconds since the epoch as an int (a datetime, or a string in the partition
values' own grammar, is converted); "decimal(p,s)" the unscaled int at scale s (a decimal.Decimal
that quantises to s exactly is converted); "binary" bytes. A column takes literals of its own type,
and a float column also a double literal (Catalyst's `floatcol > 1.5`); anything else among these
types is a PredicateError -- widening, between decimal types too, is the caller's.
"""
from __future__ import annotations

import ctypes as C
import datetime as _dt
import json
import re
import struct
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

from . import _native as N

TYPE_CODE = {"string": 0, "byte": 1, "short": 2, "integer": 3, "long": 4, "date": 5, "boolean": 6,
             "float": 7, "double": 8, "timestamp": 9, "binary": 10, "decimal": 11 | 10 << 8}
T_FLOAT, T_DOUBLE, T_TIMESTAMP, T_BINARY, T_DECIMAL = 7, 8, 9, 10, 11
_DECIMAL_RE = re.compile(r"decimal\((\d+),(\d+)\)")


def type_code(typ: str) -> Optional[int]:
    """dr_pred_type of a Spark type name (a decimal's code carries p << 8 | s << 16); None when the
    predicate program has no such type."""
    if typ in TYPE_CODE:
        return TYPE_CODE[typ]
    m = _DECIMAL_RE.fullmatch(typ) if isinstance(typ, str) else None
    if m and 1 <= int(m.group(1)) <= 38 and int(m.group(2)) <= int(m.group(1)):
        return T_DECIMAL | int(m.group(1)) << 8 | int(m.group(2)) << 16
    return None
OP_COL, OP_LIT = 0, 1
OP_CODE = {"=": 2, "!=": 3, "<": 4, "<=": 5, ">": 6, ">=": 7, "<=>": 8, "in": 9, "isnull": 10,
           "isnotnull": 11, "and": 12, "or": 13, "not": 14,
           "startswith": 15, "endswith": 16, "contains": 17, "like": 18}
PATTERN_OPS = ("startswith", "endswith", "contains", "like")
# the date functions: DR_OP_YEAR .. DR_OP_TRUNC_DATE ("date_sub" is DATE_ADD of -n)
DATE_FN_CODE = {"year": 19, "quarter": 20, "month": 21, "dayofmonth": 22, "dayofweek": 23, "dayofyear": 24,
                "weekofyear": 25, "to_date": 26, "date_add": 27, "date_sub": 27, "trunc": 28}
DATE_FN_ARG_OPS = ("date_add", "date_sub", "trunc")  # a third element that is no expression
TRUNC_UNIT = {"year": 0, "yyyy": 0, "yy": 0, "quarter": 1, "month": 2, "mm": 2, "mon": 2, "week": 3}
_INT_TYPES = ("byte", "short", "integer", "long")
_EPOCH = _dt.date(1970, 1, 1)


class PredicateError(ValueError):
    pass


def partition_schema(metadata: Optional[dict]) -> Dict[str, str]:
    """Metadata.partitionSchema: partition column -> Spark type name (ordered as partitionColumns)."""
    if not metadata:
        return {}
    schema = json.loads(metadata["schemaString"])
    fields = {f["name"]: f["type"] for f in schema["fields"]}
    return {c: fields[c] for c in metadata.get("partitionColumns") or []}


def _refs(expr) -> List[str]:
    op = expr[0]
    if op == "col":
        return [expr[1]]
    if op == "lit" or op == "stats":  # a statistics column (skipping.py) names no table column
        return []
    if op == "in":
        return _refs(expr[1]) + [r for l in expr[2] for r in _refs(l)]
    if op == "like":  # a fourth element is the escape character, no expression
        return _refs(expr[1]) + _refs(expr[2])
    if op in DATE_FN_ARG_OPS:  # the day count / the format is no expression either
        return _refs(expr[1])
    return [r for a in expr[1:] for r in _refs(a)]


def _conjuncts(expr) -> List:
    if expr[0] == "and":
        return _conjuncts(expr[1]) + _conjuncts(expr[2])
    return [expr]


def _resolve(name: str, partition_cols: Sequence[str]) -> Optional[str]:
    # rewritePartitionFilters (D/DeltaLog.scala:531-533): backticks stripped, then the session
    # resolver (spark.sql.caseSensitive=false: case-insensitive) finds the partition field
    name = name.strip("`")
    for c in partition_cols:
        if c.lower() == name.lower():
            return c
    return None


def is_partition_only(expr, partition_cols: Sequence[str]) -> bool:
    """DeltaTableUtils.isPredicatePartitionColumnsOnly: every column the expression references is
    a partition column (resolved case-insensitively, as the session resolver does)."""
    return all(_resolve(r, partition_cols) is not None for r in _refs(expr))


def split_metadata_and_data_predicates(expr, partition_cols: Sequence[str]) -> Tuple[List, List]:
    """(metadata-only conjuncts, the rest): a conjunct is metadata-only when every column it
    references is a partition column (D/DeltaTable.scala:198-230)."""
    meta, data = [], []
    for c in _conjuncts(expr):
        refs = _refs(c)
        if all(_resolve(r, partition_cols) is not None for r in refs):
            meta.append(c)
        else:
            data.append(c)
    return meta, data


@dataclass
class Program:
    ops: List[Tuple[int, int]] = field(default_factory=list)
    cols: List[Tuple[str, int]] = field(default_factory=list)      # (exact map key, type code)
    lits: List[Tuple[int, object]] = field(default_factory=list)   # (type code, value | None)


_DATE_RE = re.compile(r"(\d{4})(?:-(\d{1,2})(?:-(\d{1,2})(?:[ T].*)?)?)?")


def _date_days(s: str) -> Optional[int]:
    """Cast(string AS date) of a literal, the same grammar the device applies to partition values."""
    m = _DATE_RE.fullmatch(s.strip(" \t\n\r\x0b\x0c"))
    if not m:
        return None
    try:
        return (_dt.date(int(m.group(1)), int(m.group(2) or 1), int(m.group(3) or 1)) - _EPOCH).days
    except ValueError:
        return None


_INT_BITS = {"byte": 8, "short": 16, "integer": 32, "long": 64}
_WS = " \t\n\r\x0b\x0c"


def cast_partition_value(s: Optional[str], typ: str):
    """Cast(Literal(partitionValues(col)), partition type) on the host, non-ANSI (a failed cast is
    null), as TahoeFileIndex.listFiles builds a partition row (D/files/TahoeFileIndex.scala:61-64):
    integral types from trimmed decimal text in range, booleans from t/true/y/yes/1 and
    f/false/n/no/0, dates as datetime.date, strings unchanged. Same grammar as the device cast.
    Timestamps are UTC datetimes; one whose year datetime cannot hold (outside 1..9999, which Spark
    and the device accept) is its microseconds since the epoch as an int, never None: a file that
    dr_filter selects by such a value keeps a non-NULL group row in Snapshot.list_files."""
    if s is None:
        return None
    if typ == "string":
        return s
    t = s.strip(_WS)
    if typ in _INT_BITS:
        if not re.fullmatch(r"[+-]?\d+", t):
            return None
        v, b = int(t), _INT_BITS[typ]
        return v if -(1 << (b - 1)) <= v < (1 << (b - 1)) else None
    if typ == "boolean":
        tl = t.lower()
        return True if tl in ("t", "true", "y", "yes", "1") else False if tl in ("f", "false", "n", "no", "0") else None
    if typ == "date":
        d = _date_days(t)
        return None if d is None else _EPOCH + _dt.timedelta(days=d)
    if typ in ("float", "double"):
        return java_parse_fp(s, typ == "float")
    if typ == "binary":
        return s.encode("utf-8")
    if typ == "timestamp":
        us = timestamp_micros(s)
        if us is None:
            return None
        try:
            return _dt.datetime(1970, 1, 1, tzinfo=_dt.timezone.utc) + _dt.timedelta(microseconds=us)
        except OverflowError:  # a year outside datetime's 1..9999: the microseconds themselves
            return us
    dm = re.fullmatch(r"decimal(?:\((\d+),(\d+)\))?", typ)
    if dm:
        p, sc = (int(dm.group(1)), int(dm.group(2))) if dm.group(1) else (10, 0)
        return decimal_value(s, p, sc)
    raise PredicateError("unsupported partition type %r" % typ)


# ---- the checkpoint's other partitionValues_parsed casts (the device grammar, k_filter.hip) ------
_FP_RE = re.compile(r"[+-]?(?:NaN|Infinity|(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?[fFdD]?)")
_HEXFP_RE = re.compile(r"([+-]?)0[xX]([0-9a-fA-F]+\.?[0-9a-fA-F]*|\.[0-9a-fA-F]+)[pP]([+-]?\d+)[fFdD]?")


def _jtrim(s: str) -> str:
    b, e = 0, len(s)
    while b < e and ord(s[b]) <= 32:
        b += 1
    while e > b and ord(s[e - 1]) <= 32:
        e -= 1
    return s[b:e]


def _round_f32(x):
    """Nearest binary32 to the exact rational x (round half to even), as Float.parseFloat."""
    import struct
    from fractions import Fraction
    if x == 0:
        return 0.0
    if abs(x) >= (Fraction(2) - Fraction(1, 1 << 24)) * Fraction(2) ** 127:  # rounds past FLT_MAX
        return float("inf") if x > 0 else float("-inf")
    fmax = float((Fraction(2) - Fraction(1, 1 << 23)) * Fraction(2) ** 127)
    f = struct.unpack("<f", struct.pack("<f", min(max(float(x), -fmax), fmax)))[0]
    bits = struct.unpack("<I", struct.pack("<f", f))[0]
    best = None
    for b in (bits - 1, bits, bits + 1):
        if b < 0 or b >= 1 << 32:
            continue
        c = struct.unpack("<f", struct.pack("<I", b))[0]
        if c != c or c in (float("inf"), float("-inf")):
            continue
        d = abs(Fraction(c) - x)
        if best is None or d < best[0] or (d == best[0] and b % 2 == 0):
            best = (d, c)
    return best[1]


def java_parse_fp(s: str, is_float: bool):
    """Double.parseDouble / Float.parseFloat, else Spark's special literals (inf, nan, ...)."""
    from fractions import Fraction
    t = _jtrim(s)
    hm = _HEXFP_RE.fullmatch(t)
    if hm:  # Java's hexadecimal significand with a binary exponent
        ip, _, fp = hm.group(2).partition(".")
        x = Fraction(int((ip or "0") + fp, 16), 16 ** len(fp)) * Fraction(2) ** int(hm.group(3))
        v = _round_f32(x) if is_float else (float(x) if x < Fraction(2) ** 1025 else float("inf"))
        return -v if hm.group(1) == "-" else v
    if _FP_RE.fullmatch(t):
        body = t.rstrip("fFdD") if not t.endswith(("NaN", "Infinity")) else t
        if body.lstrip("+-") == "NaN":
            return float("nan")
        if body.lstrip("+-") == "Infinity":
            return float("-inf") if body.startswith("-") else float("inf")
        if is_float:
            v = _round_f32(Fraction(body))
            return -0.0 if v == 0 and body.startswith("-") else v
        return float(body)
    tl = t.lower()
    if tl in ("inf", "+inf", "infinity", "+infinity"):
        return float("inf")
    if tl in ("-inf", "-infinity"):
        return float("-inf")
    if tl == "nan":
        return float("nan")
    return None


def decimal_value(s: str, precision: int, scale: int):
    """Decimal.fromString + changePrecision: BigDecimal of the trimmed text, HALF_UP to `scale`,
    null beyond `precision` digits."""
    import decimal
    t = _jtrim(s)
    if not re.fullmatch(r"[+-]?(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?", t):
        return None
    ctx = decimal.Context(prec=100000, rounding=decimal.ROUND_HALF_UP)
    try:
        v = decimal.Decimal(t).quantize(decimal.Decimal(1).scaleb(-scale), context=ctx)
    except decimal.InvalidOperation:
        return None
    unscaled = abs(int(v.scaleb(scale, context=ctx)))
    return None if unscaled >= 10 ** precision else (v if v != 0 else abs(v))


_TS_RE = re.compile(r"([+-]?)(\d{4,6})(?:-(\d{1,2})(?:-(\d{1,2})(?:[ T](\d{1,2}):(\d{1,2})"
                    r"(?::(\d{1,2})(?:\.(\d*))?)?(.*))?)?)?")
_TZ_RE = re.compile(r"(?:Z|(?:UTC|GMT|UT)?(?:([+-])(\d{1,2})(?::?(\d{1,2})(?::?(\d{1,2}))?)?)?)")


def _days_from_civil(y: int, mo: int, d: int) -> Optional[int]:
    """Days since 1970-01-01 of a proleptic Gregorian date (java.time.LocalDate, which Spark uses),
    for any year -- datetime.date stops at 1..9999 and the device does not; None for no such date."""
    leap = (y % 4 == 0 and y % 100 != 0) or y % 400 == 0
    if not 1 <= mo <= 12 or not 1 <= d <= (31, 29 if leap else 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)[mo - 1]:
        return None
    y -= mo <= 2
    era, yoe = divmod(y, 400)
    doy = (153 * (mo + (-3 if mo > 2 else 9)) + 2) // 5 + d - 1
    return era * 146097 + yoe * 365 + yoe // 4 - yoe // 100 + doy - 719468


def timestamp_micros(s: str) -> Optional[int]:
    """DateTimeUtils.stringToTimestamp with the session zone UTC, the subset the device reads."""
    t = _jtrim(s)
    m = _TS_RE.fullmatch(t)
    if not m:
        return None
    sign, y, mo, d, hh, mi, ss, frac, zone = m.groups()
    day = _days_from_civil(int(y) * (-1 if sign == "-" else 1), int(mo or 1), int(d or 1))
    if day is None:
        return None
    hh, mi, ss = int(hh or 0), int(mi or 0), int(ss or 0)
    if hh > 23 or mi > 59 or ss > 59:
        return None
    us = int(((frac or "") + "000000")[:6])
    off = 0
    if zone:
        z = _TZ_RE.fullmatch(_jtrim(zone))
        if not z or not zone.strip():
            return None
        if z.group(1):
            h, mn, sc = int(z.group(2)), int(z.group(3) or 0), int(z.group(4) or 0)
            if h > 18 or mn > 59 or sc > 59:
                return None
            off = (h * 3600 + mn * 60 + sc) * (-1 if z.group(1) == "-" else 1)
    return ((day * 86400 + hh * 3600 + mi * 60 + ss) - off) * 1_000_000 + us


def double_bits(x: float) -> int:
    """The binary64 bits of x."""
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def float_bits(x: float) -> int:
    """The binary32 bits of x; PredicateError unless binary32 holds x exactly."""
    try:
        b = struct.pack("<f", x)
    except OverflowError:
        raise PredicateError("float literal %r is not a binary32 value" % (x,))
    if x == x and struct.unpack("<f", b)[0] != x:
        raise PredicateError("float literal %r is not a binary32 value" % (x,))
    return struct.unpack("<I", b)[0]


def fp_order_key(bits: int, width: int = 64) -> int:
    """The device's floating-point order key (fp_key64 / fp_key32 of csrc/kernels.h) of a value's
    bits: every NaN canonical, -0.0 as +0.0, then the magnitude bits of negative values flipped.
    The signed integer order of the keys is SQLOrderingUtil.compareDoubles / compareFloats
    (-0.0 = 0.0, NaN = NaN, NaN above +Infinity)."""
    mag = (1 << (width - 1)) - 1
    inf, qnan = (0x7ff0000000000000, 0x7ff8000000000000) if width == 64 else (0x7f800000, 0x7fc00000)
    if bits & mag > inf:
        bits = qnan
    if bits == 1 << (width - 1):
        bits = 0
    k = bits - (1 << width) if bits >> (width - 1) else bits
    return k ^ mag if k < 0 else k


def decimal_bytes(unscaled: int) -> bytes:
    """A decimal literal's wire form: the unscaled value as 16 bytes, little-endian two's complement."""
    return int(unscaled).to_bytes(16, "little", signed=True)


def _decimal_unscaled(v, p: int, s: int) -> int:
    import decimal
    if isinstance(v, decimal.Decimal):
        ctx = decimal.Context(prec=200)
        u = v.scaleb(s, context=ctx) if v.is_finite() else None
        if u is None or u != u.to_integral_value(context=ctx):
            raise PredicateError("decimal literal %s does not quantise to scale %d exactly" % (v, s))
        u = int(u)
    elif isinstance(v, int) and not isinstance(v, bool):
        u = v
    else:
        raise PredicateError("decimal literal %r: the unscaled int or a decimal.Decimal expected" % (v,))
    if abs(u) >= 10 ** p:
        raise PredicateError("decimal literal %r does not fit precision %d" % (v, p))
    return u


def _timestamp_lit(v) -> int:
    if isinstance(v, str):
        us = timestamp_micros(v)
        if us is None:
            raise PredicateError("bad timestamp literal %r" % v)
        return us
    if isinstance(v, _dt.datetime):
        if v.tzinfo is None:  # the session zone: UTC
            v = v.replace(tzinfo=_dt.timezone.utc)
        d = v - _dt.datetime(1970, 1, 1, tzinfo=_dt.timezone.utc)
        return (d.days * 86400 + d.seconds) * 1_000_000 + d.microseconds
    if isinstance(v, int) and not isinstance(v, bool):
        return v
    raise PredicateError("bad timestamp literal %r" % (v,))


def _lit(typ: str, v):
    """Literal value as the device sees it (the oracle's _lit_value): dates as days since the
    epoch, booleans as 0/1, strings and binaries as bytes, floats and doubles as their bits,
    timestamps as microseconds, decimals as their 16 bytes."""
    code = type_code(typ)
    if code is None:
        raise PredicateError("unsupported literal type %r" % typ)
    if v is None:
        return None
    if code in (T_FLOAT, T_DOUBLE):
        if isinstance(v, bool) or not isinstance(v, (float, int)) or float(v) != v and v == v:
            raise PredicateError("%s literal %r: a float expected" % (typ, v))
        return float_bits(float(v)) if code == T_FLOAT else double_bits(float(v))
    if code == T_TIMESTAMP:
        return _timestamp_lit(v)
    if code == T_BINARY:
        if not isinstance(v, (bytes, bytearray)):
            raise PredicateError("binary literal %r: bytes expected" % (v,))
        return bytes(v)
    if code & 0xff == T_DECIMAL:
        return decimal_bytes(_decimal_unscaled(v, (code >> 8) & 0xff, code >> 16))
    if typ == "date":
        if isinstance(v, str):
            days = _date_days(v)
            if days is None:
                raise PredicateError("bad date literal %r" % v)
            return days
        if isinstance(v, _dt.date):
            return (v - _EPOCH).days
        return int(v)
    if typ == "boolean":
        return 1 if v else 0
    if typ == "string":
        return str(v).encode("utf-8")
    return int(v)


def like_escape_code(escape) -> int:
    """The escape character of a LIKE as DR_OP_LIKE's arg: one character, a code point in 1..0xFFFF
    and no surrogate (Like's escapeChar is a JVM Char)."""
    if not isinstance(escape, str) or len(escape) != 1 or not 1 <= ord(escape) <= 0xFFFF or 0xD800 <= ord(escape) <= 0xDFFF:
        raise PredicateError("like: the escape must be one character (a code point in 1..0xFFFF, no surrogate), got %r"
                             % (escape,))
    return ord(escape)


def check_like_pattern(pattern: str, escape: str) -> None:
    """StringUtils.escapeLikeRegex's two errors, with its texts (dr_filter reports the same)."""
    i = 0
    while i < len(pattern):
        if pattern[i] == escape:
            if i + 1 == len(pattern):
                raise PredicateError("the pattern '%s' is invalid, it is not allowed to end with the escape character"
                                     % pattern)
            if pattern[i + 1] not in ("_", "%", escape):
                raise PredicateError("the pattern '%s' is invalid, the escape character is not allowed to precede '%s'"
                                     % (pattern, pattern[i + 1]))
            i += 1
        i += 1


def build_program(schema: Dict[str, str], preds: Sequence) -> Program:
    """AND of `preds` lowered to the postfix program of include/deltareplay.h (dr_pred_op)."""
    if not preds:
        raise PredicateError("no predicates")
    p = Program()
    colidx: Dict[object, int] = {}  # partition columns by name, statistics by (source, path)
    parts = list(schema)

    def col(name):
        exact = _resolve(name, parts)
        if exact is None:
            raise PredicateError("%s is not a partition column" % name)
        typ = schema[exact]
        if type_code(typ) is None:
            raise PredicateError("partition column %s has unsupported type %s" % (exact, typ))
        if exact not in colidx:
            colidx[exact] = len(p.cols)
            p.cols.append((exact, type_code(typ)))
        p.ops.append((OP_COL, colidx[exact]))

    def stats_col(e):
        """("stats", source, path, type): a per-file statistic as a column whose type carries the
        source (DR_SRC_STATS_*); its name is the path's segments joined by 0x01."""
        if len(e) != 4 or type_code(e[3]) is None:
            raise PredicateError("bad statistics column %r" % (e,))
        key = (int(e[1]), "\x01".join(e[2]))
        if key not in colidx:
            colidx[key] = len(p.cols)
            p.cols.append((key[1], type_code(e[3]) | key[0] << N.DR_SRC_SHIFT))
        p.ops.append((OP_COL, colidx[key]))

    def lit(typ, v):
        value = _lit(typ, v)
        p.lits.append((type_code(typ), value))
        p.ops.append((OP_LIT, len(p.lits) - 1))

    def fits(a, b):
        """A literal compared with a column is of a kind the column takes (dr_filter's own rule)."""
        if a[0] != "col" or b[0] != "lit" or b[2] is None:
            return
        exact = _resolve(a[1], parts)
        ct, lt = type_code(schema[exact]) if exact is not None else None, type_code(b[1])
        if ct is None or lt is None:
            return  # reported by col() / lit()
        if (ct & 0xff >= T_FLOAT or lt & 0xff >= T_FLOAT) and not (ct == lt or (ct == T_FLOAT and lt == T_DOUBLE)):
            raise PredicateError("a %s literal does not fit partition column %s of type %s" % (b[1], exact, schema[exact]))

    def pattern(e):
        """A string pattern: the value a string partition column, the pattern a string or NULL literal."""
        op = e[0]
        if len(e) not in ((3, 4) if op == "like" else (3,)):
            raise PredicateError("%s takes a column and a literal%s" % (op, " and an optional escape" if op == "like" else ""))
        value, pat = e[1], e[2]
        exact = _resolve(value[1], parts) if value[0] == "col" else None
        if value[0] == "stats" and len(value) == 4 and value[3] == "string":
            pass  # a string statistic: the op's operand rule looks at the type alone
        elif value[0] != "col":
            raise PredicateError("%s: the value must be a string partition column, found %r" % (op, value[0]))
        if exact is not None and schema[exact] != "string":
            raise PredicateError("%s: the value must be a string partition column, %s is %s" % (op, exact, schema[exact]))
        if pat[0] != "lit":
            raise PredicateError("%s: the pattern must be a string or NULL literal, found %r" % (op, pat[0]))
        if pat[2] is not None and (pat[1] != "string" or not isinstance(pat[2], str)):
            raise PredicateError("%s: the pattern must be a string or NULL literal, found a %s literal %r"
                                 % (op, pat[1], pat[2]))
        arg = 0
        if op == "like":
            escape = e[3] if len(e) == 4 else "\\"
            arg = like_escape_code(escape)
            if pat[2] is not None:
                check_like_pattern(pat[2], escape)
        emit(value)
        emit(pat)
        p.ops.append((OP_CODE[op], arg))

    def value_type(e):
        """The type name of a column, a literal or a date function's result; None for anything else."""
        if e[0] == "col":
            exact = _resolve(e[1], parts)
            return schema[exact] if exact is not None else None
        if e[0] == "lit":
            return e[1]
        if e[0] == "stats":
            return e[3] if len(e) == 4 else None
        if e[0] in DATE_FN_CODE:
            return "integer" if DATE_FN_CODE[e[0]] < DATE_FN_CODE["to_date"] else "date"
        return None

    def date_fn(e):
        """A date function: the operand a column or another function of the operand's type."""
        op = e[0]
        if len(e) != (3 if op in DATE_FN_ARG_OPS else 2):
            raise PredicateError("%s takes %s" % (op, "an expression and a format" if op == "trunc" else
                                                  "an expression and a day count" if op in DATE_FN_ARG_OPS else "one expression"))
        want = "timestamp" if op == "to_date" else "date"
        x = e[1]
        if not isinstance(x, tuple) or (x[0] not in ("col", "stats") and x[0] not in DATE_FN_CODE):
            raise PredicateError("%s: the operand must be a %s partition column or date function, found %r"
                                 % (op, want, x[0] if isinstance(x, tuple) else x))
        if x[0] == "col" and _resolve(x[1], parts) is None:
            col(x[1])  # raises: no partition column
        if value_type(x) != want:
            raise PredicateError("%s: the operand must be a %s value, found %s of type %s"
                                 % (op, want, "column %s" % (x[1],) if x[0] in ("col", "stats") else x[0], value_type(x)))
        arg = 0
        if op == "trunc":
            if not isinstance(e[2], str) or e[2].lower() not in TRUNC_UNIT:
                raise PredicateError("trunc: the format must be one of YEAR, YYYY, YY, QUARTER, MONTH, MM, MON, WEEK, got %r"
                                     % (e[2],))
            arg = TRUNC_UNIT[e[2].lower()]
        elif op in DATE_FN_ARG_OPS:
            n = e[2]
            if isinstance(n, bool) or not isinstance(n, int) or not -(1 << 31) <= n < (1 << 31):
                raise PredicateError("%s: the day count must be an int in the int32 range, got %r" % (op, n))
            arg = n if op == "date_add" else ((-n + (1 << 31)) % (1 << 32)) - (1 << 31)  # Int subtraction wraps
        emit(x)
        p.ops.append((DATE_FN_CODE[op], arg))

    def fn_fits(a, b):
        """A date function's result `a` against `b`: a literal of its kind or NULL, or a column or
        function result of the same family (dr_filter's own rule)."""
        if a[0] not in DATE_FN_CODE:
            return
        rt, ot = value_type(a), value_type(b)
        same = (ot == "date") if rt == "date" else (ot in _INT_TYPES)
        if b[0] == "lit":
            if b[2] is not None and not same:
                raise PredicateError("a %s literal does not fit the result of %s (%s)" % (b[1], a[0], rt))
        elif not same and not (b[0] == "col" and ot is None):  # an unknown column is reported by col()
            raise PredicateError("the result of %s (%s) does not compare with %s%s"
                                 % (a[0], rt, b[0], " of type %s" % ot if ot else ""))

    def boolean(op, e):
        """A date function's result is an integer or a date, no boolean (dr_filter's own rule)."""
        if e[0] in DATE_FN_CODE:
            raise PredicateError("%s: the operand must be a boolean, found the result of %s (%s)"
                                 % (op, e[0], value_type(e)) if op else
                                 "a predicate must be a boolean, found the result of %s (%s)" % (e[0], value_type(e)))

    def emit(e):
        op = e[0]
        if op == "col":
            col(e[1])
        elif op == "lit":
            lit(e[1], e[2])
        elif op == "stats":
            stats_col(e)
        elif op == "in":
            emit(e[1])
            for l in e[2]:
                fits(e[1], l)
                fn_fits(e[1], l)
                fn_fits(l, e[1])
                emit(l)
            p.ops.append((OP_CODE["in"], len(e[2])))
        elif op in ("isnull", "isnotnull", "not"):
            if op == "not":
                boolean(op, e[1])
            emit(e[1])
            p.ops.append((OP_CODE[op], 0))
        elif op in PATTERN_OPS:
            pattern(e)
        elif op in DATE_FN_CODE:
            date_fn(e)
        elif op in OP_CODE:
            if op in ("and", "or"):
                boolean(op, e[1])
                boolean(op, e[2])
            else:
                fits(e[1], e[2])
                fits(e[2], e[1])
                fn_fits(e[1], e[2])
                fn_fits(e[2], e[1])
            emit(e[1])
            emit(e[2])
            p.ops.append((OP_CODE[op], 0))
        else:
            raise PredicateError("unsupported expression %r" % (op,))

    for e in preds:
        boolean(None, e)
    emit(preds[0])
    for e in preds[1:]:
        emit(e)
        p.ops.append((OP_CODE["and"], 0))
    return p


def lower_program(prog: Program):
    """ctypes dr_predicate for `prog` (+ the buffers that must outlive the call)."""
    keep = []
    nops = len(prog.ops)
    ops = (N.dr_pred_op * max(nops, 1))()
    for i, (o, a) in enumerate(prog.ops):
        ops[i] = N.dr_pred_op(o, a)
    ncols = len(prog.cols)
    names = (C.c_char_p * max(ncols, 1))()
    ctypes_ = (C.c_int32 * max(ncols, 1))()
    for i, (n, t) in enumerate(prog.cols):
        b = C.create_string_buffer(n.encode("utf-8"))
        keep.append(b)
        names[i] = C.cast(b, C.c_char_p)
        ctypes_[i] = t
    nl = len(prog.lits)
    lt = (C.c_int32 * max(nl, 1))()
    li = (C.c_int64 * max(nl, 1))()
    ln = (C.c_uint8 * max(nl, 1))()
    lo = (C.c_int64 * (nl + 1))()
    blob = b""
    for i, (t, v) in enumerate(prog.lits):
        lt[i] = t
        lo[i] = len(blob)
        if v is None:
            ln[i] = 1
        elif isinstance(v, bytes):
            blob += v
        else:
            li[i] = int(v) - (1 << 64) if int(v) >= 1 << 63 else int(v)  # a double's bits as int64
    lo[nl] = len(blob)
    lb = (C.c_uint8 * max(len(blob), 1)).from_buffer_copy(blob + b"\0")
    keep += [ops, names, ctypes_, lt, li, ln, lo, lb]
    pred = N.dr_predicate(nops, ops, ncols, names, ctypes_, nl, lt, li, ln, lo, lb)
    return pred, keep
