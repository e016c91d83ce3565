"""Host side of K5 for timestamp, decimal, float, double and binary partition columns (no GPU):
literal encodings, the lowering's errors, the floating-point order key's Python twin, and the
corpus's non-vacuity (every predicate selects some files and not all, by the oracle)."""
import ctypes as C
import datetime as dt
import decimal
import itertools
import struct

import pytest

from delta_amd import predicates as P
from tests import filter_types_corpus as F

SCHEMA = dict(F.PTYPES)


def _lowered(schema, pred):
    prog = P.build_program(schema, [pred])
    cp, keep = P.lower_program(prog)
    lits = []
    for k in range(cp.nlits):
        raw = bytes(cp.lit_str_bytes[cp.lit_str_off[k]:cp.lit_str_off[k + 1]])
        lits.append((cp.lit_types[k], cp.lit_i64[k], cp.lit_null[k], raw))
    return prog, lits


def test_type_codes():
    assert P.type_code("float") == 7 and P.type_code("double") == 8 and P.type_code("timestamp") == 9
    assert P.type_code("binary") == 10 and P.type_code("decimal") == 11 | 10 << 8
    assert P.type_code("decimal(12,2)") == 11 | 12 << 8 | 2 << 16
    assert P.type_code("decimal(38,10)") == 11 | 38 << 8 | 10 << 16
    for bad in ("decimal(39,0)", "decimal(0,0)", "decimal(5,6)", "array<int>", "interval"):
        assert P.type_code(bad) is None


def test_literal_encodings_round_trip():
    col = ("col", "p")
    for x in (1.5, -0.0, 5e-324, 1e308, float("inf"), float("-inf"), 0.1):
        _, lits = _lowered({"p": "double"}, ("=", col, ("lit", "double", x)))
        t, i64, null, raw = lits[0]
        assert (t, null, raw) == (8, 0, b"")
        assert struct.unpack("<d", struct.pack("<q", i64))[0] == x
        assert struct.pack("<q", i64) == struct.pack("<d", x)  # the sign of zero too
    _, lits = _lowered({"p": "double"}, ("=", col, ("lit", "double", float("nan"))))
    assert struct.unpack("<d", struct.pack("<q", lits[0][1]))[0] != struct.unpack("<d", struct.pack("<q", lits[0][1]))[0]
    for x in (1.5, -0.0, 2.0 ** -149, 16777216.0, float("inf"), -2.5):
        _, lits = _lowered({"p": "float"}, ("=", col, ("lit", "float", x)))
        t, i64, null, raw = lits[0]
        assert (t, null, raw) == (7, 0, b"") and 0 <= i64 < 1 << 32  # zero-extended
        assert struct.pack("<I", i64) == struct.pack("<f", x)
    # a float column also takes a double literal
    prog, lits = _lowered({"p": "float"}, (">", col, ("lit", "double", 0.1)))
    assert prog.cols == [("p", 7)] and lits[0][0] == 8 and struct.pack("<q", lits[0][1]) == struct.pack("<d", 0.1)
    # decimals: 16 bytes, little-endian two's complement, the column's own (p, s) in the type code
    code = 11 | 38 << 8 | 10 << 16
    for u in (0, 1, -1, 1 << 63, (1 << 64) + 5, -(1 << 64), 10 ** 38 - 1, -(10 ** 38 - 1)):
        _, lits = _lowered({"p": "decimal(38,10)"}, ("=", col, ("lit", "decimal(38,10)", u)))
        t, _, null, raw = lits[0]
        assert (t, null, len(raw)) == (code, 0, 16)
        assert int.from_bytes(raw, "little", signed=True) == u
    _, lits = _lowered({"p": "decimal(12,2)"}, ("=", col, ("lit", "decimal(12,2)", decimal.Decimal("-12.30"))))
    assert lits[0][0] == 11 | 12 << 8 | 2 << 16 and int.from_bytes(lits[0][3], "little", signed=True) == -1230
    _, lits = _lowered({"p": "decimal"}, ("=", col, ("lit", "decimal", 7)))
    assert lits[0][0] == 11 | 10 << 8 and int.from_bytes(lits[0][3], "little", signed=True) == 7
    # timestamps: microseconds from an int, a datetime, a string in the partition values' grammar
    want = 1583065800123456
    for v in (want, dt.datetime(2020, 3, 1, 12, 30, 0, 123456), "2020-03-01 12:30:00.123456",
              dt.datetime(2020, 3, 1, 14, 30, 0, 123456, tzinfo=dt.timezone(dt.timedelta(hours=2))),
              "2020-03-01T14:30:00.123456+02:00"):
        _, lits = _lowered({"p": "timestamp"}, ("<", col, ("lit", "timestamp", v)))
        assert lits[0][:3] == (9, want, 0)
    _, lits = _lowered({"p": "timestamp"}, ("<", col, ("lit", "timestamp", -1)))
    assert lits[0][1] == -1
    _, lits = _lowered({"p": "binary"}, ("=", col, ("lit", "binary", b"\xff\x00z")))
    assert lits[0][0] == 10 and lits[0][3] == b"\xff\x00z"
    # NULL literals carry the type and no value
    for typ in ("double", "float", "timestamp", "binary", "decimal(12,2)"):
        _, lits = _lowered({"p": typ}, ("<=>", col, ("lit", typ, None)))
        assert lits[0][0] == P.type_code(typ) and lits[0][2] == 1 and lits[0][3] == b""


@pytest.mark.parametrize("schema,lit", [
    ({"p": "float"}, ("lit", "float", 0.1)),                       # not a binary32 value
    ({"p": "float"}, ("lit", "float", 1e39)),
    ({"p": "float"}, ("lit", "float", "1.5")),
    ({"p": "double"}, ("lit", "double", "1.5")),
    ({"p": "double"}, ("lit", "integer", 1)),                      # kinds that do not fit the column
    ({"p": "double"}, ("lit", "float", 1.5)),
    ({"p": "integer"}, ("lit", "double", 1.0)),
    ({"p": "long"}, ("lit", "timestamp", 5)),
    ({"p": "timestamp"}, ("lit", "long", 5)),
    ({"p": "timestamp"}, ("lit", "date", "2020-03-01")),
    ({"p": "string"}, ("lit", "binary", b"x")),
    ({"p": "binary"}, ("lit", "string", "x")),
    ({"p": "decimal(12,2)"}, ("lit", "decimal(12,3)", 1)),         # another (p, s): the caller widens
    ({"p": "decimal(12,2)"}, ("lit", "decimal(38,10)", 1)),
    ({"p": "decimal(12,2)"}, ("lit", "long", 1)),
    ({"p": "decimal(12,2)"}, ("lit", "decimal(12,2)", 10 ** 12)),  # |unscaled| >= 10^p
    ({"p": "decimal(12,2)"}, ("lit", "decimal(12,2)", -(10 ** 12))),
    ({"p": "decimal(12,2)"}, ("lit", "decimal(12,2)", decimal.Decimal("1.005"))),  # does not quantise exactly
    ({"p": "decimal(12,2)"}, ("lit", "decimal(12,2)", 1.5)),
    ({"p": "decimal(12,2)"}, ("lit", "decimal(40,2)", 1)),
    ({"p": "timestamp"}, ("lit", "timestamp", "yesterday")),
    ({"p": "timestamp"}, ("lit", "timestamp", 1.5)),
    ({"p": "binary"}, ("lit", "binary", "text")),
])
def test_literal_errors(schema, lit):
    for pred in (("=", ("col", "p"), lit), ("<", lit, ("col", "p")), ("in", ("col", "p"), [lit])):
        with pytest.raises(P.PredicateError):
            P.build_program(schema, [pred])


def test_unsupported_column_types_still_raise():
    for typ in ("array<int>", "decimal(39,1)", "interval"):
        with pytest.raises(P.PredicateError):
            P.build_program({"p": typ}, [("isnull", ("col", "p"))])


def test_order_key_is_compare_doubles():
    vals = [float("-inf"), -1.5, -0.0, 0.0, 5e-324, 1.0, float("inf"), float("nan")]
    keys = [P.fp_order_key(P.double_bits(v)) for v in vals]
    assert keys == sorted(keys) and keys[2] == keys[3] and len(set(keys)) == len(vals) - 1
    sign = lambda x: (x > 0) - (x < 0)  # noqa: E731
    for (a, ka), (b, kb) in itertools.product(zip(vals, keys), repeat=2):
        assert sign(ka - kb) == F.compare_doubles(a, b), (a, b)
    assert all(-(1 << 63) <= k < 1 << 63 for k in keys)
    # every NaN is one key, above +Infinity; binary32 alike
    for bits in (0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001, 0xffffffffffffffff):
        assert P.fp_order_key(bits) == keys[-1] > keys[-2]
    fvals = [float("-inf"), -1.5, -0.0, 0.0, 2.0 ** -149, 1.0, float("inf"), float("nan")]
    fkeys = [P.fp_order_key(P.float_bits(v), 32) for v in fvals]
    for (a, ka), (b, kb) in itertools.product(zip(fvals, fkeys), repeat=2):
        assert sign(ka - kb) == F.compare_doubles(a, b), (a, b)
    assert P.fp_order_key(0xffc00001, 32) == fkeys[-1] and all(-(1 << 31) <= k < 1 << 31 for k in fkeys)


def test_corpus_lowers_and_is_not_vacuous():
    """Every corpus predicate lowers, and by the oracle selects at least one file and not all of
    the table's live files."""
    files = [F._add(i) for i in F.live_indices()]
    assert len(files) == F.N_LIVE
    for c, vals in (("ts", F.TS), ("d", F.D), ("f", F.F), ("m", F.M), ("w", F.W), ("b", F.B)):
        assert {f["partitionValues"][c] for f in files} == set(vals), c
    for preds in F.PREDICATES:
        prog = P.build_program(SCHEMA, preds)
        P.lower_program(prog)
        n = len(F.expected(SCHEMA, files, preds))
        assert 0 < n < len(files), (preds, n)


def test_timestamps_beyond_datetime_years():
    """timestamp_micros (the literal and list_files cast) reads the years datetime cannot hold as the
    device and Spark do: it equals the corpus restatement on the years table's values, a literal of
    such a year lowers, and cast_partition_value gives the microseconds, not None."""
    for s in F.YEARS_TS:
        want = F.cast_timestamp_any_year(s, "timestamp")
        assert (None if s is None else P.timestamp_micros(s)) == want, s
        got = P.cast_partition_value(s, "timestamp")
        if want is None:
            assert got is None
        elif isinstance(got, int):
            assert got == want and not -62135596800000000 <= want <= 253402300799999999, s
        else:
            assert got == dt.datetime(1970, 1, 1, tzinfo=dt.timezone.utc) + dt.timedelta(microseconds=want)
    assert P.timestamp_micros("-0001-01-01 00:00:00") == -62198755200000000  # 719,893 days before the epoch
    assert sum(isinstance(P.cast_partition_value(s, "timestamp"), int) for s in F.YEARS_TS) == 6
    _, lits = _lowered({"p": "timestamp"}, ("<", ("col", "p"), ("lit", "timestamp", "-0044-03-15 10:00:00")))
    assert lits[0][:3] == (9, F.cast_timestamp_any_year("-0044-03-15 10:00:00", "timestamp"), 0)
    # the years corpus: lowers, and is not vacuous by its restatement
    files = [F._years_add(i) for i in range(F.N_YEARS)]
    assert {f["partitionValues"]["ts"] for f in files} == set(F.YEARS_TS)
    for preds in F.YEARS_PREDICATES:
        P.lower_program(P.build_program(F.YEARS_TYPES, preds))
        n = len(F.expected_years(F.YEARS_TYPES, files, preds))
        assert 0 < n < len(files), (preds, n)
