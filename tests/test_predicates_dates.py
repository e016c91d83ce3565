"""delta_amd.predicates over the date functions: the tuple forms lower to DR_OP_YEAR .. DR_OP_TRUNC_DATE
with their args, every `trunc` format spelling, the PredicateErrors for what dr_filter refuses, and the
metadata / data split seeing through the new forms. Nothing here evaluates a predicate."""
import pytest

from delta_amd import predicates as P

SCHEMA = {"dt": "date", "ts": "timestamp", "k": "integer", "s": "string"}
COL, LIT, OP = P.OP_COL, P.OP_LIT, P.OP_CODE
YEAR, QUARTER, MONTH, DAYOFMONTH, DAYOFWEEK, DAYOFYEAR, WEEKOFYEAR, TO_DATE, DATE_ADD, TRUNC = range(19, 29)

c = lambda n: ("col", n)  # noqa: E731
l = lambda t, v: ("lit", t, v)  # noqa: E731


def test_unary_forms_lower_to_their_opcodes():
    names = {"year": YEAR, "quarter": QUARTER, "month": MONTH, "dayofmonth": DAYOFMONTH, "dayofweek": DAYOFWEEK,
             "dayofyear": DAYOFYEAR, "weekofyear": WEEKOFYEAR}
    assert {k: P.DATE_FN_CODE[k] for k in names} == names
    for name, code in names.items():
        p = P.build_program(SCHEMA, [("=", (name, c("dt")), l("integer", 3))])
        assert p.ops == [(COL, 0), (code, 0), (LIT, 0), (OP["="], 0)], name
        assert p.cols == [("dt", P.type_code("date"))] and p.lits == [(P.type_code("integer"), 3)]
    p = P.build_program(SCHEMA, [("=", ("to_date", c("TS")), l("date", "2024-03-01"))])
    assert p.ops == [(COL, 0), (TO_DATE, 0), (LIT, 0), (OP["="], 0)] and p.cols == [("ts", P.T_TIMESTAMP)]
    assert p.lits == [(P.type_code("date"), 19783)]


def test_forms_with_an_argument():
    p = P.build_program(SCHEMA, [(">=", ("date_add", c("dt"), 7), l("date", "2024-03-08"))])
    assert p.ops == [(COL, 0), (DATE_ADD, 7), (LIT, 0), (OP[">="], 0)]
    # date_sub(x, n) is DATE_ADD of -n, with Int's wrap at -2^31
    for n, arg in ((7, -7), (-7, 7), (0, 0), (2 ** 31 - 1, -(2 ** 31 - 1)), (-2 ** 31, -2 ** 31)):
        p = P.build_program(SCHEMA, [("isnull", ("date_sub", c("dt"), n))])
        assert p.ops == [(COL, 0), (DATE_ADD, arg), (OP["isnull"], 0)], n
    for n in (2 ** 31 - 1, -2 ** 31):
        assert P.build_program(SCHEMA, [("isnull", ("date_add", c("dt"), n))]).ops[1] == (DATE_ADD, n)
    # they nest: year(ts) arrives as Year(Cast(ts AS date))
    p = P.build_program(SCHEMA, [("in", ("year", ("date_add", ("to_date", c("ts")), 1)), [l("integer", 2024), l("long", None)])])
    assert p.ops == [(COL, 0), (TO_DATE, 0), (DATE_ADD, 1), (YEAR, 0), (LIT, 0), (LIT, 1), (OP["in"], 2)]
    # the function on the right, and under NOT / AND with a plain leaf
    p = P.build_program(SCHEMA, [("<", l("integer", 3), ("month", c("dt"))), ("not", ("=", c("k"), ("quarter", c("dt"))))])
    assert p.ops == [(LIT, 0), (COL, 0), (MONTH, 0), (OP["<"], 0), (COL, 1), (COL, 0), (QUARTER, 0), (OP["="], 0), (OP["not"], 0),
                     (OP["and"], 0)]


def test_every_trunc_format_spelling():
    units = {"YEAR": 0, "YYYY": 0, "YY": 0, "QUARTER": 1, "MONTH": 2, "MM": 2, "MON": 2, "WEEK": 3}
    for fmt, arg in units.items():
        for spelling in (fmt, fmt.lower(), fmt.capitalize(), fmt[0].lower() + fmt[1:]):
            p = P.build_program(SCHEMA, [("=", ("trunc", c("dt"), spelling), l("date", "2024-03-01"))])
            assert p.ops == [(COL, 0), (TRUNC, arg), (LIT, 0), (OP["="], 0)], spelling
    for bad in ("DAY", "DD", "Y", "MONTHS", "", " MM", "WK", None, 2, ("lit", "string", "MM")):
        with pytest.raises(P.PredicateError, match="trunc: the format must be one of"):
            P.build_program(SCHEMA, [("isnull", ("trunc", c("dt"), bad))])


def test_operand_errors():
    cases = [
        (("year", c("k")), "year: the operand must be a date value, found column k of type integer"),
        (("month", c("ts")), "month: the operand must be a date value, found column ts of type timestamp"),
        (("to_date", c("dt")), "to_date: the operand must be a timestamp value, found column dt of type date"),
        (("date_add", c("s"), 1), "date_add: the operand must be a date value, found column s of type string"),
        (("trunc", c("ts"), "MM"), "trunc: the operand must be a date value, found column ts of type timestamp"),
        (("month", ("year", c("dt"))), "month: the operand must be a date value, found year of type integer"),
        (("to_date", ("to_date", c("ts"))), "to_date: the operand must be a timestamp value, found to_date of type date"),
        (("year", l("date", "2024-01-01")), "year: the operand must be a date partition column or date function, found 'lit'"),
        (("year", l("date", None)), "year: the operand must be a date partition column or date function, found 'lit'"),
        (("year", ("isnull", c("dt"))), "year: the operand must be a date partition column or date function, found 'isnull'"),
        (("year", c("nope")), "nope is not a partition column"),
        (("year",), "year takes one expression"),
        (("year", c("dt"), 1), "year takes one expression"),
        (("date_add", c("dt")), "date_add takes an expression and a day count"),
        (("trunc", c("dt")), "trunc takes an expression and a format"),
    ]
    for e, text in cases:
        with pytest.raises(P.PredicateError) as err:
            P.build_program(SCHEMA, [("isnull", e)])
        assert str(err.value) == text, e
    for n in (2 ** 31, -2 ** 31 - 1, 1.0, "1", None, True, l("integer", 1)):
        for op in ("date_add", "date_sub"):
            with pytest.raises(P.PredicateError, match="%s: the day count must be an int in the int32 range" % op):
                P.build_program(SCHEMA, [("isnull", (op, c("dt"), n))])


def test_literal_kind_errors():
    year, trunc = ("year", c("dt")), ("trunc", c("dt"), "MM")
    bad = [
        (("=", year, l("date", "2024-01-01")), "a date literal does not fit the result of year (integer)"),
        (("<", l("string", "2024"), year), "a string literal does not fit the result of year (integer)"),
        (("=", year, l("double", 2024.0)), "a double literal does not fit the result of year (integer)"),
        (("=", trunc, l("integer", 5)), "a integer literal does not fit the result of trunc (date)"),
        (("<=>", ("to_date", c("ts")), l("timestamp", 0)), "a timestamp literal does not fit the result of to_date (date)"),
        (("in", year, [l("integer", 1), l("date", 1)]), "a date literal does not fit the result of year (integer)"),
        (("in", ("date_add", c("dt"), 1), [l("string", "2024-01-01")]), "a string literal does not fit the result of date_add (date)"),
        (("=", ("month", c("dt")), c("s")), "the result of month (integer) does not compare with col of type string"),
        (("=", c("dt"), ("year", c("dt"))), "the result of year (integer) does not compare with col of type date"),
        (("=", ("date_add", c("dt"), 1), c("k")), "the result of date_add (date) does not compare with col of type integer"),
        (("=", year, ("to_date", c("ts"))), "the result of year (integer) does not compare with to_date of type date"),
        (("=", year, ("isnull", c("dt"))), "the result of year (integer) does not compare with isnull"),
    ]
    for e, text in bad:
        with pytest.raises(P.PredicateError) as err:
            P.build_program(SCHEMA, [e])
        assert str(err.value) == text, e
    ok = [("=", year, l(t, 5)) for t in ("byte", "short", "integer", "long")] + [
        ("=", year, l("string", None)), ("=", trunc, l("date", 5)), ("in", trunc, [l("date", "2024-03-01"), l("integer", None)]),
        ("=", ("month", c("dt")), c("k")), ("<", trunc, c("dt")), ("=", year, ("year", ("to_date", c("ts")))), ("isnotnull", year)]
    for e in ok:
        P.build_program(SCHEMA, [e])
    # the string patterns keep their rule: the value is a column
    with pytest.raises(P.PredicateError, match="like: the value must be a string partition column, found 'year'"):
        P.build_program(SCHEMA, [("like", year, l("string", "20%"))])


def test_a_function_result_is_no_boolean():
    year = ("year", c("dt"))
    ok = ("isnull", c("dt"))
    cases = [
        ([year], "a predicate must be a boolean, found the result of year (integer)"),
        ([ok, ("trunc", c("dt"), "MM")], "a predicate must be a boolean, found the result of trunc (date)"),
        ([("not", year)], "not: the operand must be a boolean, found the result of year (integer)"),
        ([("and", ok, year)], "and: the operand must be a boolean, found the result of year (integer)"),
        ([("or", ("date_add", c("dt"), 1), ok)], "or: the operand must be a boolean, found the result of date_add (date)"),
    ]
    for preds, text in cases:
        with pytest.raises(P.PredicateError) as err:
            P.build_program(SCHEMA, preds)
        assert str(err.value) == text, preds
    P.build_program(SCHEMA, [("not", ("isnull", year)), ("or", ok, ("=", year, l("integer", 1)))])


def test_split_sees_through_the_functions():
    parts = ["dt", "ts", "k"]
    y, m = ("=", ("year", c("dt")), l("integer", 2024)), ("in", ("month", c("DT")), [l("integer", 3)])
    data = ("=", ("year", c("event_day")), l("integer", 2024))
    mixed = ("or", ("=", ("trunc", c("dt"), "MM"), l("date", "2024-03-01")), (">", c("x"), l("long", 5)))
    add = (">=", ("date_add", ("to_date", c("ts")), 7), l("date", "2024-03-08"))
    meta, rest = P.split_metadata_and_data_predicates(("and", ("and", y, data), ("and", ("and", m, mixed), add)), parts)
    assert meta == [y, m, add] and rest == [data, mixed]
    assert P.is_partition_only(add, parts) and not P.is_partition_only(mixed, parts)
    # the day count and the format are no expressions: nothing is looked up in them
    assert P._refs(("date_sub", c("dt"), 7)) == ["dt"] and P._refs(("trunc", ("date_add", c("dt"), -1), "col")) == ["dt"]
    assert P._refs(("=", ("year", ("to_date", c("ts"))), c("k"))) == ["ts", "k"]
