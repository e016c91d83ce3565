"""The K5 predicate planner (delta_amd/csrc/pred_plan.cpp) over the date functions DR_OP_YEAR ..
DR_OP_TRUNC_DATE, host build: every refusal of check_program with its status and full text, the first
fault in program order being the one reported, and the leaf plans -- the chain fields of FilterLeaf,
the mirrored `lit op chain(col)`, the bitmap of an integer IN, and what is left to the interpreter."""
import ctypes as C
import glob
import json
import os
import subprocess

import pytest

from delta_amd import predicates as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "delta_amd", "csrc")
LIB = os.path.join(ROOT, "build", "libpredplan_dates_host.so")
SRCS = [os.path.join(ROOT, "tests", "native", "pred_plan_dates_host.cpp"), os.path.join(CSRC, "pred_plan.cpp")]
DEPS = glob.glob(os.path.join(CSRC, "*.h")) + [os.path.join(ROOT, "include", "deltareplay.h")]
INVALID_ARG = 1
OP = P.OP_CODE
COL, LIT = P.OP_COL, P.OP_LIT
YEAR, QUARTER, MONTH, DAYOFMONTH, DAYOFWEEK, DAYOFYEAR, WEEKOFYEAR, TO_DATE, DATE_ADD, TRUNC = range(19, 29)
LEAF, AND, OR, NOT = 0, 1, 2, 3  # filter_plan.h LEAF_OP_*
STRING, SHORT, INT, LONG, DATE, BOOLEAN, DOUBLE, TIMESTAMP = 0, 2, 3, 4, 5, 6, 8, 9
COLS = [("dt", DATE), ("ts", TIMESTAMP), ("k", INT), ("s", STRING)]
SCHEMA = {"dt": "date", "ts": "timestamp", "k": "integer", "s": "string"}

c = lambda n: ("col", n)  # noqa: E731
l = lambda t, v: ("lit", t, v)  # noqa: E731


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in SRCS + DEPS):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O2", "-fPIC", "-shared", "-o", LIB] + SRCS)
    L = C.CDLL(LIB)
    L.ppd_check.restype = C.c_int
    L.ppd_plan.restype = C.c_int
    k = (C.c_int32 * 3)()
    L.ppd_constants(k)
    # at most four functions per leaf; six-field initialisers read as "no function"; eight fields before
    # the chain, which is its length and four (fn, arg) pairs
    assert list(k) == [4, 0, 4 * (8 + 1 + 2 * 4)]
    return L


def check(lib, ops, lits=(), cols=COLS):
    pred, keep = P.lower_program(P.Program(ops=list(ops), cols=list(cols), lits=list(lits)))
    msg = C.create_string_buffer(2048)
    return lib.ppd_check(C.byref(pred), msg, 2048), msg.value.decode("utf-8")


def plan(lib, prog) -> dict:
    pred, keep = P.lower_program(prog)
    out = C.create_string_buffer(1 << 16)
    assert lib.ppd_plan(C.byref(pred), out, 1 << 16) == 0
    return json.loads(out.value.decode("utf-8"))


def leaf_of(lib, *preds):
    return plan(lib, P.build_program(SCHEMA, list(preds)))["leaf"]


# ---- check_program ------------------------------------------------------------------------------------
def test_operand_refusals(lib):
    operand = "predicate op %d (%s): the operand must be a %s value, found %s"
    i5 = [(INT, 5)]
    cases = [
        ([(COL, 2), (YEAR, 0), (LIT, 0), (OP["="], 0)], i5, operand % (1, "YEAR", "DATE", "partition column k of type 3")),
        ([(COL, 1), (MONTH, 0), (LIT, 0), (OP["="], 0)], i5, operand % (1, "MONTH", "DATE", "partition column ts of type 9")),
        ([(COL, 3), (WEEKOFYEAR, 0), (LIT, 0), (OP["="], 0)], i5,
         operand % (1, "WEEKOFYEAR", "DATE", "partition column s of type 0")),
        ([(COL, 0), (TO_DATE, 0), (OP["isnull"], 0)], [], operand % (1, "TO_DATE", "TIMESTAMP", "partition column dt of type 5")),
        ([(COL, 2), (DATE_ADD, 3), (OP["isnull"], 0)], [], operand % (1, "DATE_ADD", "DATE", "partition column k of type 3")),
        ([(COL, 1), (TRUNC, 2), (OP["isnull"], 0)], [], operand % (1, "TRUNC_DATE", "DATE", "partition column ts of type 9")),
        # a literal, a NULL one included: Catalyst has folded those
        ([(LIT, 0), (YEAR, 0), (LIT, 1), (OP["="], 0)], [(DATE, 19000), (INT, 2022)],
         operand % (1, "YEAR", "DATE", "literal 0 of type 5")),
        ([(LIT, 0), (QUARTER, 0), (OP["isnull"], 0)], [(DATE, None)], operand % (1, "QUARTER", "DATE", "a NULL literal")),
        ([(LIT, 0), (TO_DATE, 0), (OP["isnull"], 0)], [(TIMESTAMP, 0)], operand % (1, "TO_DATE", "TIMESTAMP", "literal 0 of type 9")),
        # a function of the wrong result type, and something that is neither column nor function
        ([(COL, 0), (YEAR, 0), (MONTH, 0), (OP["isnull"], 0)], [],
         operand % (2, "MONTH", "DATE", "the result of op 1 (opcode 19)")),
        ([(COL, 1), (TO_DATE, 0), (TO_DATE, 0), (OP["isnull"], 0)], [],
         operand % (2, "TO_DATE", "TIMESTAMP", "the result of op 1 (opcode 26)")),
        ([(COL, 0), (OP["isnull"], 0), (DAYOFWEEK, 0)], [], operand % (2, "DAYOFWEEK", "DATE", "the result of op 1 (opcode 10)")),
    ]
    for ops, lits, text in cases:
        assert check(lib, ops, lits) == (INVALID_ARG, text), ops


def test_arg_refusals(lib):
    unit = "predicate op 1 (TRUNC_DATE): the unit (arg %d) must be 0 YEAR, 1 QUARTER, 2 MONTH or 3 WEEK"
    for arg in (4, -1, 2 ** 31 - 1, -2 ** 31):
        assert check(lib, [(COL, 0), (TRUNC, arg), (OP["isnull"], 0)]) == (INVALID_ARG, unit % arg)
    for arg in (0, 1, 2, 3):
        assert check(lib, [(COL, 0), (TRUNC, arg), (OP["isnull"], 0)]) == (0, "")
    names = {YEAR: "YEAR", QUARTER: "QUARTER", MONTH: "MONTH", DAYOFMONTH: "DAYOFMONTH", DAYOFWEEK: "DAYOFWEEK",
             DAYOFYEAR: "DAYOFYEAR", WEEKOFYEAR: "WEEKOFYEAR"}
    for fn, name in names.items():
        assert check(lib, [(COL, 0), (fn, 1), (OP["isnull"], 0)]) == (
            INVALID_ARG, "predicate op 1 (%s): takes no argument (arg 1 must be 0)" % name)
        assert check(lib, [(COL, 0), (fn, 0), (OP["isnull"], 0)]) == (0, "")
    assert check(lib, [(COL, 1), (TO_DATE, -7), (OP["isnull"], 0)]) == (
        INVALID_ARG, "predicate op 1 (TO_DATE): takes no argument (arg -7 must be 0)")
    for n in (0, 7, -7, 2 ** 31 - 1, -2 ** 31):  # DATE_ADD takes any day count
        assert check(lib, [(COL, 0), (DATE_ADD, n), (OP["isnull"], 0)]) == (0, "")
    # no such opcode beyond the last
    assert check(lib, [(COL, 0), (29, 0), (OP["isnull"], 0)]) == (INVALID_ARG, "unknown predicate opcode 29")
    assert check(lib, [(YEAR, 0)]) == (INVALID_ARG, "predicate stack underflow")


def test_literal_kind_refusals(lib):
    fit = "predicate literal %d (type %d) does not fit the result of op %d (%s, type %d)"
    year = [(COL, 0), (YEAR, 0)]
    trunc = [(COL, 0), (TRUNC, 2)]
    for op in ("=", "!=", "<", "<=", ">", ">=", "<=>"):
        assert check(lib, year + [(LIT, 0), (OP[op], 0)], [(DATE, 19000)]) == (INVALID_ARG, fit % (0, DATE, 1, "YEAR", INT)), op
        assert check(lib, [(LIT, 0)] + year + [(OP[op], 0)], [(DATE, 19000)]) == (INVALID_ARG, fit % (0, DATE, 2, "YEAR", INT)), op
        assert check(lib, trunc + [(LIT, 0), (OP[op], 0)], [(INT, 5)]) == (INVALID_ARG, fit % (0, INT, 1, "TRUNC_DATE", DATE)), op
    for t, v in ((STRING, b"2024"), (BOOLEAN, 1), (DOUBLE, 0), (TIMESTAMP, 0)):
        assert check(lib, year + [(LIT, 0), (OP["="], 0)], [(t, v)]) == (INVALID_ARG, fit % (0, t, 1, "YEAR", INT)), t
    for t, v in ((STRING, b"2024-01-01"), (LONG, 5), (TIMESTAMP, 0)):
        assert check(lib, [(COL, 1), (TO_DATE, 0), (LIT, 0), (OP["="], 0)], [(t, v)]) == (
            INVALID_ARG, fit % (0, t, 1, "TO_DATE", DATE)), t
        assert check(lib, [(COL, 0), (DATE_ADD, 1), (LIT, 0), (OP["<"], 0)], [(t, v)]) == (
            INVALID_ARG, fit % (0, t, 1, "DATE_ADD", DATE)), t
    # the second IN element
    assert check(lib, year + [(LIT, 0), (LIT, 1), (OP["in"], 2)], [(INT, 2024), (DATE, 1)]) == (
        INVALID_ARG, fit % (1, DATE, 1, "YEAR", INT))
    # what fits: BYTE .. LONG for an INT result, DATE for a DATE result, NULL of any type for both
    for t in (1, SHORT, INT, LONG):
        assert check(lib, year + [(LIT, 0), (OP["="], 0)], [(t, 5)]) == (0, "")
    assert check(lib, trunc + [(LIT, 0), (OP["="], 0)], [(DATE, 5)]) == (0, "")
    for t in (STRING, INT, DATE, DOUBLE):
        assert check(lib, year + [(LIT, 0), (OP["<=>"], 0)], [(t, None)]) == (0, "")
        assert check(lib, trunc + [(LIT, 0), (LIT, 1), (OP["in"], 2)], [(DATE, 3), (t, None)]) == (0, "")


def test_column_and_function_peers(lib):
    peer = "predicate op %d: the result of op %d (%s, type %d) does not compare with %s"
    cases = [
        ([(COL, 0), (MONTH, 0), (COL, 3), (OP["="], 0)], peer % (3, 1, "MONTH", INT, "partition column s of type 0")),
        ([(COL, 3), (COL, 0), (MONTH, 0), (OP["<"], 0)], peer % (3, 2, "MONTH", INT, "partition column s of type 0")),
        ([(COL, 0), (DATE_ADD, 1), (COL, 2), (OP["="], 0)], peer % (3, 1, "DATE_ADD", DATE, "partition column k of type 3")),
        ([(COL, 0), (YEAR, 0), (COL, 0), (OP["="], 0)], peer % (3, 1, "YEAR", INT, "partition column dt of type 5")),
        ([(COL, 0), (YEAR, 0), (COL, 1), (TO_DATE, 0), (OP["="], 0)],
         peer % (4, 1, "YEAR", INT, "the result of op 3 (opcode 26)")),
        ([(COL, 0), (YEAR, 0), (COL, 0), (OP["isnull"], 0), (OP["="], 0)],
         peer % (4, 1, "YEAR", INT, "the result of op 3 (opcode 10)")),
        ([(COL, 0), (TRUNC, 0), (COL, 2), (OP["in"], 1)], peer % (3, 1, "TRUNC_DATE", DATE, "partition column k of type 3")),
    ]
    for ops, text in cases:
        assert check(lib, ops) == (INVALID_ARG, text), ops
    legal = [
        [(COL, 0), (MONTH, 0), (COL, 2), (OP["="], 0)],                       # month(dt) = k
        [(COL, 2), (COL, 0), (MONTH, 0), (OP["<"], 0)],                       # k < month(dt)
        [(COL, 0), (YEAR, 0), (COL, 1), (TO_DATE, 0), (YEAR, 0), (OP["="], 0)],  # year(dt) = year(to_date(ts))
        [(COL, 0), (TRUNC, 2), (COL, 0), (OP["="], 0)],                       # trunc(dt, 'MM') = dt
        [(COL, 1), (TO_DATE, 0), (COL, 0), (DATE_ADD, -1), (OP["<=>"], 0)],
        [(COL, 1), (TO_DATE, 0), (DATE_ADD, 1), (YEAR, 0), (OP["isnotnull"], 0)],
        [(COL, 0), (YEAR, 0), (OP["isnull"], 0)],
    ]
    for ops in legal:
        assert check(lib, ops) == (0, ""), ops


def test_pattern_ops_still_want_a_column(lib):
    assert check(lib, [(COL, 0), (YEAR, 0), (LIT, 0), (OP["like"], 92)], [(STRING, b"2%")]) == (
        INVALID_ARG, "predicate op 3 (LIKE): the value must be a STRING partition column, found the result of op 1 (opcode 19)")
    assert check(lib, [(COL, 3), (COL, 0), (YEAR, 0), (OP["contains"], 0)]) == (
        INVALID_ARG, "predicate op 3 (CONTAINS): the pattern must be a STRING or NULL literal, found the result of op 2 (opcode 19)")


def test_first_fault_in_program_order(lib):
    operand = "predicate op 1 (YEAR): the operand must be a DATE value, found partition column k of type 3"
    unit = "predicate op %d (TRUNC_DATE): the unit (arg 9) must be 0 YEAR, 1 QUARTER, 2 MONTH or 3 WEEK"
    fit = "predicate literal 0 (type 5) does not fit the result of op 1 (YEAR, type 3)"
    cases = [
        # a bad operand, then a bad unit / the other way round (both in one AND)
        ([(COL, 2), (YEAR, 0), (OP["isnull"], 0), (COL, 0), (TRUNC, 9), (OP["isnull"], 0), (OP["and"], 0)], operand),
        ([(COL, 0), (TRUNC, 9), (OP["isnull"], 0), (COL, 2), (YEAR, 0), (OP["isnull"], 0), (OP["and"], 0)], unit % 1),
        # within one op: the operand before the arg
        ([(COL, 2), (TRUNC, 9), (OP["isnull"], 0)],
         "predicate op 1 (TRUNC_DATE): the operand must be a DATE value, found partition column k of type 3"),
        # a literal that does not fit, then an unknown opcode / the other way round
        ([(COL, 0), (YEAR, 0), (LIT, 0), (OP["="], 0), (99, 0)], fit),
        ([(COL, 0), (99, 0), (YEAR, 0), (LIT, 0), (OP["="], 0)], "unknown predicate opcode 99"),
        # a bad unit below a comparison whose literal does not fit either
        ([(COL, 0), (TRUNC, 9), (LIT, 0), (OP["="], 0)], unit % 1),
        # a literal index out of range before the function that would refuse it
        ([(LIT, 3), (YEAR, 0), (OP["isnull"], 0)], "predicate literal index out of range"),
    ]
    for ops, text in cases:
        assert check(lib, ops, [(DATE, 19000)]) == (INVALID_ARG, text), ops


def test_a_function_result_is_no_boolean(lib):
    """An INT or a DATE under AND / OR / NOT, or as the program's value, is refused: the evaluators would
    read it as a truth value."""
    under = "predicate op %d (%s): the operand must be a boolean, found the result of op %d (%s, type %d)"
    isnull = [(COL, 0), (OP["isnull"], 0)]
    cases = [
        ([(COL, 0), (QUARTER, 0)], "predicate program must leave a boolean, op 1 (QUARTER) leaves a value of type 3"),
        ([(COL, 0), (DATE_ADD, 1)], "predicate program must leave a boolean, op 1 (DATE_ADD) leaves a value of type 5"),
        ([(COL, 0), (MONTH, 0), (OP["not"], 0)], under % (2, "NOT", 1, "MONTH", INT)),
        (isnull + [(COL, 0), (MONTH, 0), (OP["and"], 0)], under % (4, "AND", 3, "MONTH", INT)),
        ([(COL, 0), (TRUNC, 1)] + isnull + [(OP["or"], 0)], under % (4, "OR", 1, "TRUNC_DATE", DATE)),
        # the first fault in program order: the bad unit before the OR above it
        ([(COL, 0), (TRUNC, 7)] + isnull + [(OP["or"], 0)],
         "predicate op 1 (TRUNC_DATE): the unit (arg 7) must be 0 YEAR, 1 QUARTER, 2 MONTH or 3 WEEK"),
    ]
    for ops, text in cases:
        assert check(lib, ops) == (INVALID_ARG, text), ops
    assert check(lib, [(COL, 0), (MONTH, 0), (OP["isnull"], 0), (OP["not"], 0)]) == (0, "")


# ---- the plans ------------------------------------------------------------------------------------------
def test_function_leaves(lib):
    leaf = leaf_of(lib, ("=", ("year", c("dt")), l("integer", 2024)))
    assert leaf == {"leaves": [{"col": 0, "op": OP["="], "lit": 0, "nlit": 0, "lit_null": 0, "pad": 0, "fns": [[YEAR, 0]]}],
                    "prog": [LEAF, 0], "i64": [2024]}
    # innermost first; date_sub is DATE_ADD of -n; the literal slots hold plain integers
    leaf = leaf_of(lib, (">=", ("trunc", ("date_sub", ("to_date", c("ts")), 1), "week"), l("date", "2024-03-04")))
    assert leaf["leaves"] == [{"col": 0, "op": OP[">="], "lit": 0, "nlit": 0, "lit_null": 0, "pad": 0,
                               "fns": [[TO_DATE, 0], [DATE_ADD, -1], [TRUNC, 3]]}]
    assert leaf["i64"] == [19786]
    # a long literal against an INT result, a NULL one, IS [NOT] NULL
    leaf = leaf_of(lib, ("<", ("dayofyear", c("dt")), l("long", 2 ** 40)), ("<=>", ("quarter", c("dt")), l("integer", None)),
                   ("isnotnull", ("weekofyear", c("dt"))), ("isnull", c("dt")))
    assert [(f["op"], f["lit_null"], f["fns"]) for f in leaf["leaves"]] == [
        (OP["<"], 0, [[DAYOFYEAR, 0]]), (OP["<=>"], 1, [[QUARTER, 0]]), (OP["isnotnull"], 0, [[WEEKOFYEAR, 0]]),
        (OP["isnull"], 0, [])]
    assert leaf["i64"][0] == 2 ** 40 and leaf["prog"] == [LEAF, 0, LEAF, 1, AND, 0, LEAF, 2, AND, 0, LEAF, 3, AND, 0]
    # plain leaves beside function leaves keep an empty chain
    leaf = leaf_of(lib, ("or", ("=", c("k"), l("integer", 3)), ("not", ("=", ("month", c("dt")), l("integer", 3)))))
    assert [f["fns"] for f in leaf["leaves"]] == [[], [[MONTH, 0]]] and leaf["prog"] == [LEAF, 0, LEAF, 1, NOT, 0, OR, 0]


def test_literal_first_comparisons_are_mirrored(lib):
    mirror = {"<": ">", ">": "<", "<=": ">=", ">=": "<=", "=": "=", "!=": "!=", "<=>": "<=>"}
    for op, want in mirror.items():
        leaf = leaf_of(lib, (op, l("integer", 5), ("month", c("dt"))))
        assert leaf["leaves"] == [{"col": 0, "op": OP[want], "lit": 0, "nlit": 0, "lit_null": 0, "pad": 0, "fns": [[MONTH, 0]]}], op
        assert leaf["i64"] == [5]
        same = leaf_of(lib, (op, ("month", c("dt")), l("integer", 5)))
        assert same["leaves"][0]["op"] == OP[op] and same["leaves"][0]["fns"] == [[MONTH, 0]], op


def test_in_over_a_function(lib):
    # eight months: a bitmap (pad 1; literals [min, words, bits])
    months = [3, 1, 12, 7, 5, 6, 8, 9, 3]
    leaf = leaf_of(lib, ("in", ("month", c("dt")), [l("integer", m) for m in months] + [l("integer", None)]))
    assert leaf["leaves"] == [{"col": 0, "op": OP["in"], "lit": 0, "nlit": 8, "lit_null": 1, "pad": 1, "fns": [[MONTH, 0]]}]
    assert leaf["i64"] == [1, 1, sum(1 << (m - 1) for m in set(months))]
    # fewer than eight: a sorted set; of a DATE result too, and a bitmap of dates
    leaf = leaf_of(lib, ("in", ("dayofweek", c("dt")), [l("integer", 7), l("integer", 1)]))
    assert leaf["leaves"][0]["pad"] == 0 and leaf["leaves"][0]["nlit"] == 2 and leaf["i64"] == [1, 7]
    leaf = leaf_of(lib, ("in", ("trunc", c("dt"), "MM"), [l("date", "2024-03-01"), l("date", "2024-02-01")]))
    assert leaf["leaves"][0]["pad"] == 0 and leaf["i64"] == [19754, 19783] and leaf["leaves"][0]["fns"] == [[TRUNC, 2]]
    firsts = ["2024-%02d-01" % m for m in range(1, 9)]
    leaf = leaf_of(lib, ("in", ("trunc", ("to_date", c("ts")), "MM"), [l("date", d) for d in firsts]))
    assert leaf["leaves"][0]["pad"] == 1 and leaf["i64"][:2] == [19723, 4] and leaf["leaves"][0]["fns"] == [[TO_DATE, 0], [TRUNC, 2]]


def test_what_is_left_to_the_interpreter(lib):
    four = ("year", ("date_add", ("trunc", ("date_add", c("dt"), 1), "yy"), -1))
    pl = plan(lib, P.build_program(SCHEMA, [("=", four, l("integer", 2023))]))
    assert pl["leaf"]["leaves"][0]["fns"] == [[DATE_ADD, 1], [TRUNC, 0], [DATE_ADD, -1], [YEAR, 0]]
    five = ("year", ("date_add", ("trunc", ("date_add", ("to_date", c("ts")), 1), "yy"), -1))
    generic = [
        ([("=", five, l("integer", 2023))],
         [(COL, 0), (TO_DATE, 0), (DATE_ADD, 1), (TRUNC, 0), (DATE_ADD, -1), (YEAR, 0), (LIT, 0), (OP["="], 0)]),
        ([("=", ("year", c("dt")), ("year", ("to_date", c("ts"))))],
         [(COL, 0), (YEAR, 0), (COL, 1), (TO_DATE, 0), (YEAR, 0), (OP["="], 0)]),
        ([("=", ("month", c("dt")), c("k"))], [(COL, 0), (MONTH, 0), (COL, 1), (OP["="], 0)]),
        # one such comparison sends the whole predicate there
        ([("=", c("k"), l("integer", 1)), ("isnull", five)],
         [(COL, 0), (LIT, 0), (OP["="], 0), (COL, 1), (TO_DATE, 0), (DATE_ADD, 1), (TRUNC, 0), (DATE_ADD, -1), (YEAR, 0),
          (OP["isnull"], 0), (OP["and"], 0)]),
    ]
    for preds, lowered in generic:
        pl = plan(lib, P.build_program(SCHEMA, preds))
        assert pl["leaf"] is None, preds
        assert list(zip(pl["lowered"][0::2], pl["lowered"][1::2])) == lowered, preds
    # an IN over a function with a column among its elements
    pl = plan(lib, P.Program(ops=[(COL, 0), (MONTH, 0), (LIT, 0), (COL, 2), (OP["in"], 2)], cols=COLS, lits=[(INT, 3)]))
    # value, function, IN_START, two elements each with its IN_STEP, IN_END
    assert pl["leaf"] is None and len(pl["lowered"]) == 2 * 8


def test_sanitized_standalone_fuzz_with_date_chains():
    """tests/native/pred_plan_dates_fuzz.cpp under ASan + UBSan, run directly: arbitrary programs with chains
    of the date functions over well-formed arrays, every array in a heap block of exactly its length."""
    src = os.path.join(ROOT, "tests", "native", "pred_plan_dates_fuzz.cpp")
    exe = os.path.join(ROOT, "build", "pred_plan_dates_fuzz")
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in [src, SRCS[1]] + DEPS):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-fno-omit-frame-pointer", "-o", exe, src, SRCS[1]])
    r = subprocess.run([exe, "40000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fuzz ok" in r.stdout, r.stdout + r.stderr
