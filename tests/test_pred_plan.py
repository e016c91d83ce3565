"""The K5 predicate planner (delta_amd/csrc/pred_plan.cpp: check_program, compile_patterns,
lower_program, leafify), host build, called through ctypes with the dr_predicate that
predicates.lower_program makes -- what dr_filter runs before it launches anything. The corpora's
programs, the rejections the GPU tests provoke (status and full text), the structural failures and the
properties of the plans (operand swap, IN sets, the bitmap rule, FLOAT / DOUBLE widening, LIKE folds).
A stand-alone program fuzzes the same functions under AddressSanitizer and UndefinedBehaviorSanitizer."""
import ctypes as C
import glob
import json
import os
import subprocess

import pytest

from delta_amd import predicates as P
from tests import filter_like_corpus as FL
from tests import filter_types_corpus as FT
from tests.test_like_lane import compile_pattern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "delta_amd", "csrc")
LIB = os.path.join(ROOT, "build", "libpredplan_host.so")
LK_LIB = os.path.join(ROOT, "build", "liblikelane_host.so")
DEPS = [os.path.join(CSRC, "pred_plan.cpp")] + glob.glob(os.path.join(CSRC, "*.h")) + [
    os.path.join(ROOT, "include", "deltareplay.h")]
INVALID_ARG, UNSUPPORTED = 1, 12
OP = P.OP_CODE
COL, LIT = P.OP_COL, P.OP_LIT
PV_MAXC, PV_STACK = 16, 32  # filter_plan.h
LEAF, AND, OR, NOT = 0, 1, 2, 3  # filter_plan.h LEAF_OP_*
IN_START, IN_STEP, IN_END = 100, 101, 102  # filter_plan.h FILTER_OP_IN_*
INT, LONG, STRING, BINARY = (P.type_code(t) for t in ("integer", "long", "string", "binary"))
FLOAT, DOUBLE = P.T_FLOAT, P.T_DOUBLE

c = lambda n: ("col", n)  # noqa: E731
l = lambda t, v: ("lit", t, v)  # noqa: E731


def _stale(out, *srcs):
    return not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs)


def _build(out, srcs, deps, flags):
    if _stale(out, *srcs, *deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + ["-o", out] + srcs)


@pytest.fixture(scope="module")
def lib():
    _build(LIB, [os.path.join(ROOT, "tests", "native", "pred_plan_host.cpp"), DEPS[0]], DEPS[1:], ["-O2", "-fPIC", "-shared"])
    L = C.CDLL(LIB)
    L.pp_check.restype = C.c_int
    L.pp_plan.restype = C.c_int
    k = (C.c_int32 * 9)()
    L.pp_constants(k)  # the names above are filter_plan.h's values
    assert list(k) == [PV_MAXC, PV_STACK, LEAF, AND, OR, NOT, IN_START, IN_STEP, IN_END]
    return L


@pytest.fixture(scope="module")
def lk_lib():
    _build(LK_LIB, [os.path.join(ROOT, "tests", "native", "like_lane_host.cpp")], [os.path.join(CSRC, "like_lane.h")],
           ["-O2", "-fPIC", "-shared"])
    L = C.CDLL(LK_LIB)
    L.lk_compile.restype = C.c_int
    return L


def check(lib, prog):
    """(status, message) of check_program."""
    pred, keep = P.lower_program(prog)
    msg = C.create_string_buffer(2048)
    return lib.pp_check(C.byref(pred), msg, 2048), msg.value.decode("utf-8")


def plan_text(lib, prog) -> str:
    pred, keep = P.lower_program(prog)
    out = C.create_string_buffer(1 << 20)
    assert lib.pp_plan(C.byref(pred), out, 1 << 20) == 0
    return out.value.decode("utf-8")


def plan(lib, prog) -> dict:
    return json.loads(plan_text(lib, prog))


def corpus_programs():
    """(name, Program) of every corpus predicate."""
    for k, preds in enumerate(FT.PREDICATES):
        yield "types%d" % k, P.build_program(FT.PTYPES, preds)
    for k, preds in enumerate(FT.YEARS_PREDICATES):
        yield "years%d" % k, P.build_program(FT.YEARS_TYPES, preds)
    for k, preds in enumerate(list(FL.PREDICATES) + FL.ALWAYS_NULL + FL.NEVER_TRUE):
        yield "like%d" % k, P.build_program(FL.PTYPES, preds)


def u64(x):
    return x & (2 ** 64 - 1)


def i64(x):
    x = u64(x)
    return x - 2 ** 64 if x >= 2 ** 63 else x


def dkey(v):
    return P.fp_order_key(P.double_bits(v), 64)


def fkey(v):
    return P.fp_order_key(P.float_bits(v), 32)


# ---- the corpora ------------------------------------------------------------------------------------
def test_corpus_programs_pass_and_take_the_leaf_path(lib):
    """Every corpus predicate is columns against literals of their kind under AND / OR / NOT, which is
    what the leaf kernels evaluate (filter_eval 0 and 1 run them there; 2 forces the interpreter): each
    passes check_program, leafifies, and also lowers for the interpreter."""
    n = 0
    for name, prog in corpus_programs():
        assert check(lib, prog) == (0, ""), name
        pl = plan(lib, prog)
        assert pl["leaf"] is not None and pl["lowered"] is not None, name
        assert pl["compiled"] == any(o == OP["like"] and prog.lits[prog.ops[k - 1][1]][1] is not None
                                     for k, (o, _) in enumerate(prog.ops)), name
        leaf = pl["leaf"]
        nslots = len(leaf["i64"])
        assert len(leaf["i64hi"]) == nslots == len(leaf["str"]), name
        assert leaf["prog"][0::2].count(LEAF) == len(leaf["leaves"]), name
        for f in leaf["leaves"]:
            assert 0 <= f["col"] < len(prog.cols), name
            if f["op"] not in (OP["isnull"], OP["isnotnull"]):
                width = 2 + leaf["i64"][f["lit"] + 1] if f["pad"] == 1 else f["nlit"] if f["op"] == OP["in"] else 1
                assert 0 <= f["lit"] and f["lit"] + width <= nslots, name
        n += 1
    assert n == len(FT.PREDICATES) + len(FT.YEARS_PREDICATES) + len(FL.PREDICATES) + len(FL.ALWAYS_NULL) + len(FL.NEVER_TRUE)


# ---- rejections dr_filter reports (tests/test_gpu_filter_types.py, tests/test_gpu_filter_like.py) ----
def test_literal_rejections(lib):
    code = P.type_code("decimal(12,2)")
    other = P.type_code("decimal(12,3)")
    eq = [(COL, 0), (LIT, 1), (OP["="], 0), (COL, 0), (LIT, 0), (OP["="], 0), (OP["or"], 0)]
    ok = P.decimal_bytes(125)
    size = "decimal literal 1 must be 16 bytes (little-endian two's complement)"
    fit = "predicate literal 1 (type %d) does not fit partition column m (type %d)"
    for bad_type, bad, text in ((code, ok[:15], size), (code, ok + b"\0", size),
                                (code, P.decimal_bytes(10 ** 12), "decimal literal 1 does not fit precision 12"),
                                (other, ok, fit % (other, code)), (DOUBLE, 5, fit % (DOUBLE, code)),
                                (99, 5, "predicate literal 1 has no valid type (code 99)")):
        prog = P.Program(ops=eq, cols=[("m", code)], lits=[(code, ok), (bad_type, bad)])
        assert check(lib, prog) == (INVALID_ARG, text)
    # the same rule for an IN element, and for `lit op col`
    prog = P.Program(ops=[(COL, 0), (LIT, 0), (LIT, 1), (OP["in"], 2)], cols=[("d", DOUBLE)], lits=[(DOUBLE, 1), (FLOAT, 1)])
    assert check(lib, prog) == (INVALID_ARG, "predicate literal 1 (type 7) does not fit partition column d (type 8)")
    prog = P.Program(ops=[(LIT, 0), (COL, 0), (OP["<"], 0)], cols=[("n", INT)], lits=[(P.T_TIMESTAMP, 1)])
    assert check(lib, prog) == (INVALID_ARG, "predicate literal 0 (type 9) does not fit partition column n (type 3)")


def test_pattern_rejections(lib):
    cols = [("s", STRING), ("b", BINARY), ("n", INT)]
    like = OP["like"]
    s_pat = [(STRING, b"a%")]
    value = "predicate op 2 (%s): the value must be a STRING partition column, found %s"
    pat = "predicate op 2 (%s): the pattern must be a STRING or NULL literal, found %s"
    esc = "predicate op 2 (LIKE): the escape character (arg %d) must be a code point in 1..0xFFFF and no surrogate"
    cases = [
        ([(COL, 2), (LIT, 0), (like, 92)], s_pat, value % ("LIKE", "partition column n of type 3")),
        ([(COL, 1), (LIT, 0), (OP["startswith"], 0)], s_pat, value % ("STARTSWITH", "partition column b of type 10")),
        ([(COL, 0), (COL, 0), (OP["contains"], 0)], s_pat, pat % ("CONTAINS", "partition column s of type 0")),
        ([(LIT, 0), (LIT, 0), (OP["endswith"], 0)], s_pat, value % ("ENDSWITH", "literal 0 of type 0")),
        ([(COL, 0), (LIT, 0), (OP["endswith"], 0)], [(INT, 5)], pat % ("ENDSWITH", "literal 0 of type 3")),
        ([(COL, 0), (COL, 0), (OP["isnull"], 0), (like, 92)], s_pat, "predicate op 3 (LIKE): the pattern must be a STRING or NULL "
         "literal, found the result of op 2 (opcode 10)"),
        ([(COL, 0), (LIT, 0), (like, 92)], [(STRING, b"abc\\")], "predicate op 2 (LIKE): the pattern 'abc\\' is invalid, it is not "
         "allowed to end with the escape character"),
        ([(COL, 0), (LIT, 0), (like, 92)], [(STRING, b"a\\bc")], "predicate op 2 (LIKE): the pattern 'a\\bc' is invalid, the escape "
         "character is not allowed to precede 'b'"),
        ([(COL, 0), (LIT, 0), (like, 0)], s_pat, esc % 0),
        ([(COL, 0), (LIT, 0), (like, 0x10000)], s_pat, esc % 0x10000),
        ([(COL, 0), (LIT, 0), (like, 0xD800)], s_pat, esc % 0xD800),
        ([(COL, 0), (LIT, 0), (like, 0)], [(STRING, None)], esc % 0),
        ([(COL, 0), (LIT, 0), (like, 92)], [(STRING, b"a\xff%")], "predicate op 2 (LIKE): the pattern is not valid UTF-8"),
        ([(COL, 0), (LIT, 0), (like, 92)], [(STRING, b"%\xc3")], "predicate op 2 (LIKE): the pattern is not valid UTF-8"),
        ([(LIT, 0), (like, 92)], s_pat, "predicate stack underflow"),
    ]
    for p, e, msg in FL.INVALID_PATTERNS:
        cases.append(([(COL, 0), (LIT, 0), (like, ord(e))], [(STRING, p.encode("utf-8"))],
                      "predicate op 2 (LIKE): the pattern '%s' is invalid, %s" % (p, msg)))
    for ops, lits, text in cases:
        assert check(lib, P.Program(ops=ops, cols=cols, lits=lits)) == (INVALID_ARG, text)
    # a NULL literal of another type is a NULL pattern
    assert check(lib, P.Program(ops=[(COL, 0), (LIT, 0), (like, 92)], cols=cols, lits=[(INT, None)])) == (0, "")


def test_negative_decimal_literals(lib):
    """Found by the sanitized fuzz: the precision test assembled the 128-bit value by shifting the signed
    high word left, undefined for a negative one. Both signs, at the bound and just inside it."""
    code = P.type_code("decimal(12,2)")
    for v, fits in ((-1235, True), (-(10 ** 12) + 1, True), (-(10 ** 12), False), (10 ** 12 - 1, True), (10 ** 12, False),
                    (-(1 << 127), False)):
        prog = P.Program(ops=[(COL, 0), (LIT, 0), (OP["<"], 0)], cols=[("m", code)], lits=[(code, P.decimal_bytes(v))])
        assert check(lib, prog) == ((0, "") if fits else (INVALID_ARG, "decimal literal 0 does not fit precision 12")), v
        if fits:
            assert plan(lib, prog)["words"] == [[i64(v), v >> 64]]
    wide = P.type_code("decimal(38,0)")
    prog = P.Program(ops=[(COL, 0), (LIT, 0), (OP["<"], 0)], cols=[("w", wide)], lits=[(wide, P.decimal_bytes(-(10 ** 38) + 1))])
    assert check(lib, prog) == (0, "")


# ---- structure ----------------------------------------------------------------------------------------
def test_structural_failures(lib):
    cols, lits = [("n", INT)], [(INT, 1)]
    cases = [
        ([(COL, 0), (99, 0)], "unknown predicate opcode 99"),
        ([(COL, 0), (-1, 0)], "unknown predicate opcode -1"),
        ([(COL, 1)], "predicate column index out of range"),
        ([(COL, -1)], "predicate column index out of range"),
        ([(LIT, 1)], "predicate literal index out of range"),
        ([(LIT, -1)], "predicate literal index out of range"),
        ([(COL, 0), (OP["="], 0)], "predicate stack underflow"),
        ([(OP["not"], 0)], "predicate stack underflow"),
        ([(COL, 0), (LIT, 0), (OP["in"], 2)], "predicate stack underflow (IN)"),
        ([(COL, 0), (LIT, 0), (OP["in"], -1)], "predicate stack underflow (IN)"),
        ([(COL, 0), (LIT, 0), (OP["in"], -2 ** 31)], "predicate stack underflow (IN)"),
        ([(COL, 0), (COL, 0)], "predicate program must leave one value"),
        ([(COL, 0), (LIT, 0), (OP["in"], 0)], "predicate program must leave one value"),
        ([], "empty predicate program"),
        # the first fault in program order is the one reported
        ([(COL, 0), (OP["="], 0), (99, 0)], "predicate stack underflow"),
        ([(COL, 0), (99, 0), (OP["="], 0)], "unknown predicate opcode 99"),
    ]
    for ops, text in cases:
        assert check(lib, P.Program(ops=ops, cols=cols, lits=lits)) == (INVALID_ARG, text), ops
    many = [("c%d" % k, INT) for k in range(PV_MAXC + 1)]
    assert check(lib, P.Program(ops=[(COL, 0), (OP["isnull"], 0)], cols=many, lits=[])) == (
        UNSUPPORTED, "at most 16 partition columns per predicate")
    assert check(lib, P.Program(ops=[(COL, 0), (OP["isnull"], 0)], cols=many[:PV_MAXC], lits=[])) == (0, "")


def test_nested_in_beyond_the_device_stack(lib):
    """`n IN (n IN (.. (1)))`: every level holds its value and its accumulator while the element runs, so
    k levels need 2k + 1 slots; 15 levels fit PV_STACK, 16 do not. Neither is a leaf program."""
    def nested(k):
        return P.Program(ops=[(COL, 0)] * k + [(LIT, 0)] + [(OP["in"], 1)] * k, cols=[("n", INT)], lits=[(INT, 1)])
    assert 2 * 15 + 1 <= PV_STACK < 2 * 16 + 1
    ok = plan(lib, nested(15))
    assert ok["leaf"] is None and len(ok["lowered"]) == 2 * (15 + 1 + 15 * 3)
    deep = plan(lib, nested(16))
    assert check(lib, nested(16)) == (0, "")
    assert deep["leaf"] is None and deep["lowered"] is None
    assert (deep["lower_status"], deep["lower_error"]) == (UNSUPPORTED, "predicate program too deep")


def test_lowered_program(lib):
    """IN lists as START / STEP / END around their elements, every other op as it is."""
    prog = P.build_program({"n": "integer", "s": "string"},
                           [("or", ("in", c("n"), [l("integer", 1), l("integer", None), l("integer", 3)]),
                             ("not", ("startswith", c("s"), l("string", "a"))))])
    low = plan(lib, prog)["lowered"]
    assert list(zip(low[0::2], low[1::2])) == [
        (COL, 0), (IN_START, 0), (LIT, 0), (IN_STEP, 0), (LIT, 1), (IN_STEP, 0), (LIT, 2), (IN_STEP, 0), (IN_END, 0),
        (COL, 1), (LIT, 3), (OP["startswith"], 0), (OP["not"], 0), (OP["or"], 0)]


# ---- the leaf plan ------------------------------------------------------------------------------------
def test_literal_first_comparisons_are_mirrored(lib):
    mirror = {"<": ">", ">": "<", "<=": ">=", ">=": "<=", "=": "=", "!=": "!=", "<=>": "<=>"}
    for op, want in mirror.items():
        leaf = plan(lib, P.build_program({"n": "integer"}, [(op, l("integer", 5), c("n"))]))["leaf"]
        assert leaf["leaves"] == [{"col": 0, "op": OP[want], "lit": 0, "nlit": 0, "lit_null": 0, "pad": 0}], op
        assert leaf["i64"] == [5] and leaf["prog"] == [LEAF, 0]
        same = plan(lib, P.build_program({"n": "integer"}, [(op, c("n"), l("integer", 5))]))["leaf"]
        assert same["leaves"][0]["op"] == OP[op], op


def test_boolean_structure_of_the_leaf_program(lib):
    prog = P.build_program({"n": "integer", "s": "string"},
                           [("or", ("not", ("isnull", c("n"))), ("and", ("=", c("s"), l("string", "x")), ("<", c("n"), l("integer", 2))))])
    leaf = plan(lib, prog)["leaf"]
    assert leaf["prog"] == [LEAF, 0, NOT, 0, LEAF, 1, LEAF, 2, AND, 0, OR, 0]
    assert [(f["col"], f["op"], f["lit"]) for f in leaf["leaves"]] == [(0, OP["isnull"], 0), (1, OP["="], 0), (0, OP["<"], 1)]
    assert leaf["i64"] == [0, 2] and leaf["str"] == [b"x".hex(), ""]
    # a comparison of two columns, or of a column with an expression, is left to the interpreter
    for e in (("=", c("n"), c("n")), ("=", ("isnull", c("n")), l("boolean", True)), ("in", c("n"), [c("n")]),
              ("isnull", ("isnull", c("n")))):
        assert plan(lib, P.build_program({"n": "integer"}, [e]))["leaf"] is None, e
    # the boolean stack of the leaf kernels is one 64-bit register of 2-bit entries: 32 deep
    def chain(k):  # l AND (l AND (.. l)): k leaves pushed before the first AND
        return P.Program(ops=[(COL, 0), (OP["isnull"], 0)] * k + [(OP["and"], 0)] * (k - 1), cols=[("n", INT)], lits=[])
    assert plan(lib, chain(32))["leaf"] is not None
    assert plan(lib, chain(33))["leaf"] is None


def test_in_sets_are_sorted_and_unique(lib):
    leaf = plan(lib, P.build_program({"n": "long"}, [("in", c("n"), [l("long", v) for v in (5, -3, 5, 2 ** 40, None, -3)])]))["leaf"]
    assert leaf["leaves"] == [{"col": 0, "op": OP["in"], "lit": 0, "nlit": 3, "lit_null": 1, "pad": 0}]
    assert leaf["i64"] == [-3, 5, 2 ** 40] and leaf["i64hi"] == [0, 0, 0]
    # double and float: by order key, -0.0 with 0.0, every NaN the canonical one above +Infinity
    nan2 = 0xfff8000000000001  # a negative, non-canonical NaN
    vals = [1.5, float("nan"), -0.0, 0.0, float("inf"), -2.0, 1.5]
    prog = P.Program(ops=[(COL, 0)] + [(LIT, k) for k in range(len(vals) + 1)] + [(OP["in"], len(vals) + 1)], cols=[("d", DOUBLE)],
                     lits=[(DOUBLE, P.double_bits(v)) for v in vals] + [(DOUBLE, nan2)])
    leaf = plan(lib, prog)["leaf"]
    want = [dkey(-2.0), 0, dkey(1.5), dkey(float("inf")), 0x7ff8000000000000]
    assert want == sorted(want) and dkey(-2.0) < 0
    assert leaf["i64"] == want and leaf["leaves"][0]["nlit"] == 5 and leaf["leaves"][0]["lit_null"] == 0
    leaf = plan(lib, P.build_program({"f": "float"}, [("in", c("f"), [l("float", v) for v in (2.5, -0.0, float("nan"), -1.0, 0.0)])]))["leaf"]
    assert leaf["i64"] == [fkey(-1.0), 0, fkey(2.5), 0x7fc00000] and leaf["leaves"][0]["pad"] == 0
    # decimals: as 128-bit values, high word signed over low word unsigned
    vals = [1 << 64, -1, 5, 1 << 64, -(1 << 64), (1 << 63), (1 << 64) - 1, None]
    leaf = plan(lib, P.build_program({"w": "decimal(38,10)"}, [("in", c("w"), [l("decimal(38,10)", v) for v in vals])]))["leaf"]
    order = sorted(set(v for v in vals if v is not None))
    assert leaf["i64"] == [i64(v) for v in order] and leaf["i64hi"] == [v >> 64 for v in order]
    assert leaf["leaves"] == [{"col": 0, "op": OP["in"], "lit": 0, "nlit": len(order), "lit_null": 1, "pad": 0}]
    # strings (and binaries): bytewise, unsigned
    vals = ["é", "z", "a", "ab", "a", "", "\x7f"]
    leaf = plan(lib, P.build_program({"s": "string"}, [("in", c("s"), [l("string", v) for v in vals])]))["leaf"]
    assert leaf["str"] == [b.hex() for b in sorted(set(v.encode("utf-8") for v in vals))]
    assert leaf["str"][-1] == "c3a9" and leaf["i64"] == [0] * 6 and leaf["leaves"][0]["nlit"] == 6
    leaf = plan(lib, P.build_program({"b": "binary"}, [("in", c("b"), [l("binary", v) for v in (b"\xff", b"\x00", b"a")])]))["leaf"]
    assert leaf["str"] == ["00", "61", "ff"]


def _in_leaf(lib, typ, vals):
    return plan(lib, P.build_program({"x": typ}, [("in", c("x"), [l(typ, v) for v in vals])]))["leaf"]


def test_integer_sets_become_bitmaps_below_a_span_of_65536(lib):
    def bitmap_of(vals):
        lo, words = min(vals), (max(vals) - min(vals)) // 64 + 1
        bits = [0] * words
        for v in vals:
            bits[(v - lo) >> 6] |= 1 << ((v - lo) & 63)
        return [lo, words] + [i64(b) for b in bits]

    for typ, vals in (("integer", [3, 70, 4, 9, 200, 64, 66, 1000, 70]), ("long", [-5, -4, 0, 1, 58, 59, 60, 122]),
                      ("timestamp", [10 ** 15 + k for k in range(8)]), ("integer", [3, 4, 5, 6, 7, 8, 9, 3 + 65535])):
        leaf = _in_leaf(lib, typ, vals)
        f = leaf["leaves"][0]
        assert (f["pad"], f["nlit"], f["lit"]) == (1, len(set(vals)), 0), (typ, vals)
        assert leaf["i64"] == bitmap_of(vals), (typ, vals)
        assert len(leaf["i64hi"]) == len(leaf["str"]) == len(leaf["i64"])
    # 7 values; a span of exactly 65,536; and float / double sets whatever their keys: sorted sets
    for typ, vals in (("integer", [1, 2, 3, 4, 5, 6, 7]), ("integer", [3, 4, 5, 6, 7, 8, 9, 3 + 65536]),
                      ("long", [-2 ** 63, 2 ** 63 - 1, 0, 1, 2, 3, 4, 5])):
        leaf = _in_leaf(lib, typ, vals)
        assert leaf["leaves"][0]["pad"] == 0 and leaf["i64"] == sorted(vals), (typ, vals)
    leaf = _in_leaf(lib, "double", [float(k) for k in range(8)])
    assert leaf["leaves"][0]["pad"] == 0 and leaf["i64"] == [dkey(float(k)) for k in range(8)]
    # the smallest subnormals: keys 1..8, a span a bitmap would take were it not floating point
    tiny = [k * 2.0 ** -149 for k in range(1, 9)]
    leaf = _in_leaf(lib, "float", tiny)
    assert leaf["leaves"][0]["pad"] == 0 and leaf["i64"] == list(range(1, 9))
    leaf = _in_leaf(lib, "double", [k * 5e-324 for k in range(1, 9)])
    assert leaf["leaves"][0]["pad"] == 0 and leaf["i64"] == list(range(1, 9))


def test_float_column_with_double_literals(lib):
    """pad == 2: the leaf widens the value's key; the DOUBLE literal's key goes in as it is, a FLOAT
    element of the same IN list widened to match."""
    leaf = plan(lib, P.build_program({"f": "float"}, [(">", c("f"), l("double", 0.1))]))["leaf"]
    assert leaf["leaves"] == [{"col": 0, "op": OP[">"], "lit": 0, "nlit": 0, "lit_null": 0, "pad": 2}]
    assert leaf["i64"] == [dkey(0.1)]
    leaf = plan(lib, P.build_program({"f": "float"}, [("<", l("float", 0.5), c("f"))]))["leaf"]
    assert leaf["leaves"][0]["pad"] == 0 and leaf["i64"] == [fkey(0.5)]
    tiny = 2.0 ** -149  # a binary32 subnormal, normal as binary64
    vals = [l("float", 1.5), l("double", 0.1), l("float", -2.5), l("float", tiny), l("float", float("nan")), l("float", -0.0)]
    leaf = plan(lib, P.build_program({"f": "float"}, [("in", c("f"), vals)]))["leaf"]
    assert leaf["leaves"] == [{"col": 0, "op": OP["in"], "lit": 0, "nlit": 6, "lit_null": 0, "pad": 2}]
    assert leaf["i64"] == sorted([dkey(1.5), dkey(0.1), dkey(-2.5), dkey(tiny), dkey(float("nan")), 0])
    leaf = plan(lib, P.build_program({"f": "float"}, [("in", c("f"), [l("float", 1.5), l("float", tiny)])]))["leaf"]
    assert leaf["leaves"][0]["pad"] == 0 and leaf["i64"] == [fkey(tiny), fkey(1.5)] and fkey(tiny) == 1
    # a DOUBLE column never widens
    leaf = plan(lib, P.build_program({"d": "double"}, [("=", c("d"), l("double", 0.1))]))["leaf"]
    assert leaf["leaves"][0]["pad"] == 0


def test_like_patterns_fold(lib, lk_lib):
    folds = [("abc", OP["="], b"abc"), ("abc%", OP["startswith"], b"abc"), ("%abc", OP["endswith"], b"abc"),
             ("%abc%", OP["contains"], b"abc"), ("%", OP["startswith"], b"")]
    for pat, op, needle in folds:
        prog = P.build_program({"s": "string"}, [("like", c("s"), l("string", pat))])
        pl = plan(lib, prog)
        assert pl["compiled"] and pl["ops"] == [[COL, 0], [LIT, 1], [op, 0]], pat
        assert pl["lit_bytes"] == [pat.encode().hex(), needle.hex()] and pl["lit_types"] == [STRING, STRING], pat
        assert pl["leaf"]["leaves"] == [{"col": 0, "op": op, "lit": 0, "nlit": 0, "lit_null": 0, "pad": 0}], pat
        assert pl["leaf"]["str"] == [needle.hex()], pat
    # anything else stays LIKE over like_lane.h's byte program, a new literal; the caller's are untouched
    prog = P.build_program({"s": "string", "n": "integer"},
                           [("and", ("=", c("n"), l("integer", 7)), ("not", ("like", c("s"), l("string", "a#_c%d_"), "#")))])
    kind, program = compile_pattern(lk_lib, b"a#_c%d_", ord("#"))
    assert kind == 4
    pl = plan(lib, prog)
    assert pl["compiled"] and pl["ops"] == [[COL, 0], [LIT, 0], [OP["="], 0], [COL, 1], [LIT, 2], [OP["like"], 0], [OP["not"], 0],
                                            [OP["and"], 0]]
    assert pl["lit_bytes"] == ["", b"a#_c%d_".hex(), program.hex()] and pl["lit_i64"] == [7, 0, 0]
    assert pl["lit_types"] == [INT, STRING, STRING] and pl["lit_null"] == [0, 0, 0]
    assert pl["leaf"]["leaves"][1] == {"col": 1, "op": OP["like"], "lit": 1, "nlit": 0, "lit_null": 0, "pad": 0}
    assert pl["leaf"]["str"] == ["", program.hex()]
    prog = P.build_program({"s": "string"}, [("like", c("s"), l("string", "a_c%d"))])
    pl = plan(lib, prog)
    assert pl["ops"][2] == [OP["like"], 0] and pl["lit_bytes"][1] == compile_pattern(lk_lib, b"a_c%d", 92)[1].hex()
    # a NULL pattern: nothing to compile, a NULL leaf
    for typ in ("string", "integer"):
        pl = plan(lib, P.build_program({"s": "string"}, [("like", c("s"), l(typ, None))]))
        assert not pl["compiled"] and pl["ops"] == [[COL, 0], [LIT, 0], [OP["like"], 92]]
        assert pl["leaf"]["leaves"] == [{"col": 0, "op": OP["like"], "lit": 0, "nlit": 0, "lit_null": 1, "pad": 0}]
        assert pl["leaf"]["i64"] == [0] and pl["leaf"]["str"] == [""]


def test_sanitized_standalone_fuzz():
    """tests/native/pred_plan_fuzz.cpp under ASan + UBSan, run directly: arbitrary programs over
    well-formed arrays, every array in a heap block of exactly its length."""
    src = os.path.join(ROOT, "tests", "native", "pred_plan_fuzz.cpp")
    exe = os.path.join(ROOT, "build", "pred_plan_fuzz")
    _build(exe, [src, DEPS[0]], DEPS[1:], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                           "-fno-omit-frame-pointer"])
    r = subprocess.run([exe, "60000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fuzz ok" in r.stdout, r.stdout + r.stderr
