"""The K5 predicate planner (delta_amd/csrc/pred_plan.cpp) over predicate columns with a source
(DR_SRC_* in bits 24..27 of the type), as a stand-alone program under ASan + UBSan: every refusal of a
statistics column with its status and full text, the first fault in program order, a program mixing
sources leafified, and `nullCount < numRecords` lowered but not leafified."""
import os
import subprocess

import pytest

from delta_amd import predicates as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = [os.path.join(ROOT, "tests", "native", "pred_plan_stats_host.cpp"), os.path.join(ROOT, "delta_amd", "csrc", "pred_plan.cpp")]
INVALID_ARG, UNSUPPORTED = 1, 12
OP = P.OP_CODE
COL, LIT = P.OP_COL, P.OP_LIT
STRING, INT, LONG, DATE, BOOLEAN, DOUBLE, TIMESTAMP, BINARY = 0, 3, 4, 5, 6, 8, 9, 10
DEC = 11 | 12 << 8 | 2 << 16
src = lambda s, t: t | s << 24  # noqa: E731
ISNULL = [(COL, 0), (OP["isnull"], 0)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pps") / "pred_plan_stats_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", out] + SRCS)
    return out


def run(exe, cases):
    """cases: (cols [(name, type)], ops [(opcode, arg)], lits [(type, i64)]) -> (status, text, leaf, lowered)."""
    lines = []
    for cols, ops, lits in cases:
        tok = [str(len(cols))] + [x for n, t in cols for x in (str(t), n.encode("utf-8").hex() or "-")]
        tok += [str(len(ops))] + [str(x) for o in ops for x in o] + [str(len(lits))] + [str(x) for l in lits for x in l]
        lines.append(" ".join(tok))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe], input=("\n".join(lines) + "\n").encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    assert r.returncode == 0, r.stderr.decode("utf-8", "replace")[-3000:]
    out = []
    for line in r.stdout.decode("utf-8").splitlines():
        status, text, leaf, low = line.split("|")
        out.append((int(status), text, tuple(int(x) for x in leaf.split()) if leaf else None, int(low) if low else None))
    assert len(out) == len(cases)
    return out


def test_refusals_with_status_and_text(exe):
    cases = [
        ([("x", src(1, BOOLEAN))], "predicate column 0: minValues statistics have no BOOLEAN (type 6)"),
        ([("x", src(2, BOOLEAN))], "predicate column 0: maxValues statistics have no BOOLEAN (type 6)"),
        ([("x", src(1, BINARY))], "predicate column 0: minValues statistics have no BINARY (type 10)"),
        ([("x", src(2, BINARY))], "predicate column 0: maxValues statistics have no BINARY (type 10)"),
        ([("x", src(3, INT))], "predicate column 0: nullCount is a LONG, not type 3"),
        ([("x", src(3, DEC))], "predicate column 0: nullCount is a LONG, not type %d" % DEC),
        ([("", src(4, STRING))], "predicate column 0: numRecords is a LONG, not type 0"),
        ([("x", src(5, LONG))], "predicate column 0: unknown source 5 (DR_SRC_PARTITION .. DR_SRC_STATS_NUMRECORDS)"),
        ([("x", src(15, LONG))], "predicate column 0: unknown source 15 (DR_SRC_PARTITION .. DR_SRC_STATS_NUMRECORDS)"),
        ([("ab", src(4, LONG))], 'predicate column 0: numRecords takes the name "", not a path of 2 bytes'),
        ([("", src(1, LONG))], "predicate column 0: segment 0 of the statistics path is empty"),
        ([("a\x01", src(2, LONG))], "predicate column 0: segment 1 of the statistics path is empty"),
        ([("\x01a", src(3, LONG))], "predicate column 0: segment 0 of the statistics path is empty"),
        ([("a\x01\x01b", src(1, LONG))], "predicate column 0: segment 1 of the statistics path is empty"),
        ([("\x01".join("abcdefghi"), src(1, LONG))], "predicate column 0: a statistics path has at most 8 segments, not 9"),
        ([("y" * 256, src(2, STRING))], "predicate column 0: a statistics path has at most 255 bytes, not 256"),
        # the column index is the faulty column's
        ([("p", INT), ("ok", src(1, LONG)), ("x", src(3, INT))], "predicate column 2: nullCount is a LONG, not type 3"),
    ]
    got = run(exe, [(cols, ISNULL, []) for cols, _ in cases])
    for (cols, text), g in zip(cases, got):
        assert g[:2] == (INVALID_ARG, text), cols
    # what is not refused: every type a min or max takes, the limits themselves, a partition column named alike
    fine = [[("x", src(s, t))] for s in (1, 2) for t in (STRING, 1, 2, INT, LONG, DATE, 7, DOUBLE, TIMESTAMP, DEC)]
    fine += [[("x", src(3, LONG))], [("", src(4, LONG))], [("\x01".join("abcdefgh"), src(1, LONG))], [("y" * 255, src(2, STRING))],
             [("", INT)], [("a\x01\x01b", BOOLEAN)]]
    for cols, g in zip(fine, run(exe, [(cols, ISNULL, []) for cols in fine])):
        assert g[:2] == (0, ""), cols
    # a type that is none, with a source or without: the older refusal, as before
    for g in run(exe, [([("x", src(1, 12))], ISNULL, []), ([("x", 12)], ISNULL, []), ([("x", -1)], ISNULL, [])]):
        assert g[:2] == (UNSUPPORTED, "unsupported partition column type")


def test_first_fault_in_program_order(exe):
    two_bad = [("a", src(1, BOOLEAN)), ("b", src(5, LONG))]
    bad_op = [(COL, 0), (99, 0)]
    got = run(exe, [
        (two_bad, ISNULL, []),                                   # the first faulty column
        (list(reversed(two_bad)), ISNULL, []),
        ([("a", src(1, BOOLEAN))], bad_op, []),                  # a column's fault before any op's
        ([("a", src(1, LONG))], bad_op, []),
        # pattern ops and date functions keep their own operand rules, which look at the base type only
        ([("s", src(1, STRING))], [(COL, 0), (LIT, 0), (OP["startswith"], 0)], [(STRING, 0)]),
        ([("n", src(2, LONG))], [(COL, 0), (LIT, 0), (OP["startswith"], 0)], [(STRING, 0)]),
        ([("d", src(1, DATE))], [(COL, 0), (19, 0), (LIT, 0), (OP["="], 0)], [(INT, 2020)]),
        ([("t", src(2, TIMESTAMP))], [(COL, 0), (19, 0), (LIT, 0), (OP["="], 0)], [(INT, 2020)]),
    ])
    assert got[0][:2] == (INVALID_ARG, "predicate column 0: minValues statistics have no BOOLEAN (type 6)")
    assert got[1][:2] == (INVALID_ARG, "predicate column 0: unknown source 5 (DR_SRC_PARTITION .. DR_SRC_STATS_NUMRECORDS)")
    assert got[2][:2] == (INVALID_ARG, "predicate column 0: minValues statistics have no BOOLEAN (type 6)")
    assert got[3][:2] == (INVALID_ARG, "unknown predicate opcode 99")
    assert got[4][:2] == (0, "") and got[6][:2] == (0, "")
    assert got[5][:2] == (INVALID_ARG, "predicate op 2 (STARTSWITH): the value must be a STRING partition column, found statistics column n of type 4")
    assert got[7][:2] == (INVALID_ARG, "predicate op 1 (YEAR): the operand must be a DATE value, found statistics column t of type 9")


def test_leaf_and_generic_plans(exe):
    mixed_cols = [("p", INT), ("id", src(1, LONG)), ("id", src(2, LONG)), ("d", src(2, DOUBLE))]
    # p = 1 AND (min(id) <= 5 AND max(id) >= 5 OR min(id) IS NULL) AND max(d) > 1.5
    mixed = [(COL, 0), (LIT, 0), (OP["="], 0), (COL, 1), (LIT, 1), (OP["<="], 0), (COL, 2), (LIT, 1), (OP[">="], 0), (OP["and"], 0),
             (COL, 1), (OP["isnull"], 0), (OP["or"], 0), (OP["and"], 0), (COL, 3), (LIT, 2), (OP[">"], 0), (OP["and"], 0)]
    counts = [("id", src(3, LONG)), ("", src(4, LONG))]
    lt = [(COL, 0), (COL, 1), (OP["<"], 0)]
    got = run(exe, [(mixed_cols, mixed, [(INT, 1), (LONG, 5), (DOUBLE, P.double_bits(1.5))]), (counts, lt, []),
                    (counts, [(COL, 0), (LIT, 0), (OP[">"], 0)], [(LONG, 0)])])
    assert got[0] == (0, "", (1, 5, 9), len(mixed))   # a leaf program: five leaves, four combining ops
    assert got[1] == (0, "", (0, 0, 0), 3)            # col op col: lowered for the interpreter, no leaf form
    assert got[2] == (0, "", (1, 1, 1), 3)
