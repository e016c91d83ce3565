"""dr_state_aggregate's host side without a device: the spec and selection checks of
delta_amd/csrc/pred_plan.cpp as a stand-alone program under ASan + UBSan -- every refusal with its status
and full text, the accepted specs, check_column_source's texts unchanged for a predicate column -- and
the proof rules of Snapshot.aggregate_from_metadata (delta_amd/aggregates.py) on hand-made results."""
import os
import re
import subprocess

import numpy as np
import pytest

from delta_amd import _native as N
from delta_amd import aggregates as A
from tests import filter_stats_corpus as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = [os.path.join(ROOT, "tests", "native", "agg_plan_host.cpp"), os.path.join(ROOT, "delta_amd", "csrc", "pred_plan.cpp")]
INVALID_ARG = 1
STRING, BYTE, INT, LONG, DATE, BOOLEAN, FLOAT, DOUBLE, TIMESTAMP, BINARY = 0, 1, 3, 4, 5, 6, 7, 8, 9, 10
DEC = 11 | 12 << 8 | 2 << 16
COUNT, MIN, MAX, SUM = N.DR_AGG_COUNT, N.DR_AGG_MIN, N.DR_AGG_MAX, N.DR_AGG_SUM
COLUMN, SIZE, MTIME = N.DR_AGG_IN_COLUMN, N.DR_AGG_IN_SIZE, N.DR_AGG_IN_MTIME
src = lambda s, t: t | s << 24  # noqa: E731


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("aggplan") / "agg_plan_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", out] + SRCS)
    return out


def run(exe, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe], input=("\n".join(lines) + "\n").encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    assert r.returncode == 0, r.stderr.decode("utf-8", "replace")[-3000:]
    out = [(int(l.split("|", 1)[0]), l.split("|", 1)[1]) for l in r.stdout.decode("utf-8").splitlines()]
    assert len(out) == len(lines)
    return out


def _hex(name):
    return "0" if name is None else (name.encode("utf-8").hex() or "-")


def specs(*aggs, naggs=None):
    """aggs: (fn, input, type, name)."""
    return "S %d " % (len(aggs) if naggs is None else naggs) + " ".join("%d %d %d %s" % (f, i, t, _hex(n)) for f, i, t, n in aggs)


def selection(side, rows, off, nrows=None, ngroups=None):
    r = [] if rows is None else list(rows)
    line = "R %d %d %d %s" % (side, rows is not None, len(r) if nrows is None else nrows, " ".join(map(str, r)))
    o = [0] if off is None else list(off)
    return line + " %d %d %s" % (off is not None, (len(o) - 1) if ngroups is None else ngroups, " ".join(map(str, o)))


def test_binding_names_the_kernels_tile():
    with open(os.path.join(ROOT, "delta_amd", "csrc", "kernels.h")) as f:
        m = re.search(r"constexpr uint32_t AGG_TILE = (\d+);", f.read())
    assert m and int(m.group(1)) == N.AGG_TILE
    assert N.DR_AGG_MAX_SPECS == 16 and set(("dr_state_aggregate", "dr_agg_release")) <= set(N.OPTIONAL_SYMBOLS)


def test_spec_refusals_with_status_and_text(exe):
    ok = (COUNT, SIZE, 0, "")
    cases = [
        ("S -1", "dr_state_aggregate: naggs = -1 is outside 0..16"),
        (specs(*[ok] * 17), "dr_state_aggregate: naggs = 17 is outside 0..16"),
        ("S 2 null", "dr_state_aggregate: aggs == NULL with naggs = 2"),
        (specs((4, SIZE, 0, "")), "aggregate spec 0: unknown fn 4 (DR_AGG_COUNT .. DR_AGG_SUM)"),
        (specs(ok, (-1, COLUMN, LONG, "p")), "aggregate spec 1: unknown fn -1 (DR_AGG_COUNT .. DR_AGG_SUM)"),
        (specs((SUM, 3, 0, "")), "aggregate spec 0: unknown input 3 (DR_AGG_IN_COLUMN .. DR_AGG_IN_MTIME)"),
        (specs((SUM, -2, 0, "")), "aggregate spec 0: unknown input -2 (DR_AGG_IN_COLUMN .. DR_AGG_IN_MTIME)"),
        (specs(ok, ok, (SUM, SIZE, 0, "size")), 'aggregate spec 2: DR_AGG_IN_SIZE takes the name "" and the type 0'),
        (specs((MAX, MTIME, LONG, "")), 'aggregate spec 0: DR_AGG_IN_MTIME takes the name "" and the type 0'),
        (specs((MAX, COLUMN, LONG, None)), "aggregate spec 0: a column input needs a name"),
        (specs((MAX, COLUMN, 12, "p")), "aggregate spec 0: no valid column type (code 12)"),
        (specs((MAX, COLUMN, -5, "p")), "aggregate spec 0: no valid column type (code -5)"),
        (specs((MAX, COLUMN, 11 | 39 << 8, "p")), "aggregate spec 0: no valid column type (code %d)" % (11 | 39 << 8)),
        (specs((MAX, COLUMN, src(1, 12), "x")), "aggregate spec 0: no valid column type (code %d)" % src(1, 12)),
        # everything check_column_source refuses, with its texts and the spec index in the column's place
        (specs((MIN, COLUMN, src(1, BOOLEAN), "x")), "predicate column 0: minValues statistics have no BOOLEAN (type 6)"),
        (specs(ok, (MAX, COLUMN, src(2, BINARY), "x")), "predicate column 1: maxValues statistics have no BINARY (type 10)"),
        (specs((SUM, COLUMN, src(3, INT), "x")), "predicate column 0: nullCount is a LONG, not type 3"),
        (specs((SUM, COLUMN, src(4, STRING), "")), "predicate column 0: numRecords is a LONG, not type 0"),
        (specs(ok, ok, ok, (COUNT, COLUMN, src(5, LONG), "x")), "predicate column 3: unknown source 5 (DR_SRC_PARTITION .. DR_SRC_STATS_NUMRECORDS)"),
        (specs((COUNT, COLUMN, src(15, LONG), "x")), "predicate column 0: unknown source 15 (DR_SRC_PARTITION .. DR_SRC_STATS_NUMRECORDS)"),
        (specs((SUM, COLUMN, src(4, LONG), "ab")), 'predicate column 0: numRecords takes the name "", not a path of 2 bytes'),
        (specs((MIN, COLUMN, src(1, LONG), "")), "predicate column 0: segment 0 of the statistics path is empty"),
        (specs((MIN, COLUMN, src(1, LONG), "a\x01\x01b")), "predicate column 0: segment 1 of the statistics path is empty"),
        (specs((MIN, COLUMN, src(1, LONG), "\x01".join("abcdefghi"))), "predicate column 0: a statistics path has at most 8 segments, not 9"),
        (specs((MAX, COLUMN, src(2, STRING), "y" * 256)), "predicate column 0: a statistics path has at most 255 bytes, not 256"),
        # SUM outside BYTE .. LONG
        (specs((SUM, COLUMN, STRING, "p")), "aggregate spec 0: SUM takes BYTE .. LONG, size and modificationTime, not type 0"),
        (specs((SUM, COLUMN, DATE, "p")), "aggregate spec 0: SUM takes BYTE .. LONG, size and modificationTime, not type 5"),
        (specs((SUM, COLUMN, src(1, DOUBLE), "d")), "aggregate spec 0: SUM takes BYTE .. LONG, size and modificationTime, not type 8"),
        (specs(ok, (SUM, COLUMN, src(2, DEC), "dec")), "aggregate spec 1: SUM takes BYTE .. LONG, size and modificationTime, not type %d" % DEC),
        (specs((SUM, COLUMN, src(1, TIMESTAMP), "ts")), "aggregate spec 0: SUM takes BYTE .. LONG, size and modificationTime, not type 9"),
        # the first offending spec is the one named
        (specs((SUM, COLUMN, BOOLEAN, "p"), (9, SIZE, 0, "")), "aggregate spec 0: SUM takes BYTE .. LONG, size and modificationTime, not type 6"),
    ]
    for (line, text), got in zip(cases, run(exe, [c[0] for c in cases])):
        assert got == (INVALID_ARG, text), line


def test_accepted_specs(exe):
    fine = ["S 0", "S 0 null", specs(*[(COUNT, SIZE, 0, "")] * 16), specs((SUM, SIZE, 0, ""), (SUM, MTIME, 0, ""), (MIN, MTIME, 0, None))]
    every = (STRING, BYTE, 2, INT, LONG, DATE, BOOLEAN, FLOAT, DOUBLE, TIMESTAMP, BINARY, DEC)
    fine += [specs((f, COLUMN, t, "p")) for f in (COUNT, MIN, MAX) for t in every]
    fine += [specs((f, COLUMN, src(s, t), "x")) for f in (COUNT, MIN, MAX) for s in (1, 2) for t in every if t not in (BOOLEAN, BINARY)]
    fine += [specs((f, COLUMN, src(3, LONG), "a\x01b"), (f, COLUMN, src(4, LONG), "")) for f in (COUNT, MIN, MAX, SUM)]
    fine += [specs((SUM, COLUMN, src(s, t), "x")) for s in (0, 1, 2) for t in (BYTE, 2, INT, LONG)]
    for line, got in zip(fine, run(exe, fine)):
        assert got == (0, ""), line


def test_selection_refusals_and_accepted_selections(exe):
    cases = [
        (selection(10, [], None, nrows=-1), "dr_state_aggregate: nrows = -1 is negative"),
        (selection(10, None, [0], ngroups=-3), "dr_state_aggregate: ngroups = -3 is negative"),
        (selection(10, [0, 9, 10], None), "dr_state_aggregate: rows[2] = 10 is outside [0, 10)"),
        (selection(10, [3, -1, 11], None), "dr_state_aggregate: rows[1] = -1 is outside [0, 10)"),
        (selection(0, [0], None), "dr_state_aggregate: rows[0] = 0 is outside [0, 0)"),
        (selection(10, [1, 2, 3], [1, 3]), "dr_state_aggregate: group_off[0] = 1, not 0"),
        (selection(10, [1, 2, 3], [0, 2, 1, 3]), "dr_state_aggregate: group_off[2] = 1 is below group_off[1] = 2"),
        (selection(10, [1, 2, 3], [0, 2]), "dr_state_aggregate: group_off[1] = 2, not the selection's 3 rows"),
        (selection(10, [1, 2, 3], [0, 2, 4]), "dr_state_aggregate: group_off[2] = 4, not the selection's 3 rows"),
        (selection(10, None, [0, 9]), "dr_state_aggregate: group_off[1] = 9, not the selection's 10 rows"),
        (selection(10, [1], [0], ngroups=0), "dr_state_aggregate: group_off[0] = 0, not the selection's 1 rows"),
        # a row is named before a group offset
        (selection(10, [1, 12], [5, 2]), "dr_state_aggregate: rows[1] = 12 is outside [0, 10)"),
    ]
    for (line, text), got in zip(cases, run(exe, [c[0] for c in cases])):
        assert got == (INVALID_ARG, text), line
    fine = [selection(10, None, None), selection(0, None, None), selection(0, [], [0], ngroups=0), selection(10, [], [0, 0, 0]),
            selection(10, [9, 0, 9, 9], [0, 0, 1, 1, 4, 4]), selection(10, None, [0, 10]), selection(10, None, [0, 0, 10, 10]),
            selection(3, [2, 1, 0], [0, 1, 2, 3]), selection(10, None, None, nrows=-7), selection(10, [4], None, ngroups=-7)]
    for line, got in zip(fine, run(exe, fine)):
        assert got == (0, ""), line


def test_check_column_source_texts_are_unchanged(exe):
    """A predicate column still meets the texts tests/test_pred_plan_stats.py pins, a source above 4 included."""
    cases = [
        ("C %d %s 0" % (src(1, BOOLEAN), _hex("x")), "predicate column 0: minValues statistics have no BOOLEAN (type 6)"),
        ("C %d %s 2" % (src(3, INT), _hex("x")), "predicate column 2: nullCount is a LONG, not type 3"),
        ("C %d %s 0" % (src(5, LONG), _hex("x")), "predicate column 0: unknown source 5 (DR_SRC_PARTITION .. DR_SRC_STATS_NUMRECORDS)"),
        ("C %d %s 1" % (src(4, LONG), _hex("ab")), 'predicate column 1: numRecords takes the name "", not a path of 2 bytes'),
        ("C %d %s 0" % (src(2, LONG), _hex("a\x01")), "predicate column 0: segment 1 of the statistics path is empty"),
    ]
    for (line, text), got in zip(cases, run(exe, [c[0] for c in cases])):
        assert got == (INVALID_ARG, text), line
    fine = ["C %d %s 0" % (INT, _hex("")), "C %d %s 0" % (src(4, LONG), "-"), "C %d %s 0" % (src(1, DEC), _hex("a\x01b"))]
    assert run(exe, fine) == [(0, "")] * 3


# ---- the proof rules, on hand-made aggregate results ------------------------------------------------------
def result(group_rows, cells):
    """A State.aggregate result from per-spec lists of (nonnull, lo, hi, string) per group."""
    ng, na = len(group_rows), len(cells)
    r = {"group_rows": np.array(group_rows, dtype=np.int64), "strings": [[c[3] for c in row] for row in cells]}
    for k, name in enumerate(("nonnull", "value_lo", "value_hi")):
        r[name] = np.array([[c[k] for c in row] for row in cells], dtype=np.int64).reshape(na, ng)
    r["arg_row"] = np.full((na, ng), -1, dtype=np.int64)
    return r


def test_plan_resolves_names_and_shares_specs():
    P = A.plan([("count",), ("count", "ID"), ("min", "id"), ("max", "`id`"), ("min", "P"), ("max", "n.y.z"), ("min", "ts"), ("count", "p"),
                ("max", "nosuch"), ("min", "dt")], F.METADATA)
    nrec = ("sum", N.DR_SRC_STATS_NUMRECORDS, (), "long")
    assert P.specs == [nrec, ("sum", N.DR_SRC_STATS_NULLCOUNT, ("id",), "long"), ("min", N.DR_SRC_STATS_MIN, ("id",), "long"),
                       ("max", N.DR_SRC_STATS_MAX, ("id",), "long"), ("min", N.DR_SRC_PARTITION, "p", "integer"),
                       ("count", N.DR_SRC_PARTITION, "p", "integer"), ("min", N.DR_SRC_STATS_MIN, ("dt",), "date")]
    assert [it[0] for it in P.items] == ["count_star", "count_data", "minmax_data", "minmax_data", "minmax_part", "unproven", "unproven",
                                         "count_part", "unproven", "minmax_data"]
    assert P.allnull == [(2, ("id",)), (3, ("id",)), (6, ("dt",))]
    # a data filter: counts and data columns are not proven, partition min / max still are
    Q = A.plan([("count",), ("count", "id"), ("min", "id"), ("max", "p"), ("count", "p")], F.METADATA, data_filter=True)
    assert [it[0] for it in Q.items] == ["unproven", "unproven", "unproven", "minmax_part", "unproven"]
    assert Q.specs == [("max", N.DR_SRC_PARTITION, "p", "integer")]
    for bad in [("sum", "id"), ("min",), "count", ("count", "a", "b"), ("min", 5)]:
        with pytest.raises(Exception):
            A.plan([bad], F.METADATA)


def test_proof_rules_each_way():
    P = A.plan([("count",), ("count", "id"), ("min", "id"), ("max", "p"), ("count", "p"), ("max", "s")], F.METADATA)
    assert len(P.specs) == 5  # numRecords, nullCount.id, min(minValues.id), max(p), count(p)
    # group 0: everything present; group 1: one file of 4 lacks numRecords, one lacks nullCount and the statistic;
    # group 2: empty; group 3: the statistic is missing on 2 files, both proven all-NULL; group 4: the sums overflow
    big = 2 ** 63 - 1
    res = result([3, 4, 0, 5, 2], [
        [(3, 30, 0, None), (3, 40, 0, None), (0, 0, 0, None), (5, 50, 0, None), (2, -2, 0, None)],        # sum(numRecords): 2 * big = -2, hi 0
        [(3, 4, 0, None), (3, 1, 0, None), (0, 0, 0, None), (5, 20, 0, None), (2, 0, 0, None)],           # sum(nullCount.id)
        [(3, -7, -1, None), (3, 5, 0, None), (0, 0, 0, None), (3, 11, 0, None), (2, 1, 0, None)],         # min(minValues.id)
        [(3, 4, 0, None), (4, 2, 0, None), (0, 0, 0, None), (0, 0, 0, None), (2, 1, 0, None)],            # max(p)
        [(3, 0, 0, None), (4, 0, 0, None), (0, 0, 0, None), (0, 0, 0, None), (1, 0, 0, None)],            # count(p)
    ])
    got = A.prove(P, res, {2: [0, 0, 0, 2, 0]})
    assert got[0] == [30, 26, -7, 4, 30, None]
    assert got[1] == [None, None, None, 2, None, None]   # numRecords missing: no count; the statistic missing, not proven all-NULL
    assert got[2] == [0, 0, None, None, 0, None]         # no files: counts are 0, min / max NULL
    assert got[3] == [50, 30, 11, None, 0, None]         # 3 with the statistic + 2 all-NULL = 5 files; p NULL everywhere: count(p) = 0
    assert got[4] == [None, None, 1, 1, None, None]      # an overflowed sum proves nothing; p NULL in one of two files
    assert big + big - 2 ** 64 == -2
    # without the all-NULL counts group 3's min is not proven
    assert A.prove(P, res)[3][2] is None
    # nullCount above numRecords is no count
    res["value_lo"][1][0] = 31
    assert A.prove(P, res, {2: [0, 0, 0, 2, 0]})[0][1] is None


def test_decode_by_type():
    import decimal
    assert A.decode("long", -5, -1, None) == -5 and A.decode("date", 18628, 0, None) == 18628
    assert A.decode("boolean", 1, 0, None) is True
    assert A.decode("double", -2 ** 63, 0, None) == 0.0 and str(A.decode("double", -2 ** 63, 0, None)) == "-0.0"
    assert A.decode("float", 0x3fc00000, 0, None) == 1.5
    assert A.decode("decimal(12,2)", -12345, -1, None) == decimal.Decimal("-123.45")
    assert A.decode("decimal(38,0)", 1, 1, None) == decimal.Decimal(2 ** 64 + 1)
    assert A.decode("string", 0, 0, "café".encode()) == "café" and A.decode("binary", 0, 0, b"\xff") == b"\xff"
