"""GPU parity of the date functions of K5 (dr_filter: DR_OP_YEAR .. DR_OP_TRUNC_DATE) against the corpus
evaluator (tests/filter_dates_corpus.py, datetime.date under Spark's three-valued logic): the three
evaluators, values read from JSON commits and from the checkpoint's map column, the Snapshot layer,
and the ABI's operand, argument and literal validation."""
import ctypes as C
import os

import pytest

from tests import filter_dates_corpus as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from delta_amd.delta_log import Engine
    return Engine.get(0)


@pytest.fixture(scope="module")
def corpus_expected():
    """The corpus evaluator's selections over the table's live files, computed once."""
    files = F.live_files()
    want = [sorted(f["path"] for f in F.expected(files, p)) for p in F.PREDICATES]
    # the corpus discriminates: every function's `=` selects some files and not all
    for k in range(0, 11 * len(F.INT_FUNCS + F.DATE_FUNCS), 11):
        assert 0 < len(want[k]) < len(files), F.PREDICATES[k]
    return want


def _gpu_selected(engine, lp, preds_list):
    from delta_amd.predicates import build_program, partition_schema
    staged = engine.stage_log(lp)
    st = staged.replay(0)
    staged.release()
    try:
        live = st.export(0)
        schema = partition_schema(next(a["metaData"] for a in st.nonfile if "metaData" in a))
        out = []
        for preds in preds_list:
            sel = st.filter(build_program(schema, preds))
            assert sel == sorted(set(sel))
            out.append(sorted(live[i]["path"] for i in sel))
        return len(live), out
    finally:
        st.release()


@pytest.mark.parametrize("checkpoint", [False, True])
@pytest.mark.parametrize("filter_eval", [0, 1, 2])
def test_filter_dates_corpus(engine, tmp_path, corpus_expected, checkpoint, filter_eval):
    """Every corpus predicate under DR_OPT_FILTER_EVAL 0 (a function leaf once per dictionary code,
    k_dict_leaf), 1 (per file, k_filter_leaf_x) and 2 (the generic interpreter k_filter_typed); the
    predicates that are no leaf programs take the interpreter under all three."""
    lp = F.build(str(tmp_path), checkpoint=checkpoint)
    with engine.options(filter_eval=filter_eval):
        n, got = _gpu_selected(engine, lp, F.PREDICATES)
    assert n == F.N_LIVE
    for p, g, w in zip(F.PREDICATES, got, corpus_expected):
        assert g == w, p


def test_snapshot_layer_with_date_conjuncts(tmp_path):
    """Snapshot.list_files and files_for_scan with function conjuncts (beside a data predicate, which is
    left to the caller) return the AddFiles the corpus evaluator selects."""
    from delta_amd.delta_log import DeltaLog
    F.build(str(tmp_path))
    files = F.live_files()
    year, month = ("=", ("year", F.DT), F.INT(2024)), ("in", ("month", F.DT), [F.INT(2), F.INT(3)])
    ts = ("<", ("trunc", ("to_date", F.TS), "yyyy"), F.DATE("2021-01-01"))
    kept = F.expected(files, [year, month, ts])
    assert 0 < len(kept) < len(files)
    DeltaLog.clear_cache()
    try:
        snap = DeltaLog.for_table(str(tmp_path)).snapshot
        got = snap.files_for_scan([("and", year, ("=", F.C("id"), F.L("long", 5))), month, ts])
        assert sorted(f["path"] for f in got) == sorted(f["path"] for f in kept)
        assert all(f["partitionValues"]["dt"].strip().startswith("2024-") for f in got)
        want = {(f["size"], f["modificationTime"], os.path.join(str(tmp_path), f["path"])) for f in kept}
        groups = snap.list_files([year, month, ts])
        stats = [(s["length"], s["modificationTime"], s["path"]) for _, group in groups for s in group]
        assert len(stats) == len(want) and set(stats) == want
        for row, group in groups:  # (dt, ts, k) cast to the partition schema's types
            assert row[0].year == 2024 and row[0].month in (2, 3) and len(group) >= 1
    finally:
        DeltaLog.clear_cache()


def test_date_fn_abi_errors(engine, tmp_path):
    """dr_filter refuses on the host, before any device work: the status is DR_E_INVALID_ARG, the text of
    dr_last_error names the op or the literal, no selection comes back, and the state stays usable."""
    from delta_amd import _native as N
    from delta_amd import predicates as P
    lp = F.build(str(tmp_path))
    cols = [("dt", P.type_code("date")), ("ts", P.type_code("timestamp")), ("k", P.type_code("integer"))]
    COL, LIT, OP = P.OP_COL, P.OP_LIT, P.OP_CODE
    YEAR, MONTH, TO_DATE, DATE_ADD, TRUNC = 19, 21, 26, 27, 28
    INT, DATE, STRING = 3, 5, 0
    cases = [
        ([(COL, 2), (YEAR, 0), (LIT, 0), (OP["="], 0)], [(INT, 5)],
         "predicate op 1 (YEAR): the operand must be a DATE value, found partition column k of type 3"),
        ([(COL, 1), (MONTH, 0), (OP["isnull"], 0)], [],
         "predicate op 1 (MONTH): the operand must be a DATE value, found partition column ts of type 9"),
        ([(COL, 0), (TO_DATE, 0), (OP["isnull"], 0)], [],
         "predicate op 1 (TO_DATE): the operand must be a TIMESTAMP value, found partition column dt of type 5"),
        ([(LIT, 0), (YEAR, 0), (OP["isnull"], 0)], [(DATE, 19000)],
         "predicate op 1 (YEAR): the operand must be a DATE value, found literal 0 of type 5"),
        ([(LIT, 0), (YEAR, 0), (OP["isnull"], 0)], [(DATE, None)],
         "predicate op 1 (YEAR): the operand must be a DATE value, found a NULL literal"),
        ([(COL, 0), (YEAR, 0), (MONTH, 0), (OP["isnull"], 0)], [],
         "predicate op 2 (MONTH): the operand must be a DATE value, found the result of op 1 (opcode 19)"),
        ([(COL, 0), (TRUNC, 4), (OP["isnull"], 0)], [],
         "predicate op 1 (TRUNC_DATE): the unit (arg 4) must be 0 YEAR, 1 QUARTER, 2 MONTH or 3 WEEK"),
        ([(COL, 0), (YEAR, 2), (OP["isnull"], 0)], [], "predicate op 1 (YEAR): takes no argument (arg 2 must be 0)"),
        ([(COL, 0), (YEAR, 0), (LIT, 0), (OP["="], 0)], [(DATE, 19000)],
         "predicate literal 0 (type 5) does not fit the result of op 1 (YEAR, type 3)"),
        ([(COL, 0), (DATE_ADD, 1), (LIT, 0), (LIT, 1), (OP["in"], 2)], [(DATE, 19000), (STRING, b"2024-01-01")],
         "predicate literal 1 (type 0) does not fit the result of op 1 (DATE_ADD, type 5)"),
        ([(COL, 0), (DATE_ADD, 1), (COL, 2), (OP["="], 0)], [],
         "predicate op 3: the result of op 1 (DATE_ADD, type 5) does not compare with partition column k of type 3"),
        ([(COL, 0), (YEAR, 0), (LIT, 0), (OP["like"], 92)], [(STRING, b"20%")],
         "predicate op 3 (LIKE): the value must be a STRING partition column, found the result of op 1 (opcode 19)"),
        ([(COL, 0), (29, 0), (OP["isnull"], 0)], [], "unknown predicate opcode 29"),
        ([(COL, 0), (YEAR, 0)], [], "predicate program must leave a boolean, op 1 (YEAR) leaves a value of type 3"),
        ([(COL, 0), (MONTH, 0), (OP["not"], 0)], [],
         "predicate op 2 (NOT): the operand must be a boolean, found the result of op 1 (MONTH, type 3)"),
        # two faults: the first in program order
        ([(COL, 2), (YEAR, 0), (OP["isnull"], 0), (COL, 0), (TRUNC, 9), (OP["isnull"], 0), (OP["and"], 0)], [],
         "predicate op 1 (YEAR): the operand must be a DATE value, found partition column k of type 3"),
    ]
    staged = engine.stage_log(lp)
    st = staged.replay(0)
    staged.release()
    try:
        for ops, lits, text in cases:
            pred, keep = P.lower_program(P.Program(ops=ops, cols=cols, lits=lits))
            sel, n = C.POINTER(C.c_int64)(), C.c_int64(-1)
            with engine.lock:
                rc = engine.lib.dr_filter(st.h, C.byref(pred), C.byref(sel), C.byref(n))
                msg = engine.lib.dr_last_error(engine.ctx).decode("utf-8")
            assert (N.STATUS[rc], msg) == ("DR_E_INVALID_ARG", text), ops
            assert not sel and n.value == 0, ops  # no selection: a NULL pointer and no rows
        live = st.export(0)
        sel = st.filter(P.Program(ops=[(COL, 0), (YEAR, 0), (LIT, 0), (OP["="], 0)], cols=cols, lits=[(INT, 2024)]))
        want = [f["path"] for f in F.expected(F.live_files(), [("=", ("year", F.DT), F.INT(2024))])]
        assert sorted(live[i]["path"] for i in sel) == sorted(want) and want
    finally:
        st.release()
