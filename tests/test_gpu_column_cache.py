"""The typed column cache of a state (dr_state::pv_cols) as its six consumers share it: dr_filter,
dr_state_aggregate, dr_state_stats_column, dr_state_probe_keys, dr_state_partition_groups and
dr_state_write_checkpoint ask one function for their columns, so a column built for one call serves the
next whatever the order, a repeated key is built once, the rerun of either extract kernel (escaped
strings, floating-point values for the host) still happens, a state without live files builds nothing,
and a failed timed call leaves neither its launch hook nor its event marks behind.

Cache activity is read from the per-launch timings (Engine.set_timing / last_timings): a build shows as
k_pv_extract or k_stats_extract, its second pass as the same name with "#2". The table is the statistics
corpus (tests/filter_stats_corpus.py) with its checkpoint: 399 live files, 199 of them checkpoint rows."""
import json
import os

import numpy as np
import pytest

from delta_amd import _native as N
from tests import filter_stats_corpus as F
from tests import filter_types_corpus as T

pytestmark = pytest.mark.gpu
INVALID_ARG = 1  # enum dr_status
ID_MIN, ID_MAX = (F.MIN, ("id",), "long"), (F.MAX, ("id",), "long")
KEYS = [12, 1000, 65536, -5000, 7, 1000]


@pytest.fixture(scope="module")
def engine():
    from delta_amd.delta_log import Engine
    return Engine.get(0)


@pytest.fixture(scope="module")
def log_path(tmp_path_factory):
    return F.build(str(tmp_path_factory.mktemp("column_cache")), checkpoint=True)


def _replay(engine, lp):
    staged = engine.stage_log(lp)
    try:
        return staged.replay(0)
    finally:
        staged.release()


def _program():
    """p = 1 AND minValues.id >= 1000: the columns (p, integer) and (MIN id, long)."""
    from delta_amd.predicates import build_program
    return build_program({"p": "integer"}, [("=", F.C("p"), F.L("integer", 1)), (">=", F.ID_MIN, F.L("long", 1000))])


# the consumers in the order of the shared-state test, and the extract launches each reports there: the
# integer, long and digit-string values of these columns need no second pass
CALLS = [
    ("filter", lambda st: st.filter(_program()), {"k_pv_extract", "k_stats_extract"}),
    ("aggregate", lambda st: st.aggregate([("min", N.DR_SRC_PARTITION, "p", "integer"), ("max",) + ID_MIN]), set()),
    ("stats_column", lambda st: st.stats_column(*ID_MIN), set()),
    ("probe_keys", lambda st: st.probe_keys(ID_MIN, ID_MAX, KEYS), {"k_stats_extract"}),  # only MAX id is new
    ("partition_groups", lambda st: st.partition_groups(), {"k_pv_extract"}),  # (p, STRING) is another key
    ("partition_groups again", lambda st: st.partition_groups(), set()),
]


def _timed(engine, call):
    """(the call's result, its timings)."""
    engine.set_timing(True)
    try:
        res = call()
        return res, engine.last_timings()
    finally:
        engine.set_timing(False)


def _extracts(timings):
    return {k for k in timings if k.startswith(("k_pv_extract", "k_stats_extract"))}


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    return a == b


@pytest.fixture(scope="module")
def fresh(engine, log_path):
    """Every call's result on a state of its own, computed once."""
    out = {}
    for name, call, _ in CALLS:
        st = _replay(engine, log_path)
        try:
            out[name] = call(st)
        finally:
            st.release()
    assert 0 < len(out["filter"]) < F.N_LIVE and len(out["partition_groups"]) == 5
    assert len(out["stats_column"][0]) == F.N_LIVE and 0 < len(out["probe_keys"]["selected"]) < F.N_LIVE
    return out


def test_columns_are_shared_across_entry_points(engine, log_path, fresh):
    """One state through every consumer: each builds only the keys no earlier call has built, and answers
    what it answers on a state of its own."""
    st = _replay(engine, log_path)
    try:
        for name, call, built in CALLS:
            res, t = _timed(engine, lambda: call(st))
            assert _extracts(t) == built, (name, sorted(t))
            assert _same(res, fresh[name]), name
    finally:
        st.release()


def test_order_of_the_calls_does_not_matter(engine, log_path, fresh):
    st = _replay(engine, log_path)
    try:
        for name, call, _ in reversed(CALLS):
            assert _same(call(st), fresh[name]), name
    finally:
        st.release()


def test_a_repeated_key_is_built_once(engine, log_path):
    """MIN and MAX over one statistics column: one key twice in the request, one k_stats_extract launch (a
    LONG column needs no second pass)."""
    st = _replay(engine, log_path)
    try:
        res, t = _timed(engine, lambda: st.aggregate([("min",) + ID_MIN, ("max",) + ID_MIN]))
        assert _extracts(t) == {"k_stats_extract"}, sorted(t)
        vals, nulls = st.stats_column(*ID_MIN)
        known = vals[nulls == 0]
        assert res["nonnull"].tolist() == [[len(known)], [len(known)]]
        assert res["value_lo"].tolist() == [[int(known.min())], [int(known.max())]]
    finally:
        st.release()


def test_partition_value_build_reruns(engine, tmp_path):
    """The types corpus read from JSON: its text column `b` (BINARY: the STRING buffers and the same
    unescaping) has values written with \\u escapes, which take the arena, and its DOUBLE column `d` a value
    of 27 digits, which takes the host's strtod: k_pv_extract runs twice, and the filter selects what the
    corpus's evaluation selects."""
    from delta_amd.predicates import build_program
    from oracle import delta_oracle as O
    lp = T.build(str(tmp_path))
    with open(os.path.join(lp, "%020d.json" % 0)) as f:
        assert any('"b":"\\u00e9"' in line for line in f)  # the corpus writes some lines with ensure_ascii
    preds = [(">=", T.C("b"), T.BIN("é".encode("utf-8"))), (">", T.C("d"), T.DBL(3.14)), ("<", T.C("d"), T.DBL(3.15))]
    snap = O.state_reconstruction(O.get_log_segment(lp), 0)
    schema = O.partition_schema(snap.metadata)
    want = sorted(f["path"] for f in T.expected(schema, snap.all_files, preds))
    assert 0 < len(want) < T.N_LIVE
    st = _replay(engine, lp)
    try:
        sel, t = _timed(engine, lambda: st.filter(build_program(schema, preds)))
        assert _extracts(t) == {"k_pv_extract", "k_pv_extract#2"}, sorted(t)
        live = st.export(0)
        assert sorted(live[i]["path"] for i in sel) == want
    finally:
        st.release()


def test_statistics_build_reruns(engine, log_path):
    """minValues.s of the statistics corpus holds escaped strings (`}{\\"}{`, `back\\\\slash`): k_stats_extract
    runs twice, and s = '}{"}{' (rewritten over MIN s and MAX s) selects what the corpus's evaluator keeps."""
    from delta_amd import skipping as K
    from delta_amd.predicates import build_program
    pred = [K.rewrite(("=", F.C("s"), F.L("string", '}{"}{')), K.data_schema(F.METADATA), ["p"])]
    want = sorted(f["path"] for f in F.expected(F.live_files(), pred))
    assert 0 < len(want) < F.N_LIVE
    st = _replay(engine, log_path)
    try:
        sel, t = _timed(engine, lambda: st.filter(build_program({"p": "integer"}, pred)))
        assert _extracts(t) == {"k_stats_extract", "k_stats_extract#2"}, sorted(t)
        live = st.export(0)
        assert sorted(live[i]["path"] for i in sel) == want
    finally:
        st.release()


def test_a_state_without_live_files_builds_nothing(engine, tmp_path):
    """The table's only commit removes its one file: every consumer succeeds with an empty or zero result, and
    no call's timings name an extract kernel."""
    log = os.path.join(str(tmp_path), "_delta_log")
    os.makedirs(log)
    with open(os.path.join(log, "%020d.json" % 0), "w") as f:
        for a in ({"protocol": F.PROTOCOL}, {"metaData": F.METADATA},
                  {"remove": {"path": "f-00000.parquet", "deletionTimestamp": 1600000001000, "dataChange": True}}):
            f.write(json.dumps(a, separators=(",", ":")) + "\n")
    st = _replay(engine, log)
    try:
        assert st.counts["num_files"] == 0
        # write_checkpoint_part comes last: the calls before it that return early collect no timings of their own
        calls = [lambda: st.filter(_program()),
                 lambda: st.aggregate([("min", N.DR_SRC_PARTITION, "p", "integer"), ("max",) + ID_MIN, ("sum", "size")]),
                 lambda: st.probe_keys(ID_MIN, ID_MAX, KEYS),
                 lambda: st.stats_column(*ID_MIN),
                 lambda: st.partition_groups(),
                 lambda: st.write_checkpoint_part(1, 1, with_adds=True)]
        got = []
        for call in calls:
            res, t = _timed(engine, call)
            assert _extracts(t) == set(), sorted(t)
            got.append(res)
        sel, agg, probe, (vals, nulls), groups, (data, rows, adds) = got
        assert sel == [] and groups == [] and len(vals) == 0 and len(nulls) == 0
        assert agg["group_rows"].tolist() == [0] and not agg["nonnull"].any() and (agg["arg_row"] == -1).all()
        assert len(probe["selected"]) == 0 and probe["unknown"] == 0 and probe["key_files"].tolist() == [0] * len(KEYS)
        assert (rows, adds) == (3, 0) and bytes(data[:4]) == b"PAR1"  # protocol, metaData and the remove
    finally:
        st.release()


def test_a_failed_call_leaves_no_timings_behind(engine, log_path):
    """With timing on, dr_state_partition_groups refuses a row out of range on the host, after its timed call
    began. The kernels of the untimed export plan that follows are not recorded, and the next filter reports
    the launches it reports on a state that saw no failure."""
    from delta_amd.delta_log import DeltaError
    keys = []
    for fails in (True, False):
        st = _replay(engine, log_path)
        engine.set_timing(True)
        try:
            if fails:
                with pytest.raises(DeltaError) as e:
                    st.partition_groups(rows=[F.N_LIVE])
                assert e.value.status == INVALID_ARG
            assert st.export_plan(0, 100, 1 << 20)[-1] == F.N_LIVE  # materialises the live side: kernels, no timed call
            sel = st.filter(_program())
            keys.append(set(engine.last_timings()))
        finally:
            engine.set_timing(False)
            st.release()
        assert 0 < len(sel) < F.N_LIVE
    assert keys[0] == keys[1], sorted(keys[0] ^ keys[1])
    assert {"k_pv_extract", "k_stats_extract"} <= keys[1]
