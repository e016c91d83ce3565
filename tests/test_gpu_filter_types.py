"""GPU parity of K5 partition pruning (dr_filter) over timestamp, double, float, decimal and binary
partition columns against the oracle's filterFileList restatement (tests/filter_types_corpus.py):
the three evaluators, values read from JSON commits and from the checkpoint's map column, a column
past the dictionary's capacity, the Snapshot layer, and the ABI's literal validation."""
import json
import os

import pytest

from oracle import delta_oracle as O
from tests import filter_types_corpus as F

pytestmark = pytest.mark.gpu

C, L = F.C, F.L


@pytest.fixture(scope="module")
def engine():
    from delta_amd.delta_log import Engine
    return Engine.get(0)


def _gpu_selected(engine, lp, preds_list, cutoff=0):
    from delta_amd.predicates import build_program, partition_schema
    staged = engine.stage_log(lp)
    st = staged.replay(cutoff)
    staged.release()
    try:
        live = st.export(0)
        schema = partition_schema(next(a["metaData"] for a in st.nonfile if "metaData" in a))
        out = []
        for preds in preds_list:
            sel = st.filter(build_program(schema, preds))
            assert sel == sorted(set(sel))
            out.append(sorted(live[i]["path"] for i in sel))
        return out
    finally:
        st.release()


def _oracle_selected(lp, preds_list):
    snap = O.state_reconstruction(O.get_log_segment(lp), 0)
    schema = O.partition_schema(snap.metadata)
    return [sorted(f["path"] for f in F.expected(schema, snap.all_files, p)) for p in preds_list]


@pytest.fixture(scope="module")
def corpus_expected(tmp_path_factory):
    """The oracle's selections over the corpus table, computed once (the checkpointed table holds the
    same live files: checked by the file count below)."""
    lp = F.build(str(tmp_path_factory.mktemp("types-oracle")))
    snap = O.state_reconstruction(O.get_log_segment(lp), 0)
    assert snap.num_of_files == F.N_LIVE
    return _oracle_selected(lp, F.PREDICATES)


@pytest.mark.parametrize("checkpoint", [False, True])
@pytest.mark.parametrize("filter_eval", [0, 1, 2])
def test_filter_types_corpus(engine, tmp_path, corpus_expected, checkpoint, filter_eval):
    """Every corpus predicate under DR_OPT_FILTER_EVAL 0 (dictionary codes; decimal(38,10) has no
    dictionary, so its programs fall back to the typed leaf kernel), 1 (k_filter_leaf /
    k_filter_leaf_x) and 2 (the generic interpreter k_filter_typed)."""
    lp = F.build(str(tmp_path), checkpoint=checkpoint)
    if checkpoint:
        assert O.state_reconstruction(O.get_log_segment(lp), 0).num_of_files == F.N_LIVE
    with engine.options(filter_eval=filter_eval):
        got = _gpu_selected(engine, lp, F.PREDICATES)
    for p, g, w in zip(F.PREDICATES, got, corpus_expected):
        assert g == w, p


def _table(table, ptypes, rows):
    log = os.path.join(str(table), "_delta_log")
    os.makedirs(log)
    schema = {"type": "struct", "fields": [{"name": "x", "type": "long", "nullable": True, "metadata": {}}] +
              [{"name": c, "type": t, "nullable": True, "metadata": {}} for c, t in ptypes.items()]}
    md = {"id": "types", "format": {"provider": "parquet", "options": {}}, "schemaString": json.dumps(schema),
          "partitionColumns": list(ptypes), "configuration": {}, "createdTime": 1}
    with open(os.path.join(log, "%020d.json" % 0), "w") as f:
        f.write(json.dumps({"protocol": {"minReaderVersion": 1, "minWriterVersion": 2}}) + "\n")
        f.write(json.dumps({"metaData": md}) + "\n")
        for k, r in enumerate(rows):
            f.write(json.dumps({"add": {"path": "f%d" % k, "partitionValues": dict(zip(ptypes, r)), "size": 1 + k % 3,
                                        "modificationTime": 1000 + (k * 7) % 50, "dataChange": True}}) + "\n")
    return log


def test_filter_types_dictionary_overflow_falls_back(engine, tmp_path):
    """70,000 distinct doubles (more than the u16 dictionary's 65,534 values) take the typed leaf
    kernel; the 7-value timestamp column beside them still selects exactly."""
    n = 70000
    rows = [("%d.25" % (k - 100), "2020-03-0%d 00:00:00" % (1 + k % 7)) for k in range(n)]
    lp = _table(tmp_path, {"d": "double", "ts": "timestamp"}, rows)
    preds = [[(">=", C("d"), F.DBL(69890.25))], [("=", C("ts"), F.T("2020-03-04"))],
             [("and", ("<", C("d"), F.DBL(-80.0)), (">", C("ts"), F.T("2020-03-05 12:00:00")))]]
    got, want = _gpu_selected(engine, lp, preds), _oracle_selected(lp, preds)
    assert got == want and all(0 < len(w) < n for w in want)


def test_snapshot_layer_on_timestamp_partitions(tmp_path):
    """Snapshot.files_for_scan, list_files and initial_files over an hourly timestamp partition equal
    the oracle's selection; list_files' group rows are the values cast by cast_partition_value."""
    from delta_amd.delta_log import DeltaLog
    from delta_amd.predicates import cast_partition_value
    hours = ["2020-03-01 %02d:00:00" % h for h in range(24)] + ["2020-03-02T00:00:00Z", None, "bad"]
    rows = [(hours[k % len(hours)], str(k % 4)) for k in range(500)]
    lp = _table(tmp_path, {"hour": "timestamp", "g": "integer"}, rows)
    ref = O.state_reconstruction(O.get_log_segment(lp), 0)
    schema = O.partition_schema(ref.metadata)
    pred = [(">=", C("hour"), F.T("2020-03-01 06:00:00")), ("<", C("hour"), F.T("2020-03-01 09:00:00")),
            ("=", C("g"), L("integer", 1))]
    kept = O.filter_file_list(schema, ref.all_files, pred)
    assert 0 < len(kept) < len(ref.all_files)
    DeltaLog.clear_cache()
    try:
        snap = DeltaLog.for_table(str(tmp_path)).snapshot
        assert sorted(f["path"] for f in snap.files_for_scan(pred)) == sorted(f["path"] for f in kept)
        want = {}
        for f in kept:
            row = tuple(cast_partition_value(f["partitionValues"].get(c), t) for c, t in schema.items())
            want.setdefault(row, set()).add((f["size"], f["modificationTime"], os.path.join(str(tmp_path), f["path"])))
        got = {row: {(s["length"], s["modificationTime"], s["path"]) for s in stats}
               for row, stats in snap.list_files(pred)}
        assert got == want and len(got) == 3
        order = sorted(ref.all_files, key=lambda f: (f["modificationTime"], f["path"].encode("utf-8")))
        idx = {f["path"]: i for i, f in enumerate(order)}
        init = snap.initial_files(pred)
        assert [(g["add"]["path"], g["index"]) for g in init] == sorted(((f["path"], idx[f["path"]]) for f in kept),
                                                                         key=lambda t: t[1])
    finally:
        DeltaLog.clear_cache()


def test_malformed_decimal_literal_is_invalid_arg(engine, tmp_path):
    """dr_filter validates literals on the host: a decimal literal that is not 16 bytes, one beyond
    its precision and one of another (p, s) than its column are DR_E_INVALID_ARG naming the
    literal, and the state stays usable."""
    from delta_amd import predicates as P
    from delta_amd.delta_log import DeltaError
    rows = [(v,) for v in ("1.25", "-3.5", None, "7", "1.25")]
    lp = _table(tmp_path, {"m": "decimal(12,2)"}, rows)
    code = P.type_code("decimal(12,2)")
    staged = engine.stage_log(lp)
    st = staged.replay(0)
    staged.release()
    try:
        eq = [(P.OP_COL, 0), (P.OP_LIT, 1), (P.OP_CODE["="], 0), (P.OP_COL, 0), (P.OP_LIT, 0), (P.OP_CODE["="], 0),
              (P.OP_CODE["or"], 0)]
        ok = P.decimal_bytes(125)
        for bad_type, bad in ((code, ok[:15]), (code, ok + b"\0"), (code, P.decimal_bytes(10 ** 12)),
                              (P.type_code("decimal(12,3)"), ok), (P.type_code("double"), 5),
                              (99, 5)):  # no dr_pred_type code
            with pytest.raises(DeltaError) as e:
                st.filter(P.Program(ops=eq, cols=[("m", code)], lits=[(code, ok), (bad_type, bad)]))
            assert e.value.code == "DR_E_INVALID_ARG" and "literal 1" in str(e.value), str(e.value)
        sel = st.filter(P.build_program({"m": "decimal(12,2)"}, [("=", C("m"), F.M2(125))]))
        live = st.export(0)
        assert sorted(live[i]["path"] for i in sel) == ["f0", "f4"]
    finally:
        st.release()


@pytest.mark.parametrize("filter_eval", [0, 1, 2])
def test_filter_timestamps_beyond_datetime_years(engine, tmp_path, filter_eval):
    """Negative years, year 0 and years above 9999 (the device's signed-year path, which Spark has
    and the oracle's datetime has not) under the three evaluators, against the corpus restatement
    of their microseconds."""
    lp = F.build_years(str(tmp_path))
    snap = O.state_reconstruction(O.get_log_segment(lp), 0)
    want = [sorted(f["path"] for f in F.expected_years(F.YEARS_TYPES, snap.all_files, p)) for p in F.YEARS_PREDICATES]
    with engine.options(filter_eval=filter_eval):
        got = _gpu_selected(engine, lp, F.YEARS_PREDICATES)
    for p, g, w in zip(F.YEARS_PREDICATES, got, want):
        assert g == w, p


def test_list_files_rows_beyond_datetime_years(tmp_path):
    """Snapshot.list_files on the years table: a file selected by a year datetime cannot hold keeps a
    non-NULL group row, the microseconds dr_filter compared."""
    from delta_amd.delta_log import DeltaLog
    F.build_years(str(tmp_path))
    pred = [("<", C("ts"), F.TY("0001-01-01 00:00:00"))]
    files = [F._years_add(i) for i in range(F.N_YEARS)]
    want = {}
    for f in F.expected_years(F.YEARS_TYPES, files, pred):
        row = (F.cast_timestamp_any_year(f["partitionValues"]["ts"], "timestamp"), int(f["partitionValues"]["part"]))
        want.setdefault(row, set()).add(os.path.join(str(tmp_path), f["path"]))
    DeltaLog.clear_cache()
    try:
        snap = DeltaLog.for_table(str(tmp_path)).snapshot
        got = {row: {s["path"] for s in stats} for row, stats in snap.list_files(pred)}
        assert got == want and len(got) == 12 and all(isinstance(r[0], int) for r in got)
    finally:
        DeltaLog.clear_cache()
