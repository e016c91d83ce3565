"""GPU parity of K5's statistics columns (DR_SRC_STATS_* on predicate columns, k_stats_extract,
dr_state_stats_column) and of data skipping (Snapshot.files_for_scan(..., data_skipping=True)) against
the corpus evaluator (tests/filter_stats_corpus.py: json.loads and three-valued logic): the typed
columns of every (source, type), the three evaluators, stats read from JSON commits, from a checkpoint's
add.stats column and after dr_state_apply, the refusals, and a column past the dictionary's limit."""
import json
import os

import pytest

from delta_amd import _native as N
from tests import filter_stats_corpus as F

pytestmark = pytest.mark.gpu
MODES = ("json", "checkpoint", "apply")
INVALID_ARG, UNSUPPORTED = 1, 12  # enum dr_status


@pytest.fixture(scope="module")
def engine():
    from delta_amd.delta_log import Engine
    return Engine.get(0)


@pytest.fixture(scope="module")
def corpus():
    """The live files, the predicates and the evaluator's selections, computed once."""
    files = F.live_files()
    preds = F.predicates()
    want = [sorted(f["path"] for f in F.expected(files, p)) for p in preds]
    assert sum(0 < len(w) < len(files) for w in want) >= 55  # the corpus discriminates
    return files, preds, want


def _state(engine, table_dir, mode):
    """The corpus table's state: replayed from JSON alone, from the checkpoint and the commits after it, or
    from the v1 state with the last commit applied on top (dr_state_apply)."""
    lp = F.build(table_dir, checkpoint=mode != "json")
    staged = engine.stage_log(lp, 1 if mode == "apply" else -1)
    st = staged.replay(0)
    staged.release()
    if mode != "apply":
        return st
    with open(os.path.join(lp, "%020d.json" % 2), "rb") as f:
        tail = engine.stage_files([(2, N.DR_FILE_JSON, 0, f.read())])
    try:
        return st.apply(tail, 0)
    finally:
        tail.release()
        st.release()


@pytest.fixture(scope="module")
def states(engine, tmp_path_factory):
    out = {m: _state(engine, str(tmp_path_factory.mktemp("stats_" + m)), m) for m in MODES}
    yield out
    for st in out.values():
        st.release()


@pytest.mark.parametrize("mode", MODES)
def test_stats_columns(states, corpus, mode):
    """dr_state_stats_column of every (source, type) it serves equals the evaluator's values and null flags."""
    st = states[mode]
    by_path = {f["path"]: f for f in corpus[0]}
    live = [by_path[a["path"]] for a in st.export(0)]
    assert len(live) == F.N_LIVE
    cases = [(src, path, typ) for path, typ in F.DTYPES.items() for src in (F.MIN, F.MAX)
             if typ != "string" and not typ.startswith("decimal")]
    cases += [(F.NULLCOUNT, path, "long") for path in F.DTYPES] + [(F.NUMRECORDS, (), "long")]
    for src, path, typ in cases:
        vals, nulls = st.stats_column(src, path, typ)
        want = [F.typed(f["stats"], src, path, typ) for f in live]
        assert [bool(z) for z in nulls] == [w is None for w in want], (src, path, typ)
        assert [int(v) for v in vals] == [0 if w is None else w[0] for w in want], (src, path, typ)
        assert any(w is not None for w in want) and any(w is None for w in want)
    nr, z = st.stats_column(N.DR_SRC_STATS_NUMRECORDS)  # count(*) from metadata
    assert int(nr.sum()) == sum(F.typed(f["stats"], F.NUMRECORDS, (), "long")[0] for f in live
                                if F.typed(f["stats"], F.NUMRECORDS, (), "long"))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("filter_eval", [0, 1, 2])
def test_filter_stats_corpus(engine, states, corpus, mode, filter_eval):
    """Every corpus predicate under DR_OPT_FILTER_EVAL 0, 1 and 2 selects exactly the evaluator's files."""
    from delta_amd.predicates import build_program
    st = states[mode]
    files, preds, want = corpus
    live = st.export(0)
    with engine.options(filter_eval=filter_eval):
        for p, w in zip(preds, want):
            sel = st.filter(build_program({"p": "integer"}, p))
            assert sel == sorted(set(sel))
            assert sorted(live[i]["path"] for i in sel) == w, p


@pytest.mark.parametrize("checkpoint", [False, True])
def test_files_for_scan_with_data_skipping(tmp_path, corpus, checkpoint):
    """files_for_scan(data_skipping=True) returns the records the evaluator keeps for the rewritten filters
    ANDed onto the partition conjuncts; with False (the default) what it returned before: partition pruning."""
    from delta_amd import skipping as K
    from delta_amd.delta_log import DeltaLog
    F.build(str(tmp_path), checkpoint=checkpoint)
    files = corpus[0]
    filters = [("and", ("=", F.C("p"), F.L("integer", 1)), (">=", F.C("id"), F.L("long", 1000))),
               ("<", F.C("id"), F.L("long", 9000)), ("like", F.C("s"), F.L("string", "n%"))]
    part = [f for f in files if f["partitionValues"]["p"] == "1"]
    skip = K.skipping_predicates(filters, F.METADATA)
    assert len(skip) == 2
    kept = F.expected(part, skip)
    assert 0 < len(kept) < len(part) < len(files)
    DeltaLog.clear_cache()
    try:
        snap = DeltaLog.for_table(str(tmp_path)).snapshot
        fields = ("path", "partitionValues", "size", "modificationTime", "stats")  # what the corpus writes of a record
        key = lambda recs: sorted(json.dumps({k: r[k] for k in fields}, sort_keys=True) for r in recs)  # noqa: E731
        assert key(snap.files_for_scan(filters, data_skipping=True)) == key(kept)
        assert key(snap.files_for_scan(filters)) == key(part) == key(snap.files_for_scan(filters, data_skipping=False))
        got = {s["path"] for _, group in snap.list_files(filters, data_skipping=True) for s in group}
        assert got == {os.path.join(str(tmp_path), f["path"]) for f in kept}
        snap.release()
    finally:
        DeltaLog.clear_cache()


def test_refusals_through_dr_filter(engine, states):
    """check_program's refusals of a statistics column reach the caller through dr_filter, before any device
    work; the state stays usable."""
    from delta_amd.delta_log import DeltaError
    from delta_amd.predicates import Program, OP_COL, OP_CODE
    st = states["json"]
    src = lambda s, t: t | s << N.DR_SRC_SHIFT  # noqa: E731
    cases = [
        (("x", src(1, 6)), "predicate column 0: minValues statistics have no BOOLEAN (type 6)"),
        (("x", src(2, 10)), "predicate column 0: maxValues statistics have no BINARY (type 10)"),
        (("x", src(3, 3)), "predicate column 0: nullCount is a LONG, not type 3"),
        (("", src(4, 0)), "predicate column 0: numRecords is a LONG, not type 0"),
        (("x", src(5, 4)), "predicate column 0: unknown source 5 (DR_SRC_PARTITION .. DR_SRC_STATS_NUMRECORDS)"),
        (("x", src(4, 4)), 'predicate column 0: numRecords takes the name "", not a path of 1 bytes'),
        (("a\x01\x01b", src(1, 4)), "predicate column 0: segment 1 of the statistics path is empty"),
        (("\x01".join("abcdefghi"), src(1, 4)), "predicate column 0: a statistics path has at most 8 segments, not 9"),
        (("y" * 256, src(2, 0)), "predicate column 0: a statistics path has at most 255 bytes, not 256"),
    ]
    for col, text in cases:
        with pytest.raises(DeltaError) as e:
            st.filter(Program(ops=[(OP_COL, 0), (OP_CODE["isnull"], 0)], cols=[col], lits=[]))
        assert (e.value.status, str(e.value)) == (INVALID_ARG, text)
    for typ in ("string", "decimal(12,2)"):
        with pytest.raises(DeltaError) as e:
            st.stats_column(F.MIN, ("s",), typ)
        assert e.value.status == UNSUPPORTED
    assert len(st.filter(Program(ops=[(OP_COL, 0), (OP_CODE["isnotnull"], 0)], cols=[("id", src(1, 4))], lits=[]))) > 0


def test_min_of_high_cardinality_runs_on_the_leaf_kernel(engine, tmp_path):
    """70 000 JSON-only files with a distinct minValues.id each: the column's dictionary is abandoned past
    DICT_MAX, so `id >= a AND id < b` runs on k_filter_leaf, not k_filter_dict, and selects exactly."""
    from delta_amd.predicates import build_program
    from delta_amd import skipping as K
    n = 70000
    log = os.path.join(str(tmp_path), "_delta_log")
    os.makedirs(log)
    with open(os.path.join(log, "%020d.json" % 0), "w") as f:
        f.write(json.dumps({"protocol": F.PROTOCOL}) + "\n" + json.dumps({"metaData": F.METADATA}) + "\n")
        for i in range(n):
            f.write('{"add":{"path":"g-%d","partitionValues":{"p":"0"},"size":1,"modificationTime":1,"dataChange":true,'
                    '"stats":"{\\"numRecords\\":10,\\"minValues\\":{\\"id\\":%d},\\"maxValues\\":{\\"id\\":%d}}"}}\n' % (i, 10 * i, 10 * i + 9))
    staged = engine.stage_log(log)
    st = staged.replay(0)
    staged.release()
    try:
        paths = [a["path"] for a in st.export(0)]
        a, b = 123456, 234567
        pred = K.rewrite(("and", (">=", F.C("id"), F.L("long", a)), ("<", F.C("id"), F.L("long", b))), K.data_schema(F.METADATA), ["p"])
        engine.set_timing(True)
        try:
            sel = st.filter(build_program({"p": "integer"}, [pred]))
            t = engine.last_timings()
        finally:
            engine.set_timing(False)
        ran = [k for k in t if k.startswith("k_filter")]
        assert any(k.startswith("k_filter_leaf") for k in ran) and "k_filter_dict" not in ran, sorted(t)
        assert "k_stats_extract" in t, sorted(t)
        want = sorted("g-%d" % i for i in range(n) if 10 * i + 9 >= a and 10 * i < b)
        assert sorted(paths[i] for i in sel) == want and 0 < len(want) < n
    finally:
        st.release()


def test_more_data_columns_than_one_program_holds(tmp_path, corpus):
    """Filters on 10 data columns beside a partition conjunct would lower to 20 predicate columns; dr_filter takes
    16. files_for_scan keeps the conjuncts that fit, answers -- where the partition-only call answers -- and
    returns exactly what the evaluator keeps for those conjuncts."""
    from delta_amd import skipping as K
    from delta_amd.delta_log import DeltaLog
    from delta_amd.predicates import build_program
    F.build(str(tmp_path), checkpoint=False)
    files = corpus[0]
    wide = [("!=", F.C("id"), F.L("long", 12)), ("=", F.C("b"), F.L("byte", -10)), ("!=", F.C("sh"), F.L("short", 3)),
            ("in", F.C("i"), [F.L("integer", 0), F.L("integer", 2147483647)]), ("!=", F.C("f"), F.L("float", 0.5)),
            ("!=", F.C("d"), F.L("double", 0.0)), ("!=", F.C("dt"), F.L("date", "2021-01-01")), ("isnotnull", F.C("s")),
            ("!=", F.C("n.x"), F.L("integer", 4)), ("<", F.C('we"ird'), F.L("string", "w3"))]
    filters = [("=", F.C("p"), F.L("integer", 2))] + wide
    part = [f for f in files if f["partitionValues"]["p"] == "2"]
    skip = K.skipping_predicates(filters, F.METADATA)
    assert len(skip) == len(wide) and len(build_program({"p": "integer"}, [filters[0]] + skip).cols) == 20
    fit = K.fit_limits({"p": "integer"}, [filters[0]], skip)
    assert fit == skip[:7] + [skip[9]]
    kept = F.expected(part, fit)
    assert 0 < len(kept) < len(part)
    DeltaLog.clear_cache()
    try:
        snap = DeltaLog.for_table(str(tmp_path)).snapshot
        got = snap.files_for_scan(filters, data_skipping=True)
        assert sorted(f["path"] for f in got) == sorted(f["path"] for f in kept)
        assert sorted(f["path"] for f in snap.files_for_scan(filters)) == sorted(f["path"] for f in part)
        assert {s["path"] for _, g in snap.list_files(filters, data_skipping=True) for s in g} == {
            os.path.join(str(tmp_path), f["path"]) for f in kept}
        snap.release()
    finally:
        DeltaLog.clear_cache()
