"""GPU parity of the string pattern predicates of K5 (dr_filter: DR_OP_STARTSWITH, DR_OP_ENDSWITH,
DR_OP_CONTAINS, DR_OP_LIKE) against the corpus evaluator (tests/filter_like_corpus.py): the three
evaluators, values read from JSON commits and from the checkpoint's map column, a string column past
the dictionary's capacity, the Snapshot layer, and the ABI's operand and pattern validation."""
import json
import os

import pytest

from tests import filter_like_corpus as F

pytestmark = pytest.mark.gpu

C, L, STR = F.C, F.L, F.STR
ALL = F.PREDICATES + F.ALWAYS_NULL + F.NEVER_TRUE


@pytest.fixture(scope="module")
def engine():
    from delta_amd.delta_log import Engine
    return Engine.get(0)


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


@pytest.fixture(scope="module")
def corpus_expected():
    """The corpus evaluator's selections over the table's live files, computed once."""
    files = F.live_files()
    return [sorted(f["path"] for f in F.expected(files, p)) for p in ALL]


@pytest.mark.parametrize("checkpoint", [False, True])
@pytest.mark.parametrize("filter_eval", [0, 1, 2])
def test_filter_like_corpus(engine, tmp_path, corpus_expected, checkpoint, filter_eval):
    """Every corpus predicate under DR_OPT_FILTER_EVAL 0 (the leaf once per dictionary code,
    k_dict_leaf), 1 (per file, k_filter_leaf_x) and 2 (the generic interpreter k_filter_typed)."""
    lp = F.build(str(tmp_path), checkpoint=checkpoint)
    with engine.options(filter_eval=filter_eval):
        n, got = _gpu_selected(engine, lp, ALL)
    assert n == F.N_LIVE
    for p, g, w in zip(ALL, got, corpus_expected):
        assert g == w, p


def _table(table, ptypes, rows):
    log = os.path.join(str(table), "_delta_log")
    os.makedirs(log)
    schema = {"type": "struct", "fields": [{"name": "x", "type": "long", "nullable": True, "metadata": {}}] +
              [{"name": c, "type": t, "nullable": True, "metadata": {}} for c, t in ptypes.items()]}
    md = {"id": "like", "format": {"provider": "parquet", "options": {}}, "schemaString": json.dumps(schema),
          "partitionColumns": list(ptypes), "configuration": {}, "createdTime": 1}
    with open(os.path.join(log, "%020d.json" % 0), "w") as f:
        f.write(json.dumps({"protocol": {"minReaderVersion": 1, "minWriterVersion": 2}}) + "\n")
        f.write(json.dumps({"metaData": md}) + "\n")
        for k, r in enumerate(rows):
            f.write(json.dumps({"add": {"path": "f%d" % k, "partitionValues": dict(zip(ptypes, r)), "size": 1 + k % 3,
                                        "modificationTime": 1000 + (k * 7) % 50, "dataChange": True}}) + "\n")
    return log


def test_filter_like_dictionary_overflow_falls_back(engine, tmp_path):
    """70,000 distinct strings (more than the u16 dictionary's 65,534 values): filter_eval = 0 falls
    back to the per-file kernel, for the low-cardinality column beside them too."""
    n = 70000
    ptypes = {"s": "string", "g": "integer"}
    rows = [("k%05d-é" % k, str(k % 7)) for k in range(n)]
    lp = _table(tmp_path, ptypes, rows)
    preds = [[("like", C("s"), STR("k_12%_é"))], [("contains", C("s"), STR("999"))],
             [("and", ("like", C("s"), STR("%7_-_")), ("=", C("g"), L("integer", 3)))]]
    files = [{"path": "f%d" % k, "partitionValues": dict(zip(ptypes, r))} for k, r in enumerate(rows)]
    want = [sorted(f["path"] for f in F.expected(files, p, ptypes)) for p in preds]
    with engine.options(filter_eval=0):
        live, got = _gpu_selected(engine, lp, preds)
    assert live == n and got == want and all(0 < len(w) < n for w in want)


def test_snapshot_layer_with_like_conjuncts(tmp_path):
    """Snapshot.files_for_scan and list_files with a `like` conjunct (beside a data predicate, which
    is left to the caller) return the AddFiles the corpus evaluator selects."""
    from delta_amd.delta_log import DeltaLog
    ptypes = {"dt": "string", "g": "integer"}
    days = ["2024-03-%02d" % d for d in range(1, 28)] + ["2024-04-01", "2024_03_01", None, ""]
    rows = [(days[k % len(days)], str(k % 4)) for k in range(500)]
    _table(tmp_path, ptypes, rows)
    files = [{"path": "f%d" % k, "partitionValues": dict(zip(ptypes, r)), "size": 1 + k % 3,
              "modificationTime": 1000 + (k * 7) % 50} for k, r in enumerate(rows)]
    like = ("like", C("dt"), STR("2024-03-0_"))
    pred = [("and", like, ("=", C("x"), L("long", 5))), ("=", C("g"), L("integer", 1))]
    kept = F.expected(files, [like, pred[1]], ptypes)
    assert 0 < len(kept) < len(files)
    DeltaLog.clear_cache()
    try:
        snap = DeltaLog.for_table(str(tmp_path)).snapshot
        got = snap.files_for_scan(pred)
        assert sorted(f["path"] for f in got) == sorted(f["path"] for f in kept)
        assert all(f["partitionValues"]["dt"].startswith("2024-03-0") and f["partitionValues"]["g"] == "1" for f in got)
        want = {}
        for f in kept:
            row = (f["partitionValues"]["dt"], int(f["partitionValues"]["g"]))
            want.setdefault(row, set()).add((f["size"], f["modificationTime"], os.path.join(str(tmp_path), f["path"])))
        rows_got = {row: {(s["length"], s["modificationTime"], s["path"]) for s in stats}
                    for row, stats in snap.list_files([like, pred[1]])}
        assert rows_got == want and len(rows_got) == 9
        esc = [("like", C("dt"), STR("2024#_03#__1"), "#")]
        assert sorted(f["path"] for f in snap.files_for_scan(esc)) == sorted(f["path"] for f in F.expected(files, esc, ptypes))
    finally:
        DeltaLog.clear_cache()


def test_pattern_abi_errors(engine, tmp_path):
    """dr_filter validates the operands and the pattern on the host: each violation is
    DR_E_INVALID_ARG naming the op and what was found, and the state stays usable."""
    from delta_amd import predicates as P
    from delta_amd.delta_log import DeltaError
    rows = [("abc", "abc", "1"), ("a%c", "x", "2"), (None, None, None)]
    lp = _table(tmp_path, {"s": "string", "b": "binary", "n": "integer"}, rows)
    cols = [("s", 0), ("b", P.type_code("binary")), ("n", P.type_code("integer"))]
    staged = engine.stage_log(lp)
    st = staged.replay(0)
    staged.release()
    LIKE = P.OP_CODE["like"]
    s_pat = [(0, b"a%")]
    cases = [
        # (ops, literals, message parts)
        ([(P.OP_COL, 2), (P.OP_LIT, 0), (LIKE, 92)], s_pat, ["op 2 (LIKE)", "STRING partition column", "column n"]),
        ([(P.OP_COL, 1), (P.OP_LIT, 0), (P.OP_CODE["startswith"], 0)], s_pat,
         ["op 2 (STARTSWITH)", "STRING partition column", "column b"]),
        ([(P.OP_COL, 0), (P.OP_COL, 0), (P.OP_CODE["contains"], 0)], s_pat,
         ["op 2 (CONTAINS)", "STRING or NULL literal", "column s"]),
        ([(P.OP_LIT, 0), (P.OP_LIT, 0), (P.OP_CODE["endswith"], 0)], s_pat,
         ["op 2 (ENDSWITH)", "STRING partition column", "literal 0"]),
        ([(P.OP_COL, 0), (P.OP_LIT, 0), (P.OP_CODE["endswith"], 0)], [(P.type_code("integer"), 5)],
         ["op 2 (ENDSWITH)", "STRING or NULL literal", "literal 0 of type 3"]),
        ([(P.OP_COL, 0), (P.OP_LIT, 0), (LIKE, 92)], [(0, b"abc\\")],
         ["op 2 (LIKE)", "the pattern 'abc\\' is invalid, it is not allowed to end with the escape character"]),
        ([(P.OP_COL, 0), (P.OP_LIT, 0), (LIKE, 92)], [(0, b"a\\bc")],
         ["op 2 (LIKE)", "the pattern 'a\\bc' is invalid, the escape character is not allowed to precede 'b'"]),
        ([(P.OP_COL, 0), (P.OP_LIT, 0), (LIKE, 0)], s_pat, ["op 2 (LIKE)", "escape character (arg 0)"]),
        ([(P.OP_COL, 0), (P.OP_LIT, 0), (LIKE, 0x10000)], s_pat, ["op 2 (LIKE)", "escape character (arg 65536)"]),
        ([(P.OP_COL, 0), (P.OP_LIT, 0), (LIKE, 0xD800)], s_pat, ["op 2 (LIKE)", "escape character (arg 55296)"]),
        ([(P.OP_COL, 0), (P.OP_LIT, 0), (LIKE, 0)], [(0, None)], ["op 2 (LIKE)", "escape character (arg 0)"]),
        ([(P.OP_COL, 0), (P.OP_LIT, 0), (LIKE, 92)], [(0, b"a\xff%")], ["op 2 (LIKE)", "not valid UTF-8"]),
        ([(P.OP_COL, 0), (P.OP_LIT, 0), (LIKE, 92)], [(0, b"%\xc3")], ["op 2 (LIKE)", "not valid UTF-8"]),
        ([(P.OP_LIT, 0), (LIKE, 92)], s_pat, ["stack underflow"]),
    ]
    try:
        for ops, lits, parts in cases:
            with pytest.raises(DeltaError) as e:
                st.filter(P.Program(ops=ops, cols=cols, lits=lits))
            assert e.value.code == "DR_E_INVALID_ARG", str(e.value)
            for part in parts:
                assert part in str(e.value), (part, str(e.value))
        # the state stays usable; a NULL literal of another type is a NULL pattern
        live = st.export(0)
        sel = st.filter(P.Program(ops=[(P.OP_COL, 0), (P.OP_LIT, 0), (LIKE, 92)], cols=cols, lits=[(0, b"a\\%_")]))
        assert [live[i]["path"] for i in sel] == ["f1"]
        sel = st.filter(P.Program(ops=[(P.OP_COL, 0), (P.OP_LIT, 0), (LIKE, 92), (P.OP_CODE["not"], 0)], cols=cols,
                                  lits=[(P.type_code("integer"), None)]))
        assert sel == []
    finally:
        st.release()
