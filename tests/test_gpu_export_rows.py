"""Selected-rows export (dr_state_export_rows): the pruned rows of a side fetched by position, in the
caller's order, without taking the whole side -- what PartitionFiltering.filesForScan
(D/PartitionFiltering.scala:27-42), TahoeFileIndex.listFiles (D/files/TahoeFileIndex.scala:58-81) and
DeltaSourceSnapshot.initialFiles (D/files/DeltaSourceSnapshot.scala:53-95) hand on. Every one of the
24 columns equals dr_state_export's gathered at the rows with numpy and rebased to 0, byte for byte,
on both device paths: the walk of a side that is not resident and the gather from a resident one."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import delta_oracle as O
from tests import filter_corpus as F

pytestmark = pytest.mark.gpu

COL, LIT = F.C, F.L
SCALARS = ("size", "modification_time", "deletion_timestamp", "deletion_timestamp_valid",
           "extended_file_metadata", "stats_null", "pv_null", "tags_null")


@pytest.fixture(scope="module")
def engine():
    from delta_amd.delta_log import Engine
    return Engine.get(0)


def _ranges(off, idx):
    """The variable-length items `idx` of an offset column: (their offsets from 0, the source
    positions of their elements in order)."""
    idx = np.asarray(idx, dtype=np.int64)
    lens = off[idx + 1] - off[idx]
    new = np.zeros(len(idx) + 1, dtype=np.int64)
    np.cumsum(lens, out=new[1:])
    src = np.repeat(off[idx] - new[:-1], lens) + np.arange(int(new[-1]), dtype=np.int64)
    return new, src


def _expected(full, rows):
    """dr_state_export's columns gathered at `rows` on the host."""
    rows = np.asarray(rows, dtype=np.int64)
    out = {name: full[name][rows] for name in SCALARS}
    for s in ("path", "stats"):
        out[s + "_off"], src = _ranges(full[s + "_off"], rows)
        out[s + "_bytes"] = full[s + "_bytes"][src]
    for side in ("pv", "tags"):
        out[side + "_entry_off"], ent = _ranges(full[side + "_entry_off"], rows)
        out[side + "_val_null"] = full[side + "_val_null"][ent]
        for kv in ("key", "val"):
            out["%s_%s_off" % (side, kv)], src = _ranges(full["%s_%s_off" % (side, kv)], ent)
            out["%s_%s_bytes" % (side, kv)] = full["%s_%s_bytes" % (side, kv)][src]
    return out


def _assert_columns(got, want, what):
    assert set(got) == set(want) and len(want) == 24
    for name, w in want.items():
        g = got[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name)


def _row_sets(n, seed):
    rng = np.random.default_rng(seed)
    sets = {"empty": [], "all": list(range(n)), "reversed": list(range(n - 1, -1, -1)),
            "every7th": list(range(0, n, 7)), "random": [int(x) for x in rng.integers(0, max(n, 1), size=n)]}
    if n:
        sets["first"] = [0]
        sets["last"] = [n - 1]
    return sets


def _copy(cols):
    return {k: v.copy() for k, v in cols.items()}


def _check_rows(st, which, full, sets, what):
    n = len(full["path_off"]) - 1
    for name, rows in sets.items():
        got = st.export_rows(which, rows)
        _assert_columns(got, _expected(full, rows), (what, which, name))
        assert got["path_off"][0] == 0 and len(got["path_off"]) == len(rows) + 1
        if name == "all":  # the whole export itself
            assert len(rows) == n
            _assert_columns(got, full, (what, which, "whole"))


def _replay(engine, lp, cutoff):
    staged = engine.stage_log(lp)
    try:
        return staged.replay(cutoff)
    finally:
        staged.release()


def _shapes_table(root):
    """A checkpoint + churn commits + one hand-written commit with every record shape: null, escaped
    and missing partition values, a missing partitionValues, tags present and null, stats null, an
    absolute path that is canonicalised, a remove with and one without deletionTimestamp."""
    from delta_amd.testing import synth as S
    spec = S.ChurnSpec(ckpt_files=600, ckpt_version=1, n_deltas=2, removes_per_delta=60, adds_per_delta=60,
                       readd_frac=0.5, ncols=2)
    S.build_table(root, spec, seed=23, row_group_size=250)
    lp = os.path.join(root, "_delta_log")
    mt = S.T0 + 77
    lines = [
        '{"add":{"path":"/abs//x.parquet","partitionValues":{"p0":"2020-01-01","p1":"7"},"size":1,'
        '"modificationTime":%d,"dataChange":true,"stats":"{\\"numRecords\\":3}","tags":{"k":"v","n":null}}}' % mt,
        '{"add":{"path":"a.parquet","partitionValues":{"p0":"2020-01-01","p1":null},"size":2,'
        '"modificationTime":%d,"dataChange":true,"stats":null,"tags":null}}' % mt,
        '{"add":{"path":"\\u00e9.parquet","partitionValues":{"p0":"2020-01-0\\u0031","p\\u0031":"\\u0037"},"size":3,'
        '"modificationTime":%d,"dataChange":true,"tags":{}}}' % mt,
        '{"add":{"path":"m1.parquet","partitionValues":{"p0":"2020-01-02"},"size":4,"modificationTime":%d,'
        '"dataChange":true}}' % mt,
        '{"add":{"path":"m2.parquet","size":5,"modificationTime":%d,"dataChange":true,"stats":"{}"}}' % mt,
        '{"remove":{"path":"gone1.parquet","deletionTimestamp":%d,"dataChange":true,"extendedFileMetadata":true,'
        '"partitionValues":{"p0":"2020-01-03","p1":"1"},"size":9,"tags":{"t":"1"}}}' % (mt + 1),
        '{"remove":{"path":"gone2.parquet","dataChange":true}}',
    ]
    v = spec.ckpt_version + spec.n_deltas + 1
    with open(os.path.join(lp, "%020d.json" % v), "w") as f:
        f.write("\n".join(lines) + "\n")
    return lp, v


def test_rows_of_both_sides_on_both_paths(engine, tmp_path):
    """Every record shape, both sides, every row set; first on a freshly replayed state (nothing
    resident: the walk path; the expected whole export comes from a second state of the segment),
    then after materialize() (the gather path). Cutoff -1: the remove without a deletionTimestamp
    (delTimestamp 0) survives too."""
    lp, _ = _shapes_table(str(tmp_path))
    ref = _replay(engine, lp, -1)
    st = _replay(engine, lp, -1)
    try:
        full = {w: _copy(ref.export_columns(w)) for w in (0, 1)}
        tomb = ref.export(1)
        byp = {r["path"]: r for r in tomb}
        assert byp["gone1.parquet"]["deletionTimestamp"] is not None and byp["gone2.parquet"]["deletionTimestamp"] is None
        assert any(r["path"].endswith("abs/x.parquet") and r["tags"] == {"k": "v", "n": None} for r in ref.export(0))
        sets = {w: _row_sets(len(full[w]["path_off"]) - 1, 100 + w) for w in (0, 1)}
        assert len(sets[0]["all"]) > 600 and len(sets[1]["all"]) > 64  # more than one wave of rows a side
        for w in (0, 1):
            _check_rows(st, w, full[w], sets[w], "walk")
        assert st.materialize() > 0
        for w in (0, 1):
            _check_rows(st, w, full[w], sets[w], "gather")
        # records through the same columns
        pick = sets[0]["random"][:50]
        live = ref.export(0)
        assert st.export_rows_records(0, pick) == [live[i] for i in pick]
        pick = sets[1]["random"][:50]
        assert st.export_rows_records(1, pick) == [tomb[i] for i in pick]
    finally:
        st.release()
        ref.release()


def _walk_then_gather(st, seed):
    """The random draw of both sides on the state's walk path, then -- the whole export taken, which
    leaves the side resident -- on its gather path."""
    n = (st.counts["num_files"], st.counts["num_removes"])
    rng = np.random.default_rng(seed)
    rows = {w: [int(x) for x in rng.integers(0, max(n[w], 1), size=n[w])] for w in (0, 1)}
    walked = {w: st.export_rows(w, rows[w]) for w in (0, 1)}
    for w in (0, 1):
        full = _copy(st.export_columns(w))
        assert len(full["path_off"]) - 1 == n[w]
        want = _expected(full, rows[w])
        _assert_columns(walked[w], want, ("walk", w))
        _assert_columns(st.export_rows(w, rows[w]), want, ("gather", w))
    return n


def test_rows_of_a_json_only_log(engine, tmp_path):
    from delta_amd.testing import synth as S
    exp = S.build_config(1, str(tmp_path), scale=0.05)
    st = _replay(engine, os.path.join(str(tmp_path), "_delta_log"), exp.min_file_retention_timestamp)
    try:
        n = _walk_then_gather(st, 5)
        assert n[0] > 0
    finally:
        st.release()


def test_rows_of_an_applied_state(engine, tmp_path):
    """A state built by dr_state_apply over a base plus a tail: checkpoint rows and JSON lines of two
    sources (the src_id / json_bases path of the walk)."""
    from delta_amd import _native as N
    from delta_amd.testing import synth as S
    lp, v = _shapes_table(str(tmp_path))
    base = _replay(engine, lp, -1)
    tail_text = ('{"add":{"path":"t.parquet","partitionValues":{"p0":"2020-01-01","p1":"7"},"size":3,'
                 '"modificationTime":%d,"dataChange":true,"tags":{"a":"b"}}}\n'
                 '{"remove":{"path":"a.parquet","deletionTimestamp":5}}\n'
                 '{"remove":{"path":"m1.parquet"}}\n' % (S.T0 + 99))
    tail = engine.stage_files([(v + 1, N.DR_FILE_JSON, 0, tail_text.encode("utf-8"))])
    st = base.apply(tail, -1)
    tail.release()
    try:
        n = _walk_then_gather(st, 6)
        assert n[0] == base.counts["num_files"] - 1 and n[1] == base.counts["num_removes"] + 2
        assert "t.parquet" in {r["path"] for r in st.export_rows_records(0, range(n[0]))}
    finally:
        st.release()
        base.release()


def test_refusals_leave_the_state_usable(engine, tmp_path):
    from delta_amd import _native as N
    from delta_amd.delta_log import DeltaError
    from delta_amd.testing import synth as S
    exp = S.build_config(3, str(tmp_path), scale=0.002)
    st = _replay(engine, os.path.join(str(tmp_path), "_delta_log"), exp.min_file_retention_timestamp)
    try:
        n = st.counts["num_files"]
        for rows, pos in (([n], 0), ([-1], 0), ([0, 1, n], 2), ([0, -1, n], 1)):
            with pytest.raises(DeltaError) as ei:
                st.export_rows(0, rows)
            assert ei.value.code == "DR_E_INVALID_ARG"
            assert "rows[%d]" % pos in str(ei.value) and str(rows[pos]) in str(ei.value), str(ei.value)
        with pytest.raises(DeltaError) as ei:
            st.export_rows(2, [0])
        assert ei.value.code == "DR_E_INVALID_ARG" and "which = 2" in str(ei.value)
        e, h = N.dr_export(), C.c_void_p()
        lib = engine.lib
        assert lib.dr_state_export_rows(st.h, 0, None, 1, C.byref(h), C.byref(e)) == 1  # DR_E_INVALID_ARG
        assert "position 0" in lib.dr_state_last_error(st.h).decode() and not h.value
        assert lib.dr_state_export_rows(st.h, 0, None, -1, C.byref(h), C.byref(e)) == 1
        assert "nrows" in lib.dr_state_last_error(st.h).decode()
        # NULL rows with nrows = 0 is a valid empty selection
        assert lib.dr_state_export_rows(st.h, 0, None, 0, C.byref(h), C.byref(e)) == N.DR_OK
        assert e.n == 0 and e.path_off[0] == 0 and e.pv_key_off[0] == 0 and e.tags_val_off[0] == 0
        assert lib.dr_range_release(h) == N.DR_OK
        # the state still serves: a valid call, equal to the whole export's rows
        full = _copy(st.export_columns(0))
        rows = [n - 1, 0, n // 2, 0]
        _assert_columns(st.export_rows(0, rows), _expected(full, rows), "after refusals")
        assert st.counts["num_files"] == exp.num_files
    finally:
        st.release()


def test_rows_outlive_their_state_and_context(tmp_path):
    """A rows export is a dr_range: its host columns stay readable after dr_state_release and after
    dr_ctx_destroy, and a second dr_range_release is refused."""
    from delta_amd import _native as N
    from delta_amd.delta_log import Engine, State
    from delta_amd.testing import synth as S
    exp = S.build_config(3, str(tmp_path), scale=0.003)
    eng = Engine(0)  # a context of its own: destroyed below
    st = _replay(eng, os.path.join(str(tmp_path), "_delta_log"), exp.min_file_retention_timestamp)
    n, nt = st.counts["num_files"], st.counts["num_removes"]
    rng = np.random.default_rng(9)
    jobs = [(0, [int(x) for x in rng.integers(0, n, size=500)]), (0, list(range(n - 1, -1, -3))),
            (1, [int(x) for x in rng.integers(0, nt, size=200)])]

    def native(which, rows):
        e, h = N.dr_export(), C.c_void_p()
        arr = (C.c_int64 * len(rows))(*rows)
        eng.check(eng.lib.dr_state_export_rows(st.h, which, arr, len(rows), C.byref(h), C.byref(e)))
        return h, e

    held = [native(0, jobs[0][1])]  # walk path
    full = {w: _copy(st.export_columns(w)) for w in (0, 1)}
    held += [native(w, rows) for w, rows in jobs[1:]]  # gather path
    st.release()

    def check(k):
        which, rows = jobs[k]
        _assert_columns(_copy(State._columns(held[k][1])), _expected(full[which], rows), k)

    check(0)  # the state is gone
    assert eng.lib.dr_range_release(held[0][0]) == N.DR_OK
    assert eng.lib.dr_range_release(held[0][0]) == 1  # DR_E_INVALID_ARG: not a live range any more
    eng.lib.dr_ctx_destroy(eng.ctx)
    eng.ctx = None
    check(1)  # the context is gone
    check(2)
    assert eng.lib.dr_range_release(held[1][0]) == N.DR_OK
    assert eng.lib.dr_range_release(held[2][0]) == N.DR_OK


def _no_whole_export(monkeypatch):
    from delta_amd.delta_log import State

    def refuse(self, which):
        raise AssertionError("the whole side was fetched")
    monkeypatch.setattr(State, "export", refuse)


def test_config4_files_for_scan_fetches_the_pruned_rows_only(tmp_path, monkeypatch):
    """Config 4's flow at reduced scale (100 checkpoint parts, 4 partition columns): filesForScan's
    records equal the oracle's filterFileList and the generator's count, and the whole side is never
    exported."""
    from delta_amd.delta_log import DeltaLog, ManualClock
    from delta_amd.testing import synth as S
    scale = 0.002
    exp = S.build_config(4, str(tmp_path), scale=scale, workers=4)
    lp = os.path.join(str(tmp_path), "_delta_log")
    DeltaLog.clear_cache()
    snap = DeltaLog.for_table(str(tmp_path), clock=ManualClock(exp.min_file_retention_timestamp + 604800000)).snapshot
    ref = O.state_reconstruction(O.get_log_segment(lp), snap.min_file_retention_timestamp)
    want = sorted(O.filter_file_list(O.partition_schema(ref.metadata), ref.all_files, S.config4_predicate()),
                  key=lambda f: f["path"])
    with monkeypatch.context() as m:
        _no_whole_export(m)
        got = sorted(snap.files_for_scan(S.config4_predicate()), key=lambda f: f["path"])
    assert got == want
    assert len(got) == S.config4_selected(str(tmp_path), scale) > 0
    assert snap._all is None
    # with the side cached the same records come from it
    assert len(snap.all_files) == exp.num_files
    assert sorted(snap.files_for_scan(S.config4_predicate()), key=lambda f: f["path"]) == want
    DeltaLog.clear_cache()


def _churn_snapshot(root, seed, ckpt_files, ckpt_version, n_deltas, per_delta, rg):
    from delta_amd.delta_log import DeltaLog, ManualClock
    from delta_amd.testing import synth as S
    spec = S.ChurnSpec(ckpt_files=ckpt_files, ckpt_version=ckpt_version, n_deltas=n_deltas, removes_per_delta=per_delta,
                       adds_per_delta=per_delta, readd_frac=0.5, ncols=4)
    exp = S.build_table(root, spec, seed=seed, row_group_size=rg)
    DeltaLog.clear_cache()
    snap = DeltaLog.for_table(root, clock=ManualClock(exp.min_file_retention_timestamp + 604800000)).snapshot
    ref = O.state_reconstruction(O.get_log_segment(os.path.join(root, "_delta_log")), snap.min_file_retention_timestamp)
    return snap, ref


def test_list_files_fetches_the_pruned_rows_only(tmp_path, monkeypatch):
    """test_tahoe_list_files' table and comparison with the whole-side export forbidden; without a
    filter listFiles still goes through all_files."""
    import datetime as dt
    from delta_amd.delta_log import DeltaLog
    snap, ref = _churn_snapshot(str(tmp_path), 9, 2000, 2, 2, 300, 700)
    schema = O.partition_schema(ref.metadata)
    pred = [("<", COL("p1"), LIT("integer", 40))]

    def wanted(kept):
        want = {}
        for f in kept:
            row = []
            for c, t in schema.items():
                v = O.cast_string(f["partitionValues"].get(c), t)
                row.append(dt.date(1970, 1, 1) + dt.timedelta(days=v) if t == "date" and v is not None
                           else (bool(v) if t == "boolean" and v is not None else v))
            want.setdefault(tuple(row), set()).add((f["size"], f["modificationTime"], os.path.join(str(tmp_path), f["path"])))
        return want

    def listed(filters):
        return {row: {(s["length"], s["modificationTime"], s["path"]) for s in stats} for row, stats in snap.list_files(filters)}

    with monkeypatch.context() as m:
        _no_whole_export(m)
        got = listed(pred)
        assert got == wanted(O.filter_file_list(schema, ref.all_files, pred)) and len(got) > 1
        assert snap._all is None
        with pytest.raises(AssertionError, match="whole side"):
            snap.list_files()  # no selection: all_files
    assert listed(()) == wanted(ref.all_files)
    assert listed(pred) == got  # the side is cached now: indexed as before
    DeltaLog.clear_cache()


def test_initial_files_fetches_the_kept_rows_only(tmp_path, monkeypatch):
    """test_delta_source_initial_files' table and comparison with the whole-side export forbidden
    whenever a partition-only filter selects; without one initialFiles goes through all_files."""
    from delta_amd.delta_log import DeltaLog
    from delta_amd.testing import synth as S
    snap, ref = _churn_snapshot(str(tmp_path), 7, 3000, 5, 3, 400, 1000)
    order = sorted(ref.all_files, key=lambda f: (f["modificationTime"], f["path"].encode("utf-8")))
    idx = {f["path"]: i for i, f in enumerate(order)}
    schema = O.partition_schema(ref.metadata)
    part = ("in", COL("p1"), [LIT("integer", v) for v in range(0, 300)])
    mixed = ("and", ("=", COL("p2"), LIT("string", S.WORDS[3])), ("=", COL("value"), LIT("integer", 1)))

    def check(filters):
        got = snap.initial_files(filters)
        keep = O.filter_file_list(schema, order, [part]) if filters else order
        want = sorted(keep, key=lambda f: idx[f["path"]])
        assert [(g["add"], g["index"]) for g in got] == [(f, idx[f["path"]]) for f in want]
        assert all(g["version"] == snap.version and g["remove"] is None and not g["isLast"] for g in got)
        return len(got)

    with monkeypatch.context() as m:
        _no_whole_export(m)
        assert 0 < check([part]) < len(order)
        check([part, mixed])
        assert snap._all is None
        with pytest.raises(AssertionError, match="whole side"):
            snap.initial_files([])
        with pytest.raises(AssertionError, match="whole side"):
            snap.initial_files([mixed])  # names a data column: not applied, no selection
    assert check([]) == len(order)
    check([part])  # the side is cached now
    DeltaLog.clear_cache()
