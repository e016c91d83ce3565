"""Path lookup (dr_state_lookup_paths): which side of a resident state holds a given path, and at
which export position -- the state-side question of DeltaCommand.generateCandidateFileMap /
getTouchedFile (D/commands/DeltaCommand.scala:96-104,159-168), VacuumCommand's anti-join
(D/commands/VacuumCommand.scala:185-206) and OptimisticTransaction.checkForConflicts
(D/OptimisticTransaction.scala:829-833). Expectations come from the oracle's own canonicalisation and
key (O.canonicalize_path, O.replay_key) over the state's whole exports: a query expects the (side,
position) of the exported record with its key, else absent."""
import os
import threading

import numpy as np
import pytest

from oracle import delta_oracle as O
from tests import filter_corpus as F

pytestmark = pytest.mark.gpu

ABSENT, LIVE, TOMB = 0, 1, 2


@pytest.fixture(scope="module")
def engine():
    from delta_amd.delta_log import Engine
    return Engine.get(0)


def _replay(engine, lp, cutoff):
    staged = engine.stage_log(lp)
    try:
        return staged.replay(cutoff)
    finally:
        staged.release()


def _key(q: bytes) -> str:
    """The oracle's replay key of a query's bytes. Its functions only look at ASCII ('/', "file:"),
    so latin-1 carries any byte string, valid UTF-8 or not, through them unchanged."""
    return O.replay_key(O.canonicalize_path(q.decode("latin-1")))


def _expect_map(st):
    """{replay key: (hit, export position)} over both whole exports of the state."""
    m = {}
    for side in (0, 1):
        for pos, rec in enumerate(st.export(side)):
            k = _key(rec["path"].encode("utf-8"))
            assert k not in m, k
            m[k] = (side + 1, pos)
    return m


def _check(st, queries, emap, what=""):
    queries = [q.encode("utf-8") if isinstance(q, str) else q for q in queries]
    hit, row = st.lookup_paths(queries)
    assert hit.dtype == np.uint8 and row.dtype == np.int64 and len(hit) == len(row) == len(queries)
    want = [emap.get(_key(q), (ABSENT, -1)) for q in queries]
    bad = [(i, queries[i], int(hit[i]), int(row[i]), want[i]) for i in range(len(queries))
           if (int(hit[i]), int(row[i])) != want[i]]
    assert not bad, (what, len(bad), bad[:5])
    return hit, row


def _variants(paths, seed):
    """The query set of a list of known paths: themselves, shuffled with repeats, each with its last
    byte changed, one byte appended ('x' and '/'), its last and its first byte dropped, never-seen
    names and the empty path."""
    paths = [p.encode("utf-8") if isinstance(p, str) else p for p in paths]
    rng = np.random.default_rng(seed)
    q = list(paths)
    q += [paths[int(i)] for i in rng.integers(0, len(paths), size=len(paths) + 17)]
    for p in paths:
        if p:
            q += [p[:-1] + bytes([p[-1] ^ 1]), p[:-1], p[1:]]
        q += [p + b"x", p + b"/"]
    q += [b"never-%d.parquet" % i for i in range(40)] + [b"/never/seen.parquet", b"file:/never.parquet", b"file:", b"/", b"//", b""]
    return q


def _shapes_table(root):
    """A 600-row checkpoint in three row groups, two churn commits (removes with deletionTimestamps
    on both sides of the generator's cutoff, adds, re-adds) and one hand-written commit: an absolute
    path with '//', the two spellings of a file: URI, an add written with a JSON escape, an empty
    path, a remove with and one without deletionTimestamp."""
    from delta_amd.testing import synth as S
    spec = S.ChurnSpec(ckpt_files=600, ckpt_version=1, n_deltas=2, removes_per_delta=60, adds_per_delta=60,
                       readd_frac=0.5, ncols=2)
    exp = S.build_table(root, spec, seed=31, row_group_size=250)
    lp = os.path.join(root, "_delta_log")
    mt = S.T0 + 77
    add = '{"add":{"path":"%s","partitionValues":{"p0":"2020-01-01","p1":"7"},"size":%d,"modificationTime":%d,"dataChange":true}}'
    lines = [add % (p, k + 1, mt) for k, p in enumerate(
        ["/abs//x.parquet", "file:/t/k.parquet", "file:///t/m.parquet", "\\u00e9.parquet", "", "a.parquet", "m1.parquet"])]
    lines += ['{"remove":{"path":"gone1.parquet","deletionTimestamp":%d,"dataChange":true}}' % (exp.min_file_retention_timestamp + 5),
              '{"remove":{"path":"gone2.parquet","dataChange":true}}']
    v = spec.ckpt_version + spec.n_deltas + 1
    with open(os.path.join(lp, "%020d.json" % v), "w") as f:
        f.write("\n".join(lines) + "\n")
    return lp, v, exp


SPELLINGS = ["/abs/x.parquet", "/abs//x.parquet/", "file:/abs/x.parquet", "file:///abs/x.parquet", "/abs//x.parquet"]


def _all_paths(engine, lp):
    """Every path the segment's last action leaves on either side at cutoff -1 (nothing expired)."""
    st = _replay(engine, lp, -1)
    try:
        return [r["path"] for side in (0, 1) for r in st.export(side)]
    finally:
        st.release()


def _shape_queries(engine, lp):
    return _variants(_all_paths(engine, lp), 3) + SPELLINGS + ["file:///t/k.parquet", "file:/t/k.parquet", "file:/t/m.parquet",
                                                               "file:///t/m.parquet", "é.parquet"]


@pytest.mark.parametrize("expire", [False, True])
def test_record_shapes(engine, tmp_path, expire):
    """Every live, tombstone, expired and never-seen path and their one-byte neighbours, at cutoff -1
    and at the generator's cutoff (inside the deletionTimestamp window: about half the churn
    tombstones and the remove without a timestamp are expired there, and answer ABSENT)."""
    lp, _, exp = _shapes_table(str(tmp_path))
    cutoff = exp.min_file_retention_timestamp if expire else -1
    queries = _shape_queries(engine, lp)
    ref = _replay(engine, lp, cutoff)
    st = _replay(engine, lp, cutoff)
    try:
        emap = _expect_map(ref)
        n_all = len(set(_key(p.encode("utf-8")) for p in _all_paths(engine, lp)))
        assert (len(emap) < n_all) == expire and st.counts["num_removes"] > 10  # some expired, some kept
        hit, row = _check(st, queries, emap, "shapes")
        assert {ABSENT, LIVE, TOMB} == set(int(h) for h in hit)
        by = {q: (int(h), int(r)) for q, h, r in zip(queries, hit, row) if isinstance(q, str)}
        assert len({by[s] for s in SPELLINGS}) == 1 and by[SPELLINGS[0]][0] == LIVE
        assert by["file:///t/k.parquet"] == by["file:/t/k.parquet"] and by["file:/t/k.parquet"][0] == LIVE
        assert by["file:/t/m.parquet"] == by["file:///t/m.parquet"] and by["file:/t/m.parquet"][0] == LIVE
        assert by["é.parquet"][0] == LIVE
        gone = st.lookup_paths(["gone1.parquet", "gone2.parquet"])[0]
        assert [int(x) for x in gone] == [TOMB, ABSENT if expire else TOMB]
        # the hits' rows are the records asked for
        for side in (0, 1):
            at = [i for i in range(len(queries)) if hit[i] == side + 1]
            recs = st.export_rows_records(side, [int(row[i]) for i in at])
            qs = [queries[i].encode("utf-8") if isinstance(queries[i], str) else queries[i] for i in at]
            assert [_key(r["path"].encode("utf-8")) for r in recs] == [_key(q) for q in qs]
            assert all(r["path"] == O.canonicalize_path(r["path"]) for r in recs)
    finally:
        st.release()
        ref.release()


@pytest.mark.parametrize("bits", [4, 1])
def test_key_collisions_change_no_answer(engine, tmp_path, request, bits):
    """With the index keeping 4 bits, then 1 bit, of every key (context option lookup_key_bits) the
    survivors share 16 keys, then one: every probe walks a run of many equal keys and finds its path
    by the byte comparison alone. Same answers as with 64 bits. (The homes of such keys are the first
    slots of a table of 2,048, so these runs do not wrap past its last slot: DESIGN.md §4i.)"""
    lp, _, _ = _shapes_table(str(tmp_path))
    queries = _shape_queries(engine, lp)
    ref = _replay(engine, lp, -1)
    full = ref.lookup_paths(queries)
    emap = _expect_map(ref)
    request.addfinalizer(lambda: engine.set_option("lookup_key_bits", 64))
    assert engine.set_option("lookup_key_bits", bits) == 64
    st = _replay(engine, lp, -1)
    try:
        hit, row = _check(st, queries, emap, "bits=%d" % bits)
        assert np.array_equal(hit, full[0]) and np.array_equal(row, full[1])
        # the option is read at index build time: the first state's index keeps its 64 bits
        again = ref.lookup_paths(queries)
        assert np.array_equal(again[0], full[0]) and np.array_equal(again[1], full[1])
    finally:
        st.release()
        ref.release()
    from delta_amd.delta_log import DeltaError
    for bad in (0, 65, -1):
        with pytest.raises(DeltaError) as ei:
            engine.set_option("lookup_key_bits", bad)
        assert ei.value.code == "DR_E_INVALID_ARG"
    assert engine.get_option("lookup_key_bits") == bits


def _lookup_then_export(st, seed, what):
    """Lookups on a state nothing was exported from, checked against its own exports taken after."""
    counts = st.counts
    n = (counts["num_files"], counts["num_removes"])
    # positions first: a prefix of each side fetched by row, not by whole export
    some = [r["path"] for side in (0, 1) for r in st.export_rows_records(side, range(min(n[side], 50)))]
    before = st.lookup_paths(_variants(some, seed))
    emap = _expect_map(st)
    assert len(emap) == n[0] + n[1]
    allp = [r["path"] for side in (0, 1) for r in st.export(side)]
    _check(st, _variants(allp, seed + 1), emap, what)
    after = _check(st, _variants(some, seed), emap, what + " (first queries again)")
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    return emap


def test_commit_only_state(engine, tmp_path):
    """A JSON-only log: every path lies in the staged JSON buffer."""
    from delta_amd.testing import synth as S
    exp = S.build_config(1, str(tmp_path), scale=0.05)
    st = _replay(engine, os.path.join(str(tmp_path), "_delta_log"), exp.min_file_retention_timestamp)
    try:
        assert len(_lookup_then_export(st, 11, "json")) == exp.num_files > 64
    finally:
        st.release()


def test_checkpoint_only_state(engine, tmp_path):
    """A checkpoint and no commit after it: every path lies in the decompressed page arena."""
    from delta_amd.testing import synth as S
    spec = S.ChurnSpec(ckpt_files=700, ckpt_version=3, n_deltas=0, removes_per_delta=0, adds_per_delta=0, readd_frac=0.0)
    exp = S.build_table(str(tmp_path), spec, seed=2, row_group_size=300)
    st = _replay(engine, os.path.join(str(tmp_path), "_delta_log"), exp.min_file_retention_timestamp)
    try:
        assert len(_lookup_then_export(st, 12, "checkpoint")) == 700
    finally:
        st.release()


def test_apply_chain_states_answer_as_of_their_own_version(engine, tmp_path):
    """A base and two applied tails that add, remove and re-add known paths. The head is asked first;
    then the middle state, after the head exists, answers as of its own version; then the base."""
    from delta_amd import _native as N
    from delta_amd.testing import synth as S
    lp, v, _ = _shapes_table(str(tmp_path))
    base = _replay(engine, lp, -1)
    add = '{"add":{"path":"%s","partitionValues":{"p0":"2020-01-01","p1":"7"},"size":3,"modificationTime":%d,"dataChange":true}}\n'
    t1 = (add % ("t.parquet", S.T0 + 99) + '{"remove":{"path":"a.parquet","deletionTimestamp":5}}\n'
          '{"remove":{"path":"/abs/x.parquet/"}}\n')
    t2 = (add % ("a.parquet", S.T0 + 100) + '{"remove":{"path":"t.parquet","deletionTimestamp":6}}\n' +
          add % ("file:///abs/x.parquet", S.T0 + 101) + add % ("/abs/y.parquet", S.T0 + 102))
    states = [base]
    try:
        for k, text in enumerate((t1, t2)):
            tail = engine.stage_files([(v + 1 + k, N.DR_FILE_JSON, 0, text.encode("utf-8"))])
            try:
                states.append(states[-1].apply(tail, -1))
            finally:
                tail.release()
        known = ["a.parquet", "t.parquet", "/abs//x.parquet", "/abs/y.parquet", "m1.parquet"]
        want = {2: [LIVE, TOMB, LIVE, LIVE, LIVE], 1: [TOMB, LIVE, TOMB, ABSENT, LIVE], 0: [LIVE, ABSENT, LIVE, ABSENT, LIVE]}
        for g in (2, 1, 0):
            assert [int(h) for h in states[g].lookup_paths(known)[0]] == want[g], g
        for g in (2, 1, 0):
            _lookup_then_export(states[g], 20 + g, "chain state %d" % g)
    finally:
        for st in reversed(states):
            st.release()


def test_materialized_state_and_positions_of_a_filter(engine, tmp_path):
    """The same answers before and after export / filter / materialize on one state, and the rows of
    a dr_filter selection, looked up by path, are the selection itself."""
    from delta_amd.predicates import build_program, partition_schema
    lp, _, exp = _shapes_table(str(tmp_path))
    cutoff = exp.min_file_retention_timestamp
    ref = _replay(engine, lp, cutoff)
    st = _replay(engine, lp, cutoff)
    try:
        emap = _expect_map(ref)
        queries = _shape_queries(engine, lp)
        first = _check(st, queries, emap, "fresh")
        live = st.export(0)
        metadata = next(a["metaData"] for a in st.nonfile if "metaData" in a)
        sel = st.filter(build_program(partition_schema(metadata), [("<", F.C("p1"), F.L("integer", 40))]))
        assert 0 < len(sel) < len(live)
        hit, row = st.lookup_paths([live[i]["path"] for i in sel])
        assert set(int(h) for h in hit) == {LIVE} and [int(r) for r in row] == list(sel)
        assert st.materialize() > 0
        for what in ("after export, filter and materialize", "again"):
            got = _check(st, queries, emap, what)
            assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1])
    finally:
        st.release()
        ref.release()


def test_many_queries_cross_a_batch_and_many_workgroups(engine, tmp_path):
    """60,000 checkpoint rows and 30 churn commits (more than 50,000 survivors, an index of 2^17
    slots or more) and 300,000 queries -- more than one staging batch of 2^18 paths, about 1,200
    workgroups -- half of them present (with repeats), half absent, in random order."""
    from delta_amd.testing import synth as S
    exp = S.build_config(3, str(tmp_path), scale=0.006)
    st = _replay(engine, os.path.join(str(tmp_path), "_delta_log"), exp.min_file_retention_timestamp)
    try:
        emap, paths = {}, []
        for side in (0, 1):
            cols = st.export_columns(side)
            off, data = cols["path_off"], cols["path_bytes"].tobytes()
            for pos in range(len(off) - 1):
                p = data[off[pos]:off[pos + 1]]
                emap[_key(p)] = (side + 1, pos)
                paths.append(p)
        assert len(emap) == len(paths) == exp.num_files + exp.num_removes >= 50000 and exp.num_removes > 1000
        rng = np.random.default_rng(8)
        nq = 300000
        pick = rng.integers(0, len(paths), size=nq)
        absent = rng.random(nq) < 0.5
        queries = [paths[int(i)] + b"x" if a else paths[int(i)] for i, a in zip(pick, absent)]
        hit, row = st.lookup_paths(queries)
        want = [(ABSENT, -1) if a else emap[_key(paths[int(i)])] for i, a in zip(pick, absent)]
        assert not any(_key(q) in emap for q, a in zip(queries[:2000], absent[:2000]) if a)
        assert [int(h) for h in hit] == [w[0] for w in want]
        assert [int(r) for r in row] == [w[1] for w in want]
        assert 0.45 < float(np.mean(hit != 0)) < 0.55 and int((hit == TOMB).sum()) > 0
    finally:
        st.release()


def test_refusals_name_the_index_and_leave_the_state_usable(engine, tmp_path):
    from delta_amd import _native as N
    lp, _, _ = _shapes_table(str(tmp_path))
    st = _replay(engine, lp, -1)
    lib = engine.lib
    try:
        emap = _expect_map(st)
        probe = ["a.parquet", "gone1.parquet", "nope", "/abs/x.parquet"]

        def usable():
            hit, _ = _check(st, probe, emap, "after a refusal")
            assert [int(h) for h in hit] == [LIVE, TOMB, ABSENT, LIVE]

        blob = np.frombuffer(b"a.parquetnope", dtype=np.uint8)
        hit = np.full(4, 77, dtype=np.uint8)
        row = np.full(4, 77, dtype=np.int64)

        def call(off, n, flags=0, b=blob, h=hit, r=row):
            off = None if off is None else np.asarray(off, dtype=np.int64)
            rc = lib.dr_state_lookup_paths(st.h, None if b is None else b.ctypes.data, None if off is None else off.ctypes.data,
                                           n, flags, None if h is None else h.ctypes.data, None if r is None else r.ctypes.data)
            return rc, lib.dr_state_last_error(st.h).decode()

        good = [0, 9, 13]
        cases = [
            (dict(off=good, n=2, flags=1), "flags"),
            (dict(off=good, n=-1), "npaths = -1"),
            (dict(off=good, n=2, b=None), "path_bytes is NULL at index 0"),
            (dict(off=None, n=2), "path_off is NULL at index 0"),
            (dict(off=good, n=2, h=None), "hit is NULL at index 0"),
            (dict(off=good, n=2, r=None), "row is NULL at index 0"),
            (dict(off=[-1, 9, 13], n=2), "path_off[0] = -1"),
            (dict(off=[0, 5, 3, 13], n=3), "path_off[2] = 3"),
            # the offsets are refused on the host: the 2^31 bytes they claim are never read
            (dict(off=[0, 9, 9 + (1 << 31)], n=2), "path 1 holds 2147483648 bytes"),
        ]
        for kw, text in cases:
            rc, msg = call(**kw)
            assert rc == 1 and text in msg, (kw, rc, msg)  # DR_E_INVALID_ARG
            assert set(hit) == {77} and set(row) == {77}  # nothing written
            usable()
        for kw in (dict(off=None, n=0, b=None, h=None, r=None), dict(off=good, n=0)):
            rc, msg = call(**kw)
            assert rc == N.DR_OK and set(hit) == {77}, msg
        rc, msg = call(off=good, n=2)
        assert rc == N.DR_OK and list(hit[:2]) == [LIVE, ABSENT] and list(hit[2:]) == [77, 77], msg
        assert row[0] == emap[_key(b"a.parquet")][1] and row[1] == -1
        usable()
    finally:
        st.release()


def test_a_sharded_state_is_refused(tmp_path):
    """A rank of a sharded replay holds source-side survivors: DR_E_UNSUPPORTED with a message, on
    every rank (the loopback communicator, W = 2 as threads of this process)."""
    from delta_amd.delta_log import DeltaError, Engine
    from delta_amd.sharded import stage_shard
    from delta_amd.testing import synth as S
    exp = S.build_table(str(tmp_path), S.config_spec(3, 0.003), seed=5, row_group_size=4000)
    lp = os.path.join(str(tmp_path), "_delta_log")
    world = 2
    uid = Engine.comm_loopback_id()
    res, err = [None] * world, [None] * world

    def body(r):
        try:
            eng = Engine.get(0)
            comm = eng.comm(uid, world, r)
            try:
                staged = stage_shard(eng, lp, world, r)
                try:
                    st = comm.replay_sharded(staged, exp.min_file_retention_timestamp, True)
                finally:
                    staged.release()
                try:
                    with pytest.raises(DeltaError) as ei:
                        st.lookup_paths(["a.parquet"])
                    res[r] = (ei.value.code, str(ei.value), st.counts["num_files"])
                finally:
                    st.release()
            finally:
                comm.release()
        except BaseException as e:  # noqa: BLE001
            err[r] = e

    th = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in th), "a loopback rank hung"
    for e in err:
        if e is not None:
            raise e
    for code, msg, files in res:
        assert code == "DR_E_UNSUPPORTED" and "sharded" in msg and files == exp.num_files


def test_snapshot_files_by_path_touched_files_unreferenced(tmp_path, monkeypatch):
    from delta_amd.delta_log import DeltaError, DeltaLog, ManualClock, State
    root = str(tmp_path)
    _, _, exp = _shapes_table(root)
    DeltaLog.clear_cache()
    # tombstone retention one week: the snapshot's cutoff is the generator's
    snap = DeltaLog.for_table(root, clock=ManualClock(exp.min_file_retention_timestamp + 604800000)).snapshot
    assert snap.min_file_retention_timestamp == exp.min_file_retention_timestamp
    ref = _replay(snap.delta_log.engine, snap.delta_log.log_path, snap.min_file_retention_timestamp)
    try:
        live, tomb = ref.export(0), ref.export(1)
    finally:
        ref.release()
    by_key = {_key(f["path"].encode("utf-8")): f for f in live}
    queries = ([f["path"] for f in live[::7]] + [t["path"] for t in tomb[:20]] + SPELLINGS +
               ["nope.parquet", "file:///t/k.parquet", "é.parquet", "", "gone2.parquet"])
    want = [by_key.get(_key(q.encode("utf-8"))) for q in queries]
    assert sum(w is None for w in want) >= 22 and sum(w is not None for w in want) > 80

    with monkeypatch.context() as m:
        def refuse(self, which):
            raise AssertionError("the whole side was fetched")
        m.setattr(State, "export", refuse)
        assert snap.files_by_path(queries) == want
        assert snap.files_by_path([]) == [] and snap.files_by_path(["nope"]) == [None]
        assert snap._all is None
        # getTouchedFile: names under the table's data path are relativised, others pass through
        rel = [f["path"] for f in live if not f["path"].startswith("file:")][:30]
        named = [os.path.join(snap.delta_log.data_path, p) for p in rel] + ["/abs//x.parquet", "a.parquet"]
        assert snap.touched_files(named) == [by_key[_key(p.encode("utf-8"))] for p in rel + ["/abs//x.parquet", "a.parquet"]]
        for missing in (tomb[0]["path"], os.path.join(snap.delta_log.data_path, "nope.parquet"),
                        snap.delta_log.data_path + "x/a.parquet"):
            with pytest.raises(DeltaError) as ei:
                snap.touched_files(named[:3] + [missing, "also-missing"])
            assert ei.value.kind == "IllegalStateException"
            assert str(ei.value) == "File (%s) to be rewritten not found among candidate files" % missing
        # VACUUM's anti-join: what is neither live nor an unexpired tombstone
        listing = [f["path"] for f in live[:40]] + ["junk-1.parquet"] + [t["path"] for t in tomb] + ["gone2.parquet", "junk-2"]
        n = 40 + 1 + len(tomb)
        assert snap.unreferenced(listing) == [40, n, n + 1]
    assert len(snap.all_files) == len(live)
    assert snap.files_by_path(queries) == want  # indexed from the cached side
    DeltaLog.clear_cache()
