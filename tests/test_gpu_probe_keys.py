"""GPU parity of dr_state_probe_keys (k_probe.hip) against the brute-force evaluator of
tests/key_probe_ref.py: every field of the result over a table of 1 500 live files with steered statistics,
over states from JSON commits, from a checkpoint and after dr_state_apply; key counts around every capacity
constant of the kernel, selections around its workgroup and grid sizes, every supported type, the partition
source, both search variants, a cross-check against dr_filter, and the handle's and the refusals' rules."""
import ctypes as C
import os
import random
import threading

import numpy as np
import pytest

from delta_amd import _native as N
from delta_amd import predicates as P
from tests import key_probe_ref as R

pytestmark = pytest.mark.gpu
MODES = ("json", "checkpoint", "apply")
INVALID_ARG, UNSUPPORTED = 1, 12  # enum dr_status
TAB = N.PROBE_TAB  # the splitter table: up to TAB keys the segment length is 1, up to 2 * TAB it is 2, then 3
# 0, 1, 2, a wave +- 1; the table one below, at and one above (TAB + 1: the last segment holds a single key);
# the same where the segment length goes from 2 to 3 (2 * TAB + 1 = 3 * 2730 + 3: a last segment of 3; 2 * TAB + 2
# leaves a single key again)
KEY_COUNTS = (0, 1, 2, 63, 64, 65, TAB - 1, TAB, TAB + 1, 2 * TAB - 1, 2 * TAB, 2 * TAB + 1, 2 * TAB + 2)


@pytest.fixture(scope="module")
def engine():
    from delta_amd.delta_log import Engine
    return Engine.get(0)


def _state(engine, table_dir, mode):
    lp = R.build(table_dir, checkpoint=mode != "json")
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
    """Per mode: (state, the live files in export order)."""
    by_path = {f["path"]: f for f in R.live_files()}
    out = {}
    for m in MODES:
        st = _state(engine, str(tmp_path_factory.mktemp("probe_" + m)), m)
        live = [by_path[a["path"]] for a in st.export(0)]
        assert len(live) == R.N_LIVE == 1500
        out[m] = (st, live)
    yield out
    for st, _ in out.values():
        st.release()


_BOUNDS = {}


def stat_bounds(live, column, mode):
    """bounds[r] of the (minValues.column, maxValues.column) pair, computed once per mode and left unchanged."""
    if (mode, column) not in _BOUNDS:
        _BOUNDS[mode, column] = [(R.stat_word(f, R.MIN, column), R.stat_word(f, R.MAX, column)) for f in live]
    return _BOUNDS[mode, column]


def pair(column):
    typ = R.TYPES[column]
    return (R.MIN, (column,), typ), (R.MAX, (column,), typ)


def check(st, typ, lo, hi, bounds, keys, key_null=None, rows=None):
    """One probe: every field equals the evaluator's."""
    lo_stats, hi_stats = lo[0] != N.DR_SRC_PARTITION, hi[0] != N.DR_SRC_PARTITION
    want = R.evaluate(typ, bounds, lo_stats, hi_stats, keys, key_null, rows)
    got = st.probe_keys(lo, hi, keys, key_null, rows)
    assert got["selected"].tolist() == want[0]
    assert got["hits"].tolist() == want[1]
    assert got["unknown"] == want[2]
    assert got["key_files"].tolist() == want[3]
    return got


def shuffled(xs, seed):
    xs = list(xs)
    random.Random(seed).shuffle(xs)
    return xs


@pytest.mark.parametrize("count", KEY_COUNTS)
def test_key_counts_around_every_capacity_constant(states, count):
    """All 1 500 files against `count` distinct keys, unsorted: the steered ranges sit on the first and last
    entry of the table and of its segments at each count."""
    st, live = states["json"]
    lo, hi = pair("id")
    got = check(st, "long", lo, hi, stat_bounds(live, "id", "json"), shuffled(R.long_keys(count), count))
    assert got["unknown"] == 5  # a NULL min, a NULL max, no stats, JSON null... : the files without a bound
    if count >= 64:
        assert 0 < len(got["selected"]) < len(live) and got["hits"].max() == count and got["key_files"].min() >= 1


def test_key_counts_constants_are_the_kernels():
    """KEY_COUNTS brackets the table's capacity as kernels.h defines it (probe_seg: ceil(ndist / PROBE_TAB))."""
    seg = lambda d: 1 if d <= TAB else -(-d // TAB)  # noqa: E731
    assert [seg(c) for c in (TAB - 1, TAB, TAB + 1, 2 * TAB, 2 * TAB + 1, 2 * TAB + 2)] == [1, 1, 2, 2, 3, 3]
    assert (TAB + 1) % 2 == 1 and (2 * TAB + 2) % 3 == 1  # a last segment of a single key
    assert all(e in R.EDGES for e in (0, TAB - 1, TAB, TAB + 1, 2 * TAB - 1, 2 * TAB, 2 * TAB + 1))


def test_long_segments_over_the_whole_table(engine, states):
    """Every integer of [-2 100, 90 400) as a key, unsorted: 92 500 keys make segments of 23 keys behind a table
    of 4 022 entries whose last segment holds 17, so the second level bisects a real stretch of global memory
    and the `id` ranges, which lie all over that interval, start and end at every offset of a segment. With
    consecutive integers the count inside a range is a subtraction, which every file is checked against; the
    evaluator (files x keys) takes the first steered ranges and every 10th file."""
    st, live = states["json"]
    lo, hi = pair("id")
    bounds = stat_bounds(live, "id", "json")
    k0, k1 = -2100, 90400
    keys = shuffled(range(k0, k1), 21)
    seg = -(-len(keys) // TAB)
    assert seg == 23 and len(keys) - (-(-len(keys) // seg) - 1) * seg == 17
    rows = [r for r, f in enumerate(live) if int(f["path"][2:7]) < 14 or r % 10 == 0]
    assert 150 < len(rows) < 170
    check(st, "long", lo, hi, bounds, keys, rows=rows)
    got = st.probe_keys(lo, hi, keys)
    with engine.options(probe_search=1):
        plain = st.probe_keys(lo, hi, keys)
    assert all(np.array_equal(got[k], plain[k]) for k in ("selected", "hits", "key_files")) and got["unknown"] == plain["unknown"]
    want = [(r, -1 if a is None or b is None else max(0, min(b, k1 - 1) - max(a, k0) + 1)) for r, (a, b) in enumerate(bounds)]
    want = [(r, h) for r, h in want if h]
    assert got["selected"].tolist() == [r for r, _ in want] and got["hits"].tolist() == [h for _, h in want]
    assert got["hits"].max() == len(keys) and sum(h > seg for _, h in want) > len(want) // 2   # most ranges span segments
    files_of = dict(zip(keys, got["key_files"].tolist()))
    for k in (k0, k0 + 1, -1, 0, 1, 22, 23, 24, 40960 - 1, 40960, 81919, k1 - 18, k1 - 17, k1 - 2, k1 - 1):
        assert files_of[k] == sum(1 for a, b in bounds if a is not None and b is not None and a <= k <= b), k


@pytest.mark.parametrize("mode", MODES)
def test_every_mode_and_both_search_variants(engine, states, mode):
    st, live = states[mode]
    lo, hi = pair("id")
    bounds = stat_bounds(live, "id", mode)
    for count in (65, TAB + 1):
        keys = shuffled(R.long_keys(count), 3)
        a = check(st, "long", lo, hi, bounds, keys)
        with engine.options(probe_search=1):
            b = check(st, "long", lo, hi, bounds, keys)
        assert all(np.array_equal(a[k], b[k]) for k in ("selected", "hits", "key_files"))


def test_selections(engine, states):
    from delta_amd.predicates import build_program
    st, live = states["json"]
    lo, hi = pair("id")
    bounds = stat_bounds(live, "id", "json")
    keys = shuffled(R.long_keys(100), 1)
    rng = random.Random(7)
    n = len(live)
    block, sweep = N.PROBE_BLOCK, N.PROBE_BLOCK * N.PROBE_GRID   # one workgroup; one sweep of the strided grid
    selections = [[], [0], list(range(block - 1)), list(range(block)), list(range(block + 1)),
                  [rng.randrange(n) for _ in range(3000)],                        # shuffled, with repeats
                  st.filter(build_program({"p": "integer", "q": "double"}, [("=", ("col", "p"), ("lit", "integer", 1))]))]
    assert 100 < len(selections[-1]) < n
    for rows in selections:
        check(st, "long", lo, hi, bounds, keys, rows=rows)
    base = np.asarray([rng.randrange(n) for _ in range(sweep + 1)], dtype=np.int64)
    for size in (sweep - 1, sweep, sweep + 1):
        check(st, "long", lo, hi, bounds, keys, rows=base[:size])


def test_runs_of_lanes_at_one_counter(engine, states):
    """k_probe_files adds once per run of neighbouring lanes that share a `start` or an `end` counter: runs of
    one row that fill a wave, cross its edge and a workgroup's, are cut by a file without a hit, by an unknown
    one, by a change of the first key alone and of the last key alone, and a selection that ends inside a wave."""
    st, live = states["json"]
    lo, hi = pair("id")
    bounds = stat_bounds(live, "id", "json")
    top = R.KEY_STEP * 3 * TAB
    a, a_hi, a_top, b, b_top, none, unk = (bounds.index(x) for x in ((630, 630), (630, 635), (630, top), (20, 20), (20, top), (50, 40), (None, 5)))
    rows = [a] * 64 + [a] * 63 + [b] + [a] * 65 + [none] + [a] * 3 + [unk] + [a] * 2 + [b] * 2 + [a, none] * 40
    rows += [a, a_hi, a_hi, a_top, a_top, a, b_top, a_top, b_top, b_top, a_hi] * 7 + [a_top] * 130 + [b] + [unk] * 3 + [a] * 70 + [b_top] * 5
    assert len(rows) % 64 not in (0, 63) and len(rows) > 2 * N.PROBE_BLOCK
    keys = shuffled(R.long_keys(100), 8)
    for sel in (rows, rows[::-1], rows[:64], rows[:65], [a_top] * 64 + [a]):
        x = check(st, "long", lo, hi, bounds, keys, rows=sel)
        with engine.options(probe_search=1):
            y = check(st, "long", lo, hi, bounds, keys, rows=sel)
        assert np.array_equal(x["key_files"], y["key_files"])
    assert x["key_files"][keys.index(630)] == 65 and x["key_files"][keys.index(640)] == 64


def test_keys_unsorted_duplicated_and_null(states):
    st, live = states["json"]
    lo, hi = pair("id")
    bounds = stat_bounds(live, "id", "json")
    keys = shuffled(R.long_keys(300) * 2 + [R.I64_MIN, R.I64_MAX, -1, 5, 5, 5], 9)
    nulls = [1 if i % 7 == 0 else 0 for i in range(len(keys))]
    got = check(st, "long", lo, hi, bounds, keys, nulls)
    kf = got["key_files"].tolist()
    by_key = {}
    for k, z, c in zip(keys, nulls, kf):
        if z:
            assert c == 0
        else:
            assert by_key.setdefault(k, c) == c    # duplicated keys get the same count
    check(st, "long", lo, hi, bounds, keys, [1] * len(keys))          # every key NULL: only the unknown files
    got = check(st, "long", lo, hi, bounds, [])                          # no key at all
    assert got["hits"].tolist() == [-1] * got["unknown"] and got["unknown"] == len(got["selected"]) > 0
    check(st, "long", lo, hi, bounds, [], rows=[])


def _fp_words(typ, values):
    return [P.float_bits(v) if typ == "float" else R.signed64(P.double_bits(v)) for v in values]


@pytest.mark.parametrize("column", list(R.TYPES))
def test_every_supported_type(states, column):
    st, live = states["checkpoint"]
    typ = R.TYPES[column]
    lo, hi = pair(column)
    bounds = stat_bounds(live, column, "checkpoint")
    assert any(a is None for a, _ in bounds) and any(b is None for _, b in bounds) and any(a is not None and b is not None for a, b in bounds)
    rng = random.Random(5)
    known = [w for ab in bounds for w in ab if w is not None]
    keys = rng.sample(sorted(set(known)), 40)                      # keys that are some file's bound
    if typ in ("float", "double"):
        nan2 = 0x7fc00001 if typ == "float" else R.signed64(0xfff8000000000123)   # another NaN payload
        keys += _fp_words(typ, [float("nan"), -0.0, 0.0, float("inf"), float("-inf"), 0.125, -7.75, 1024.0]) + [nan2]
    else:
        keys += [k + d for k in keys[:10] for d in (-1, 1)] + [0, -1]
        keys += [R.I64_MIN, R.I64_MAX, R.I32_MAX + 1, R.I32_MIN - 1, 2 ** 40, 128, -129, 32768]   # outside the narrow kinds' ranges
    got = check(st, typ, lo, hi, bounds, shuffled(keys, 2))
    assert got["unknown"] > 0 and (got["hits"] > 0).any()
    # mixed sources of one type: a bound from maxValues on both sides
    check(st, typ, hi, hi, [(b, b) for _, b in bounds], keys[:5])


@pytest.mark.parametrize("column,typ", [("p", "integer"), ("q", "double")])
def test_partition_source_is_a_semi_join(states, column, typ):
    st, live = states["apply"]

    def word(s):
        v = P.cast_partition_value(s, typ)
        return None if v is None else (v if typ == "integer" else R.signed64(P.double_bits(v)))
    bounds = [(word(f["partitionValues"][column]),) * 2 for f in live]
    assert any(b[0] is None for b in bounds)
    keys = [3, 3, -2, 99, 0] if typ == "integer" else _fp_words(typ, [0.0, float("nan"), 1.5, 7.0, float("-inf")])
    src = (N.DR_SRC_PARTITION, column, typ)
    got = check(st, typ, src, src, bounds, keys, rows=shuffled(range(len(live)), 4))
    assert got["unknown"] == 0 and set(got["hits"].tolist()) == {1}   # a NULL partition value joins nothing
    assert len(got["selected"]) < len(live)


def test_cross_check_against_dr_filter(states):
    """(min IS NULL OR max IS NULL) OR OR_k (min <= k AND max >= k) through dr_filter selects the same files:
    the probe's order and null rules are dr_filter's."""
    from delta_amd.predicates import build_program
    st, live = states["json"]
    for column, keys in (("id", [0, 630, 40960, -1, R.I64_MAX, 81930, 7, 20]), ("i", [R.I32_MIN, 0, 3, 977, R.I32_MAX]),
                         ("d", [float("nan"), -0.0, 2.5, float("inf"), -33.125, 1.0]), ("f", [0.0, float("nan"), -1.25, 3.5]),
                         ("dt", ["2019-04-14", "2019-06-01", "2020-01-01"])):
        typ = R.TYPES[column]
        mn, mx = ("stats", R.MIN, (column,), typ), ("stats", R.MAX, (column,), typ)
        pred = ("or", ("isnull", mn), ("isnull", mx))
        for k in keys:
            pred = ("or", pred, ("and", ("<=", mn, ("lit", typ, k)), (">=", mx, ("lit", typ, k))))
        want = st.filter(build_program({"p": "integer", "q": "double"}, [pred]))
        words = [P._lit(typ, k) for k in keys]
        words = [R.signed64(w) for w in words]
        lo, hi = pair(column)
        got = st.probe_keys(lo, hi, words)
        assert got["selected"].tolist() == want and 0 < len(want) < len(live), column


def test_repeatable_under_a_permutation_of_the_keys(states):
    st, live = states["json"]
    lo, hi = pair("id")
    keys = R.long_keys(TAB + 77) + [5, 5, -3]
    perm = shuffled(range(len(keys)), 12)
    a = st.probe_keys(lo, hi, keys)
    b = st.probe_keys(lo, hi, [keys[i] for i in perm])
    c = st.probe_keys(lo, hi, [keys[i] for i in perm])
    assert np.array_equal(a["selected"], b["selected"]) and np.array_equal(a["hits"], b["hits"]) and a["unknown"] == b["unknown"]
    assert a["key_files"][perm].tolist() == b["key_files"].tolist()
    assert all(np.array_equal(b[k], c[k]) for k in ("selected", "hits", "key_files"))


def _raw(engine, st, rows, nrows, lo, hi, keys, nkeys, flags=0, key_null=None, release=True):
    """dr_state_probe_keys as a C caller meets it: (status, message, handle, result)."""
    p64 = C.POINTER(C.c_int64)
    r = None if rows is None else (C.c_int64 * max(len(rows), 1))(*rows)
    k = None if keys is None else (C.c_int64 * max(len(keys), 1))(*keys)
    z = None if key_null is None else (C.c_uint8 * max(len(key_null), 1))(*key_null)
    handle, out = C.c_void_p(), N.dr_probe_result()
    with engine.lock:
        rc = engine.lib.dr_state_probe_keys(st.h, None if r is None else C.cast(r, p64), nrows, lo[0], lo[1], hi[0], hi[1],
                                            None if k is None else C.cast(k, p64), None if z is None else C.cast(z, C.POINTER(C.c_uint8)),
                                            nkeys, flags, C.byref(handle), C.byref(out))
        msg = engine.lib.dr_last_error(engine.ctx).decode("utf-8", "replace") if rc else ""
    if rc != 0:
        assert not handle.value and not out.selected and not out.key_files
    elif release:
        assert engine.lib.dr_probe_release(handle) == 0
        assert engine.lib.dr_probe_release(handle) == INVALID_ARG  # a second release is refused
    return rc, msg, handle, out


def test_refusals_leave_the_state_usable(engine, states):
    from delta_amd.predicates import build_program
    st, live = states["json"]
    n = len(live)
    src = lambda s, t: t | s << N.DR_SRC_SHIFT  # noqa: E731
    LO, HI = (b"id", src(1, 4)), (b"id", src(2, 4))
    P_ = "dr_state_probe_keys: "
    cases = [
        ((None, 0, LO, HI, [1], 1, 2), INVALID_ARG, P_ + "flags = 2, not 0"),
        (([0], -1, LO, HI, [1], 1), INVALID_ARG, P_ + "nrows = -1 is negative"),
        ((None, 0, LO, HI, [1], -1), INVALID_ARG, P_ + "nkeys = -1 is outside 0..2147483647"),
        ((None, 0, LO, HI, [1], 2 ** 31), INVALID_ARG, P_ + "nkeys = 2147483648 is outside 0..2147483647"),
        ((None, 0, LO, HI, None, 2), INVALID_ARG, P_ + "keys == NULL with nkeys = 2"),
        (([0, n - 1, n], 3, LO, HI, [1], 1), INVALID_ARG, P_ + "rows[2] = %d is outside [0, %d)" % (n, n)),
        (([0, -1, n], 3, LO, HI, [1], 1), INVALID_ARG, P_ + "rows[1] = -1 is outside [0, %d)" % n),
        ((None, 0, LO, (b"id", src(2, 3)), [1], 1), INVALID_ARG, P_ + "lo is of type 4 and hi of type 3; both bounds take one base type"),
        ((None, 0, (b"id", src(7, 4)), HI, [1], 1), INVALID_ARG, "predicate column lo: unknown source 7"),
        ((None, 0, LO, (b"a\x01\x01b", src(2, 4)), [1], 1), INVALID_ARG, "predicate column hi: segment 1 of the statistics path is empty"),
        ((None, 0, LO, (b"id", 12), [1], 1), INVALID_ARG, P_ + "hi has no valid column type (code 12)"),
        ((None, 0, (b"s", src(1, 0)), (b"s", src(2, 0)), [1], 1), UNSUPPORTED, P_ + "lo is of type 0"),
        ((None, 0, (b"x", src(1, 10)), (b"x", src(2, 10)), [1], 1), UNSUPPORTED, P_ + "lo is of type 10"),
        ((None, 0, (b"x", 11 | 10 << 8), (b"x", 11 | 10 << 8), [1], 1), UNSUPPORTED, P_ + "lo is of type 11"),
        ((None, 0, (b"p", 3), (b"x", 6), [1], 1), UNSUPPORTED, P_ + "hi is of type 6"),
    ]
    prog = build_program({"p": "integer", "q": "double"}, [("=", ("col", "p"), ("lit", "integer", 1))])
    want = st.filter(prog)
    for args, status, text in cases:
        rc, msg, _, _ = _raw(engine, st, *args)
        assert rc == status and text in msg, (args, msg)
        assert st.filter(prog) == want   # the state still answers
    assert _raw(engine, st, None, -5, LO, HI, None, 0)[0] == 0   # nrows is ignored with rows == NULL; keys may be NULL with none
    assert _raw(engine, st, [], 0, LO, HI, [4], 1)[0] == 0       # an empty selection


def test_result_outlives_the_state_and_the_context(tmp_path):
    from delta_amd.delta_log import Engine
    eng = Engine(0)  # a context of its own: destroyed below
    staged = eng.stage_log(R.build(str(tmp_path), checkpoint=False), -1)
    st = staged.replay(0)
    staged.release()
    keys = R.long_keys(70)
    rc, _, handle, res = _raw(eng, st, None, 0, (b"id", 4 | 1 << 24), (b"id", 4 | 2 << 24), keys, len(keys), release=False)
    assert rc == 0
    want = st.probe_keys(*pair("id"), keys)
    st.release()
    eng.lib.dr_ctx_destroy(eng.ctx)
    eng.ctx = None
    n = res.nselected
    assert n == len(want["selected"]) > 5 and res.nkeys == len(keys) and res.unknown == want["unknown"]
    assert [res.selected[i] for i in range(n)] == want["selected"].tolist()
    assert [res.hits[i] for i in range(n)] == want["hits"].tolist()
    assert [res.key_files[i] for i in range(res.nkeys)] == want["key_files"].tolist()
    assert eng.lib.dr_probe_release(handle) == 0
    assert eng.lib.dr_probe_release(handle) == INVALID_ARG  # a second release is refused
    assert eng.lib.dr_probe_release(None) == 0


def test_a_sharded_state_is_refused(tmp_path):
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
                        st.probe_keys((R.MIN, ("id",), "long"), (R.MAX, ("id",), "long"), [1, 2])
                    res[r] = (ei.value.code, str(ei.value))
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
    for code, msg in res:
        assert code == "DR_E_UNSUPPORTED" and "dr_state_probe_keys: a sharded state" in msg and "mislead" in msg


@pytest.mark.parametrize("checkpoint", [False, True])
def test_files_for_keys_end_to_end(tmp_path, checkpoint):
    from delta_amd.delta_log import DeltaLog
    R.build(str(tmp_path), checkpoint=checkpoint)
    DeltaLog.clear_cache()
    snap = DeltaLog.for_table(str(tmp_path)).snapshot
    try:
        live = snap.all_files
        by_path = {f["path"]: f for f in R.live_files()}
        live = [by_path[a["path"]] for a in live]
        flt = [("in", ("col", "p"), [("lit", "integer", 1), ("lit", "integer", 4)])]
        kept = [r for r, f in enumerate(live) if f["partitionValues"]["p"] in ("1", "4")]
        # a statistics column, without and with filters
        keys = [0, 630, None, 40960, 630, -77, 2 ** 70]
        words, nulls = [0, 630, 0, 40960, 630, -77, 0], [0, 0, 1, 0, 0, 0, 1]
        bounds = [(R.stat_word(f, R.MIN, "id"), R.stat_word(f, R.MAX, "id")) for f in live]
        for filters, rows in (((), None), (flt, kept)):
            want = R.evaluate("long", bounds, True, True, words, nulls, rows)
            files, key_files = snap.files_for_keys("ID", keys, filters=filters)
            assert [f["path"] for f in files] == [live[r]["path"] for r in want[0]] and len(files) > want[2] > 0
            assert key_files.tolist() == want[3] and key_files[1] == key_files[4] > 0
        # a partition column, without and with filters
        pb = [(P.cast_partition_value(f["partitionValues"]["p"], "integer"),) * 2 for f in live]
        for filters, rows in (((), None), (flt, kept)):
            want = R.evaluate("integer", pb, False, False, [4, -2, 77], None, rows)
            files, key_files = snap.files_for_keys("p", [4, -2, 77], filters=filters)
            assert [f["path"] for f in files] == [live[r]["path"] for r in want[0]] and want[2] == 0
            assert key_files.tolist() == want[3] and key_files[2] == 0 < key_files[0]
        # a type the probe does not take: every file of the filter selection, no counts
        files, key_files = snap.files_for_keys("s", ["a7"], filters=flt)
        assert key_files is None and [f["path"] for f in files] == [live[r]["path"] for r in kept]
    finally:
        snap.release()
        DeltaLog.clear_cache()
