"""GPU parity of dr_state_aggregate (k_agg.hip) and of the layers over it -- State.aggregate,
Snapshot.scan_sizes, Snapshot.aggregate_from_metadata -- against a plain-Python fold over exported records
(tests/agg_expect.py) on the corpus of tests/filter_stats_corpus.py, replayed from JSON, from a checkpoint
and through dr_state_apply: every (fn, source, type) cell, selections cut at the wave and tile sizes,
group layouts with empty, single-row and tile-spanning groups, ties and the float order, the 128-bit sum,
determinism, the refusals, and the same cells on the bounds build."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from delta_amd import _native as N
from tests import agg_expect as E
from tests import filter_stats_corpus as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("json", "checkpoint", "apply")
INVALID_ARG, UNSUPPORTED = 1, 12  # enum dr_status
T = N.AGG_TILE
INT_KINDS = ("byte", "short", "integer", "long")


@pytest.fixture(scope="module")
def engine():
    from delta_amd.delta_log import Engine
    return Engine.get(0)


def _state(engine, table_dir, mode):
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
    """Per mode: the state and its live records in export order (the corpus's own dicts), computed once."""
    by_path = {f["path"]: f for f in F.live_files()}
    out = {}
    for m in MODES:
        st = _state(engine, str(tmp_path_factory.mktemp("agg_" + m)), m)
        live = [by_path[a["path"]] for a in st.export(0)]
        assert len(live) == F.N_LIVE
        out[m] = (st, live)
    yield out
    for st, _ in out.values():
        st.release()


def all_cells():
    """Every (fn, input) the ABI admits over the corpus: (agg_spec form, fn, getter, is a statistics column)."""
    cells = []
    for path, typ in F.DTYPES.items():
        for src in (F.MIN, F.MAX):
            tail, get = E.stats_input(src, path, typ)
            fns = ("min", "max", "count") + (("sum",) if typ in INT_KINDS else ())
            cells += [((fn,) + tail, fn, get, True) for fn in fns]
        tail, get = E.stats_input(F.NULLCOUNT, path, "long")
        cells += [((fn,) + tail, fn, get, True) for fn in ("min", "max", "count", "sum")]
    tail, get = E.stats_input(F.NUMRECORDS, (), "long")
    cells += [((fn,) + tail, fn, get, True) for fn in ("min", "max", "count", "sum")]
    tail, get = E.partition_input()
    cells += [((fn,) + tail, fn, get, False) for fn in ("min", "max", "count", "sum")]
    for which in ("size", "mtime"):
        tail, get = E.builtin_input(which)
        cells += [((fn,) + tail, fn, get, False) for fn in ("min", "max", "count", "sum")]
    return cells


def check(st, live, cells, rows=None, off=None, what=""):
    """One State.aggregate call per 16 cells against the fold; returns the results."""
    out = []
    for k in range(0, len(cells), N.DR_AGG_MAX_SPECS):
        batch = cells[k:k + N.DR_AGG_MAX_SPECS]
        res = st.aggregate([c[0] for c in batch], rows, off)
        n = len(live) if rows is None else len(rows)
        o = [0, n] if off is None else list(off)
        assert [int(x) for x in res["group_rows"]] == [o[g + 1] - o[g] for g in range(len(o) - 1)], what
        for a, c in enumerate(batch):
            E.compare(res, a, E.fold(c[1], c[2], live, rows, off), (what, c[0]))
        out.append(res)
    return out


# a spec of every combine class and input width, for the layout tests
def mixed_cells():
    pick = [("sum", F.NUMRECORDS, (), "long"), ("min", F.MIN, ("id",), "long"), ("max", F.MAX, ("s",), "string"),
            ("max", F.MAX, ("d",), "double"), ("min", F.MIN, ("dec",), "decimal(12,2)"), ("count", F.NULLCOUNT, ("s",), "long"),
            ("min", F.MIN, ("f",), "float"), ("max", F.MIN, ("b",), "byte"), ("min", F.MIN, ("n", "y", "z"), "string"),
            ("sum", "size"), ("max", "mtime"), ("max", N.DR_SRC_PARTITION, "p", "integer")]
    by_spec = {c[0]: c for c in all_cells()}
    return [by_spec[p] for p in pick]


def test_library_has_aggregate(engine, states):
    """Fails on a library without the feature: the symbols are there and one call answers."""
    assert N.has_aggregate(engine.lib)
    st, live = states["json"]
    res = st.aggregate([("count", "size"), ("sum", "size")])
    assert int(res["group_rows"][0]) == F.N_LIVE == int(res["nonnull"][0, 0])
    assert int(res["value_lo"][1, 0]) == sum(f["size"] for f in live) and int(res["value_hi"][1, 0]) == 0
    empty = st.aggregate([])  # naggs == 0: group_rows only
    assert [int(x) for x in empty["group_rows"]] == [F.N_LIVE] and empty["nonnull"].shape == (0, 1)


@pytest.mark.parametrize("mode", MODES)
def test_every_cell_one_group_all_live(states, mode):
    st, live = states[mode]
    cells = all_cells()
    assert len(cells) > 150
    for spec, fn, get, is_stats in cells:
        if is_stats:  # each statistics column holds NULL and non-NULL inputs
            vals = [get(f) for f in live]
            assert any(v is None for v in vals) and any(v is not None for v in vals), spec
    check(st, live, cells, what=mode)


def test_cut_points(states):
    """Selections drawn with repeats, unsorted, of every length around the wave, the workgroup and the tile."""
    st, live = states["checkpoint"]
    rng = np.random.RandomState(20260101)
    cells = mixed_cells()
    for n in (0, 1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 5):
        rows = [int(x) for x in rng.randint(0, len(live), size=n)]
        check(st, live, cells, rows, None, what="n=%d" % n)
        if n:
            check(st, live, cells[:4], sorted(rows, reverse=True), None, what="descending n=%d" % n)


def test_group_layouts(states):
    st, live = states["json"]
    rng = np.random.RandomState(7)
    cells = mixed_cells()
    draw = lambda n: [int(x) for x in rng.randint(0, len(live), size=n)]  # noqa: E731
    null_id = [i for i, f in enumerate(live) if F.typed(f["stats"], F.MIN, ("id",), "long") is None]
    assert len(null_id) > 20
    layouts = {
        # empty groups at the start, in the middle and at the end; boundaries at T - 1, T and T + 1
        "empty+tile": (draw(2 * T + 100), [0, 0, 0, 5, 5, 300, 300, T - 1, T, T + 1, 2 * T + 100, 2 * T + 100, 2 * T + 100]),
        # single-row groups across a whole tile and into the next: ngroups == nrows
        "singles": (draw(T + 7), list(range(T + 8))),
        # one group over three tiles between two small ones (the last one crosses a tile as well)
        "span3": (draw(3 * T + 5), [0, 3, 2 * T + 500, 3 * T + 5]),
        # groups that end exactly with their tile, one per tile, and one of two tiles
        "aligned": (draw(4 * T), [0, T, 2 * T, 4 * T]),
        # a group whose min(id) inputs are all NULL, between two that have values, and one at a tile's edge
        "allnull": (draw(T - 10) + null_id[:20] + draw(30) + null_id[:3], [0, T - 10, T + 10, T + 40, T + 43]),
        "one-row": ([5], [0, 1]),
        "no-rows-groups": ([], [0, 0, 0]),
    }
    for name, (rows, off) in layouts.items():
        res = check(st, live, cells, rows, off, what=name)
        if name == "allnull":
            assert int(res[0]["nonnull"][1][1]) == 0 and int(res[0]["arg_row"][1][1]) == -1 and int(res[0]["group_rows"][1]) == 20
    # rows == None with groups over all live files
    check(st, live, cells, None, [0, 100, 100, F.N_LIVE], what="all live, grouped")
    # dr_state_partition_groups' pair straight through, of all live files and of a selection with repeats
    for sel in (None, draw(2 * T + 3)):
        order, off = st.partition_group_offsets(sel)
        assert len(off) - 1 == 5 and off[-1] == (F.N_LIVE if sel is None else len(sel))
        check(st, live, cells, order, off, what="partition_groups")


def test_ties_go_to_the_earliest_position(states):
    """Two files with the same minValues.id on both sides of a wave boundary and of a tile boundary."""
    st, live = states["apply"]
    ids = [F.typed(f["stats"], F.MIN, ("id",), "long") for f in live]
    lowest = min(t[0] for t in ids if t is not None and t[0] > -10 ** 6)
    twins = [i for i, t in enumerate(ids) if t is not None and t[0] == lowest]
    filler = [i for i, t in enumerate(ids) if t is not None and t[0] > lowest]
    assert len(twins) >= 2 and len(filler) > 50
    a, b = twins[0], twins[1]
    cell = [c for c in all_cells() if c[0] == ("min", F.MIN, ("id",), "long")]
    for at in (63, 64, 255, 256, T - 1, T, 2 * T):
        for first, second in ((a, b), (b, a)):
            rows = [filler[k % len(filler)] for k in range(2 * T + 50)]
            rows[at - 1], rows[at] = first, second
            rows[at + 7] = first  # and once more, later
            sel = [r for r in rows if ids[r][0] >= lowest]
            res = check(st, live, cell, sel, None, what="tie at %d" % at)[0]
            assert int(res["arg_row"][0][0]) == first and int(res["value_lo"][0][0]) == lowest


def test_float_order_and_own_bits(engine, tmp_path):
    """-0.0 = 0.0 (the earlier one wins, with its own bits), NaN above +Infinity and equal to itself: a table
    of three commits whose minValues hold the values (the corpus has no NaN beside an infinity in one column)."""
    log = os.path.join(str(tmp_path), "_delta_log")
    os.makedirs(log)
    vals = [-0.0, 0.0, "NaN", "Infinity", 1.5, -3.0, "NaN", "-Infinity"]
    for v in range(3):
        with open(os.path.join(log, "%020d.json" % v), "w") as f:
            if v == 0:
                f.write(json.dumps({"protocol": F.PROTOCOL}) + "\n" + json.dumps({"metaData": F.METADATA}) + "\n")
            for i in range(3 * v, min(3 * v + 3, len(vals))):
                stats = {"numRecords": 1, "minValues": {"d": vals[i], "f": vals[i]}}
                f.write(json.dumps({"add": {"path": "z-%d" % i, "partitionValues": {"p": "0"}, "size": 1, "modificationTime": 1,
                                            "dataChange": True, "stats": json.dumps(stats)}}) + "\n")
    staged = engine.stage_log(log)
    st = staged.replay(0)
    staged.release()
    try:
        recs = st.export(0)
        live = [{"stats": a["stats"], "partitionValues": a["partitionValues"], "size": a["size"], "modificationTime": a["modificationTime"]}
                for a in recs]
        at = {int(a["path"][2:]): i for i, a in enumerate(recs)}  # value index -> live row
        assert len(at) == len(vals)
        neg0, pos0, nan, inf, nan2, ninf = at[0], at[1], at[2], at[3], at[6], at[7]
        for typ, zero_bits in (("double", -2 ** 63), ("float", 0x80000000)):
            tail, get = E.stats_input(F.MIN, (typ[0],), typ)
            mn, mx = (("min",) + tail, "min", get, True), (("max",) + tail, "max", get, True)
            assert get(live[neg0])[1] == zero_bits and get(live[pos0])[1] == 0
            for first, second, bits in ((neg0, pos0, zero_bits), (pos0, neg0, 0)):
                res = check(st, live, [mn, mx], [at[4], first, second, nan, first], None, what="zeros are the minimum")[0]
                assert (int(res["arg_row"][0][0]), int(res["value_lo"][0][0])) == (first, bits)
                res = check(st, live, [mn, mx], [at[5], ninf, first, second, first], None, what="zeros are the maximum")[0]
                assert (int(res["arg_row"][1][0]), int(res["value_lo"][1][0])) == (first, bits)
            # NaN above +Infinity, equal to itself (the earlier one), never the minimum beside a number
            for a, b in ((nan, nan2), (nan2, nan)):
                res = check(st, live, [mn, mx], [inf, a, inf, b, at[4]], None, what="nan")[0]
                assert int(res["arg_row"][1][0]) == a and int(res["arg_row"][0][0]) == at[4]
            res = check(st, live, [mn, mx], [nan, nan2], None, what="only nan")[0]
            assert int(res["arg_row"][0][0]) == nan == int(res["arg_row"][1][0])
            check(st, live, [mn, mx], None, [0, 3, 3, len(vals)], what="all, grouped")
    finally:
        st.release()


def test_sum_carries_into_the_high_word(engine, tmp_path):
    log = os.path.join(str(tmp_path), "_delta_log")
    os.makedirs(log)
    counts = [2 ** 63 - 1, 2 ** 63 - 1, 5]
    with open(os.path.join(log, "%020d.json" % 0), "w") as f:
        f.write(json.dumps({"protocol": F.PROTOCOL}) + "\n" + json.dumps({"metaData": F.METADATA}) + "\n")
        for i, n in enumerate(counts):
            f.write(json.dumps({"add": {"path": "h-%d" % i, "partitionValues": {"p": "0"}, "size": 2 ** 62, "modificationTime": -1,
                                        "dataChange": True, "stats": json.dumps({"numRecords": n})}}) + "\n")
    staged = engine.stage_log(log)
    st = staged.replay(0)
    staged.release()
    try:
        res = st.aggregate([("sum", F.NUMRECORDS, (), "long"), ("sum", "size"), ("sum", "mtime")])
        total = sum(counts) % (1 << 128)
        assert (int(res["value_lo"][0, 0]), int(res["value_hi"][0, 0])) == (E.s64(total), E.s64(total >> 64)) == (3, 1)
        assert int(res["value_hi"][0, 0]) != int(res["value_lo"][0, 0]) >> 63  # how a host sees the overflow
        assert (int(res["value_lo"][1, 0]), int(res["value_hi"][1, 0])) == (E.s64(3 * 2 ** 62), 0)
        assert (int(res["value_lo"][2, 0]), int(res["value_hi"][2, 0])) == (-3, -1)
        # repeats count twice, and the carry survives many partial sums
        rows = [0, 1] * (T + 3)
        res = st.aggregate([("sum", F.NUMRECORDS, (), "long")], rows)
        total = (2 * (T + 3) * (2 ** 63 - 1)) % (1 << 128)
        assert (int(res["value_lo"][0, 0]), int(res["value_hi"][0, 0])) == (E.s64(total), E.s64(total >> 64))
    finally:
        st.release()


def test_determinism_and_split_groups(states):
    st, live = states["checkpoint"]
    rng = np.random.RandomState(99)
    rows = [int(x) for x in rng.randint(0, len(live), size=3 * T + 77)]
    specs = [("sum", F.NUMRECORDS, (), "long"), ("count", F.MIN, ("id",), "long"), ("min", F.MIN, ("id",), "long"),
             ("max", F.MAX, ("s",), "string"), ("sum", "size")]
    one = st.aggregate(specs, rows)
    again = st.aggregate(specs, rows)
    for k in ("group_rows", "nonnull", "value_lo", "value_hi", "arg_row"):
        assert np.array_equal(one[k], again[k]), k
    assert one["strings"] == again["strings"]
    for cut in (1, 64, T, T + 500, len(rows) - 1):
        two = st.aggregate(specs, rows, [0, cut, len(rows)])
        for a in (0, 1, 4):  # counts and sums add (128 bits)
            assert int(two["nonnull"][a].sum()) == int(one["nonnull"][a][0])
            total = sum((int(two["value_hi"][a][g]) << 64) + (int(two["value_lo"][a][g]) & E.M64) for g in (0, 1)) % (1 << 128)
            assert (E.s64(total), E.s64(total >> 64)) == (int(one["value_lo"][a][0]), int(one["value_hi"][a][0]))
        # min: the smaller value, the first group's on a tie
        g = 1 if int(two["nonnull"][2][0]) == 0 or (int(two["nonnull"][2][1]) and int(two["value_lo"][2][1]) < int(two["value_lo"][2][0])) else 0
        assert (int(two["value_lo"][2][g]), int(two["arg_row"][2][g])) == (int(one["value_lo"][2][0]), int(one["arg_row"][2][0]))
        # max over bytes: the larger value, the first group's on a tie
        s0, s1 = two["strings"][3]
        g = 1 if s0 is None or (s1 is not None and s1 > s0) else 0
        assert (two["strings"][3][g], int(two["arg_row"][3][g])) == (one["strings"][3][0], int(one["arg_row"][3][0]))


def _raw(engine, st, rows, nrows, off, ngroups, specs, naggs):
    """dr_state_aggregate as a C caller meets it: (status, message)."""
    p64 = C.POINTER(C.c_int64)
    r = None if rows is None else (C.c_int64 * max(len(rows), 1))(*rows)
    o = None if off is None else (C.c_int64 * max(len(off), 1))(*off)
    arr = None if specs is None else (N.dr_agg_spec * max(len(specs), 1))(*[N.dr_agg_spec(*s) for s in specs])
    handle, out = C.c_void_p(), N.dr_agg_result()
    with engine.lock:
        rc = engine.lib.dr_state_aggregate(st.h, None if r is None else C.cast(r, p64), nrows, None if o is None else C.cast(o, p64),
                                           ngroups, arr, naggs, C.byref(handle), C.byref(out))
        msg = engine.lib.dr_last_error(engine.ctx).decode("utf-8", "replace") if rc else ""
    if rc == 0:
        assert engine.lib.dr_agg_release(handle) == 0
        assert engine.lib.dr_agg_release(handle) == INVALID_ARG  # a second release is refused
    else:
        assert not handle.value and not out.group_rows
    return rc, msg


def test_refusals_leave_the_state_usable(engine, states):
    st, live = states["json"]
    n = F.N_LIVE
    src = lambda s, t: t | s << N.DR_SRC_SHIFT  # noqa: E731
    ok = (N.DR_AGG_COUNT, N.DR_AGG_IN_SIZE, b"", 0)
    col = lambda fn, name, t: (fn, N.DR_AGG_IN_COLUMN, name, t)  # noqa: E731
    cases = [
        ((None, 0, None, 0, None, 2), "aggs == NULL with naggs = 2"),
        ((None, 0, None, 0, [ok] * 17, 17), "naggs = 17 is outside 0..16"),
        ((None, 0, None, 0, [ok], -1), "naggs = -1 is outside 0..16"),
        (([0], -1, None, 0, [ok], 1), "nrows = -1 is negative"),
        ((None, 0, [0], -1, [ok], 1), "ngroups = -1 is negative"),
        (([0, n - 1, n], 3, None, 0, [ok], 1), "rows[2] = %d is outside [0, %d)" % (n, n)),
        (([0, -1], 2, None, 0, [ok], 1), "rows[1] = -1 is outside [0, %d)" % n),
        (([1, 2, 3], 3, [1, 3], 1, [ok], 1), "group_off[0] = 1, not 0"),
        (([1, 2, 3], 3, [0, 2, 1, 3], 3, [ok], 1), "group_off[2] = 1 is below group_off[1] = 2"),
        (([1, 2, 3], 3, [0, 2], 1, [ok], 1), "group_off[1] = 2, not the selection's 3 rows"),
        ((None, 0, [0, 5], 1, [ok], 1), "group_off[1] = 5, not the selection's %d rows" % n),
        ((None, 0, None, 0, [(7, N.DR_AGG_IN_SIZE, b"", 0)], 1), "aggregate spec 0: unknown fn 7"),
        ((None, 0, None, 0, [ok, (N.DR_AGG_SUM, 5, b"", 0)], 2), "aggregate spec 1: unknown input 5"),
        ((None, 0, None, 0, [(N.DR_AGG_SUM, N.DR_AGG_IN_SIZE, b"size", 0)], 1), 'aggregate spec 0: DR_AGG_IN_SIZE takes the name "" and the type 0'),
        ((None, 0, None, 0, [(N.DR_AGG_SUM, N.DR_AGG_IN_MTIME, b"", 4)], 1), 'aggregate spec 0: DR_AGG_IN_MTIME takes the name "" and the type 0'),
        ((None, 0, None, 0, [col(N.DR_AGG_MAX, b"p", 12)], 1), "aggregate spec 0: no valid column type (code 12)"),
        ((None, 0, None, 0, [col(N.DR_AGG_MIN, b"x", src(1, 6))], 1), "predicate column 0: minValues statistics have no BOOLEAN (type 6)"),
        ((None, 0, None, 0, [ok, col(N.DR_AGG_MAX, b"x", src(2, 10))], 2), "predicate column 1: maxValues statistics have no BINARY (type 10)"),
        ((None, 0, None, 0, [col(N.DR_AGG_SUM, b"x", src(3, 3))], 1), "predicate column 0: nullCount is a LONG, not type 3"),
        ((None, 0, None, 0, [col(N.DR_AGG_SUM, b"", src(4, 0))], 1), "predicate column 0: numRecords is a LONG, not type 0"),
        ((None, 0, None, 0, [col(N.DR_AGG_COUNT, b"x", src(5, 4))], 1), "predicate column 0: unknown source 5 (DR_SRC_PARTITION .. DR_SRC_STATS_NUMRECORDS)"),
        ((None, 0, None, 0, [col(N.DR_AGG_SUM, b"ab", src(4, 4))], 1), 'predicate column 0: numRecords takes the name "", not a path of 2 bytes'),
        ((None, 0, None, 0, [col(N.DR_AGG_MIN, b"a\x01\x01b", src(1, 4))], 1), "predicate column 0: segment 1 of the statistics path is empty"),
        ((None, 0, None, 0, [col(N.DR_AGG_MIN, b"\x01".join([b"a"] * 9), src(1, 4))], 1), "predicate column 0: a statistics path has at most 8 segments, not 9"),
        ((None, 0, None, 0, [col(N.DR_AGG_MAX, b"y" * 256, src(2, 0))], 1), "predicate column 0: a statistics path has at most 255 bytes, not 256"),
        ((None, 0, None, 0, [col(N.DR_AGG_SUM, b"s", src(1, 0))], 1), "aggregate spec 0: SUM takes BYTE .. LONG, size and modificationTime, not type 0"),
        ((None, 0, None, 0, [ok, col(N.DR_AGG_SUM, b"d", src(2, 8))], 2), "aggregate spec 1: SUM takes BYTE .. LONG, size and modificationTime, not type 8"),
        ((None, 0, None, 0, [col(N.DR_AGG_SUM, b"p", 5)], 1), "aggregate spec 0: SUM takes BYTE .. LONG, size and modificationTime, not type 5"),
    ]
    want = sum(f["size"] for f in live)
    for args, text in cases:
        rc, msg = _raw(engine, st, *args)
        assert rc == INVALID_ARG and text in msg, (args[4], msg)
        res = st.aggregate([("sum", "size")])  # the state still answers
        assert int(res["value_lo"][0, 0]) == want
    assert _raw(engine, st, None, -5, None, -5, [ok], 1) == (0, "")  # nrows / ngroups are ignored with NULL arrays
    assert _raw(engine, st, [], 0, [0], 0, None, 0) == (0, "")


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
                        st.aggregate([("sum", "size")])
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
        assert code == "DR_E_UNSUPPORTED" and "sharded" in msg


# ---- the Python layer ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def snapshot(tmp_path_factory):
    from delta_amd.delta_log import DeltaLog
    d = str(tmp_path_factory.mktemp("agg_snap"))
    F.build(d, checkpoint=True)
    DeltaLog.clear_cache()
    snap = DeltaLog.for_table(d).snapshot
    yield snap
    snap.release()
    DeltaLog.clear_cache()


def _data_size(recs):
    n = [F.typed(f["stats"], F.NUMRECORDS, (), "long") for f in recs]
    return {"bytesCompressed": sum(f["size"] for f in recs), "rows": None if any(t is None for t in n) else sum(t[0] for t in n),
            "files": len(recs)}


def test_scan_sizes(snapshot):
    filters = [("and", ("=", F.C("p"), F.L("integer", 1)), (">=", F.C("id"), F.L("long", 1000))), ("<", F.C("id"), F.L("long", 9000))]
    total = _data_size(snapshot.all_files)
    assert total["rows"] is None and total["files"] == F.N_LIVE  # the corpus has files without numRecords
    for skipping in (False, True):
        got = snapshot.scan_sizes(filters, data_skipping=skipping)
        assert got["total"] == total
        assert got["partition"] == _data_size(snapshot.files_for_scan(filters))
        assert got["scanned"] == _data_size(snapshot.files_for_scan(filters, data_skipping=skipping))
    assert got["scanned"]["files"] < got["partition"]["files"] < total["files"]
    # a selection in which every file has numRecords: rows is their sum
    narrow = [("=", F.C("p"), F.L("integer", 2)), (">=", F.C("id"), F.L("long", 20000))]
    got = snapshot.scan_sizes(narrow, data_skipping=True)
    want = _data_size(snapshot.files_for_scan(narrow, data_skipping=True))
    assert got["scanned"] == want and want["files"] > 0
    assert snapshot.scan_sizes([]) == {"total": total, "partition": total, "scanned": total}


def _prove_by_hand(recs, kind, path=None, typ=None):
    """The rules of aggregate_from_metadata, written over records."""
    n = [F.typed(f["stats"], F.NUMRECORDS, (), "long") for f in recs]
    if kind == "count":
        return None if any(t is None for t in n) else sum(t[0] for t in n)
    nc = [F.typed(f["stats"], F.NULLCOUNT, path, "long") for f in recs]
    if kind == "count_col":
        return None if any(t is None for t in n + nc) else sum(t[0] for t in n) - sum(t[0] for t in nc)
    src = F.MIN if kind == "min" else F.MAX
    vals = [F.typed(f["stats"], src, path, typ) for f in recs]
    for v, a, b in zip(vals, n, nc):
        if v is None and (a is None or b is None or a[0] != b[0]):
            return None
    have = [v[0] for v in vals if v is not None]
    return (min if kind == "min" else max)(have) if have else None


def test_aggregate_from_metadata(snapshot):
    files = snapshot.all_files
    by_p = lambda k: [f for f in files if f["partitionValues"]["p"] == str(k)]  # noqa: E731
    exprs = [("count",), ("count", "id"), ("min", "id"), ("max", "id"), ("min", "p"), ("max", "P"), ("count", "p"), ("max", "dt"),
             ("min", "ts"), ("max", "s"), ("min", "d"), ("min", "dec"), ("min", "b"), ("count", "s")]
    got = snapshot.aggregate_from_metadata(exprs)
    # the corpus has files with absent and malformed stats: no count, no data-column answer over all files
    assert got == [None, None, None, None, 0, 4, None, None, None, None, None, None, None, None]
    assert _prove_by_hand(files, "count") is None and _prove_by_hand(files, "min", ("id",), "long") is None
    # one partition: what the rules give over its files (partition answers always)
    regular = [("=", F.C("p"), F.L("integer", 3))]
    sel = by_p(3)
    got = snapshot.aggregate_from_metadata(exprs, regular)
    want = [_prove_by_hand(sel, "count"), _prove_by_hand(sel, "count_col", ("id",)), _prove_by_hand(sel, "min", ("id",), "long"),
            _prove_by_hand(sel, "max", ("id",), "long"), 3, 3, _prove_by_hand(sel, "count"), _prove_by_hand(sel, "max", ("dt",), "date"),
            None, None, None, None, _prove_by_hand(sel, "min", ("b",), "byte"), _prove_by_hand(sel, "count_col", ("s",))]
    assert got == want
    # by partition: each group against the rules over its files (the proven side of the count and data-column
    # rules is test_missing_statistic_with_all_null_column's: every partition here holds a file without stats)
    groups = snapshot.aggregate_from_metadata(exprs, by_partition=True)
    assert [g[0] for g in groups] == [(k,) for k in range(5)]
    for (k,), answers in groups:
        sel = by_p(k)
        want = [_prove_by_hand(sel, "count"), _prove_by_hand(sel, "count_col", ("id",)), _prove_by_hand(sel, "min", ("id",), "long"),
                _prove_by_hand(sel, "max", ("id",), "long"), k, k, _prove_by_hand(sel, "count"), _prove_by_hand(sel, "max", ("dt",), "date"),
                None, None, None, None, _prove_by_hand(sel, "min", ("b",), "byte"), _prove_by_hand(sel, "count_col", ("s",))]
        assert answers == want, k
        assert answers[:4] == [None] * 4 and answers[4:6] == [k, k]
    # a data conjunct: partition answers stay, every count and data-column answer is None
    got = snapshot.aggregate_from_metadata([("count",), ("min", "id"), ("max", "p"), ("count", "p")],
                                           [("=", F.C("p"), F.L("integer", 1)), (">", F.C("id"), F.L("long", 0))])
    assert got == [None, None, 1, None]


def test_missing_statistic_with_all_null_column(engine, tmp_path):
    """min / max of a data column stays proven when the files without the statistic hold no non-NULL value."""
    from delta_amd.delta_log import DeltaLog
    log = os.path.join(str(tmp_path), "_delta_log")
    os.makedirs(log)
    stats = [{"numRecords": 10, "minValues": {"id": 5}, "maxValues": {"id": 9}, "nullCount": {"id": 0}},
             {"numRecords": 4, "minValues": {}, "maxValues": {}, "nullCount": {"id": 4}},       # all NULL: no statistic
             {"numRecords": 6, "minValues": {"id": -2}, "maxValues": {"id": 3}, "nullCount": {"id": 1}},
             {"numRecords": 4, "minValues": {}, "maxValues": {}, "nullCount": {"id": 3}}]       # p = 1: a value the statistics miss
    with open(os.path.join(log, "%020d.json" % 0), "w") as f:
        f.write(json.dumps({"protocol": F.PROTOCOL}) + "\n" + json.dumps({"metaData": F.METADATA}) + "\n")
        for i, s in enumerate(stats):
            f.write(json.dumps({"add": {"path": "m-%d" % i, "partitionValues": {"p": str(i // 3)}, "size": 1, "modificationTime": 1,
                                        "dataChange": True, "stats": json.dumps(s)}}) + "\n")
    DeltaLog.clear_cache()
    try:
        snap = DeltaLog.for_table(str(tmp_path)).snapshot
        exprs = [("min", "id"), ("max", "id"), ("count", "id"), ("count",)]
        assert snap.aggregate_from_metadata(exprs) == [None, None, 16, 24]
        assert snap.aggregate_from_metadata(exprs, [("=", F.C("p"), F.L("integer", 0))]) == [-2, 9, 15, 20]
        assert snap.aggregate_from_metadata(exprs, by_partition=True) == [((0,), [-2, 9, 15, 20]), ((1,), [None, None, 1, 4])]
        # every file has numRecords: DeltaScan's rows are their sum
        sizes = snap.scan_sizes([("=", F.C("p"), F.L("integer", 0)), (">", F.C("id"), F.L("long", 4))], data_skipping=True)
        assert sizes == {"total": {"bytesCompressed": 4, "rows": 24, "files": 4}, "partition": {"bytesCompressed": 3, "rows": 20, "files": 3},
                         "scanned": {"bytesCompressed": 2, "rows": 14, "files": 2}}
        snap.release()
    finally:
        DeltaLog.clear_cache()


def test_cells_and_groups_on_the_bounds_build():
    lib = os.path.join(ROOT, "delta_amd", "libdeltareplay_bounds.so")
    assert os.path.exists(lib), "make builds libdeltareplay_bounds.so"
    if os.environ.get("DR_LIB") == "libdeltareplay_bounds.so":
        return  # this is the child
    sel = ["tests/test_gpu_aggregate.py::test_every_cell_one_group_all_live", "tests/test_gpu_aggregate.py::test_group_layouts"]
    env = dict(os.environ, DR_LIB="libdeltareplay_bounds.so")
    r = subprocess.run([sys.executable, "-u", "-m", "pytest", "-x", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider"] + sel,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "4 passed" in out
