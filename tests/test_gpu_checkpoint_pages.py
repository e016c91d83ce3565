"""The device checkpoint writer's pages (dr_state_write_checkpoint; k_enc_count / k_enc_fill / k_enc_pack /
k_snap_compress / k_snap_gather of k_encode.hip) against references that share nothing with it.

Compressor: the add.stats page of a one-add table is steered through the string the writer copies verbatim
(tests/ckpt_writer_corpus.py: body kinds x page sizes). Every SNAPPY page body of the part decodes, with the
strict reference decoder and with libsnappy, to the page the same part holds uncompressed; the uncompressed
add.stats page is the bytes the format prescribes for the test's string; the elements keep the fragment rule
the kernel's comment promises, show the forms the body was built for, and stay within counts that follow from
the algorithm (one thread per 64-byte slice, greedy, earliest position per bucket), never from a measurement.

Reader: the written part, put into a copy of the log as its checkpoint, replays on the device to the oracle's
state of the original log without a page going to the serial decoder.

Levels and values: every column of the pyarrow read-back equals expected_rows (replayed by the test from its
own action dicts) for row groups and parts that begin and end at every boundary of the head / adds / removes
sections, degenerate states, maps of every shape, int64 extremes and BOOLEAN leaves of 1, 7, 8 and 9 values.
The two file-action sides compare as multisets keyed by path (tests/test_gpu_export_order.py pins the order)."""
import io
import os
import shutil

import pytest

from oracle import delta_oracle as O
from tests import ckpt_writer_corpus as W
from tests import snappy_corpus as S
from tests.test_gpu_parity import _assert_same
from tests.test_gpu_snappy_pages import _report

pytestmark = pytest.mark.gpu

F = W.FRAG


@pytest.fixture(scope="module")
def engine():
    from delta_amd.delta_log import Engine
    return Engine.get(0)


def _state(engine, lp, cutoff=0):
    staged = engine.stage_log(lp)
    try:
        return staged.replay(cutoff)
    finally:
        staged.release()


def _part(st, part=1, parts=1, **kw):
    data, n = st.write_checkpoint_part(part, parts, **dict(dict(stats=True, parsed=False), **kw))
    return bytes(data), n


def _rows(data):
    import pyarrow.parquet as pq
    return pq.read_table(io.BytesIO(data)).to_pylist()


def _leaf_pages(buf):
    """{leaf: [(codec, num_values, uncompressed size, body)]} over all row groups, in file order."""
    out = {}
    for _, _, md, leaf, start, end in S._chunks(buf)[1]:
        for h, pos, _, _ in S._pages(buf, start, end):
            assert S._get(h, 1) == 0     # DATA_PAGE
            out.setdefault(leaf, []).append((S._get(md, 4), S._get(S._get(h, 5), 1), S._get(h, 2), buf[pos:pos + S._get(h, 3)]))
    return out


def _copies(el):
    return [e for e in el if e[0] == "copy"]


def _lits(el):
    return [e for e in el if e[0] == "lit"]


def _in_fragment(el, f):
    return [e for op, _, e in S.spans(el) if op // F == f]


def _n_in(el):
    return sum(len(S.encode_element(e)) for e in el)


def _check_body(body, raw):
    """The SNAPPY body decodes to `raw` with both decoders, behind a minimal preamble; its elements keep the
    fragment rule at 8 KiB (and so the reader's at 64 KiB) and fit the compressor's slot."""
    n = len(raw)
    assert S.reference(body, n) == raw
    assert S.pyarrow_decode(body, n) == raw
    assert body[:S.preamble_of(body)[1]] == S.varint(n)
    el = S.elements_of(body)
    assert el is not None and S.keeps_fragments(el)
    for op, ln, e in S.spans(el):
        assert op // F == (op + ln - 1) // F, ("an element crosses a fragment end", op, ln)
        assert e[0] == "lit" or 0 < e[1] <= op % F, ("a copy reaches before its fragment", op, e)
    for f in range(-(-n // F)):
        assert _n_in(_in_fragment(el, f)) <= W.SLOT
    return el


# ---- the compressor ------------------------------------------------------------------------------------------
_SOME = [193, 197, 8192, 8193, 16384, 65536, 65537, 2 * 65536 + 100]
CASES = [("random", s) for s in [W.SMALLEST] + W.SIZES]
CASES += [(k, s) for k in ("runs", "slice_literals(1)", "periodic64") for s in _SOME]
CASES += [("slice_literals(%d)" % L, s) for L in (59, 60, 61, 63) for s in (8192, 8195)]
CASES += [("utf8", s) for s in (197, 8193, 65537)]
CASES += [(k, s) for k in ("copy_lengths", "collide") for s in (8192, 16384)]


def _forms(kind, size, el, page):
    """What the body kind was built for, on the elements of its add.stats page."""
    n = len(page)
    sp = S.spans(el)
    if kind == "random":
        # a slice costs at most its bytes and a two-byte literal tag; a copy of 4 or more bytes costs at most 3 and the
        # literal it splits off one tag more, so no slice grows by more than 2. 64 symbols: a group recurs by chance
        # about 8192 / 64^4 of the time per position, far below 1 % of the bytes
        assert _n_in(el) <= n + 2 * -(-n // 64)
        assert sum(e[2] for e in _copies(el)) <= n / 100
        if size in (252, 253):     # the tail slice is one literal of 60 (one-byte tag) or 61 (60 << 2 and a length byte)
            assert el[-1] == ("lit", page[-(size - 192):], 0 if size == 252 else 1)
        if size in (193, 195):
            assert el[-1] == ("lit", page[192:], 0)
    if kind in ("slice_literals(1)", "slice_literals(59)", "slice_literals(60)"):
        L = int(kind[15:-1])
        assert sum(len(e[1]) == L and e[2] == 0 for e in _lits(el)) >= 30 * (n // F) or n < F
        assert sum(e[2] == 64 - L for e in _copies(el)) >= 30 * (n // F) or n < F
    if kind in ("slice_literals(61)", "slice_literals(63)"):
        assert sum(len(e[1]) == 64 and e[2] == 1 for e in _lits(el)) >= 30
    if kind == "copy_lengths":
        at = {op: e for op, _, e in sp if e[0] == "copy"}
        for f0 in range(0, n, F):
            for s, t, ln in W.COPY_PLAN:
                assert at.get(f0 + t) == ("copy", t - s, ln, 1 if ln <= 11 and t - s < 2048 else 2), (f0, s, t, ln, at.get(f0 + t))
        tags = {(e[1], e[2]): e[3] for e in at.values()}
        assert tags[(2047, 4)] == tags[(2047, 11)] == 1 and tags[(2047, 12)] == 2
        assert tags[(2048, 4)] == tags[(2048, 11)] == tags[(2048, 12)] == 2
    if kind == "runs":
        if n >= 3 * W.RUN:
            for off in (1, 2, 3):
                assert any(e[1] == off and e[2] > off for e in _copies(el)), off
        # inside the first run (one byte) a slice is a copy, or a literal and a copy
        per = {}
        for op, _, _ in sp:
            per[op // 64] = per.get(op // 64, 0) + 1
        assert all(per[s] <= 2 for s in range(1, min(n, W.RUN) // 64))
    if kind == "periodic64":
        for f in range(n // F):     # full fragments: the first slice's literal, one copy per remaining slice
            mine = _in_fragment(el, f)
            assert len(mine) <= 128 and _n_in(mine) <= 66 + 127 * 3, (f, len(mine), _n_in(mine))
    if kind == "collide":
        # the earliest-position table holds the FIRST of the bucket's groups: the repeat of the last one finds the
        # wrong candidate and is lost, so its four bytes leave as literal bytes (a most-recent table would copy them)
        for f0 in range(0, n, F):
            _, rep = W.collide_repeat(f0)
            assert all(e[0] == "lit" for op, ln, e in sp if op < rep + 4 and op + ln > rep)


@pytest.mark.parametrize("kind,size", CASES, ids=["%s-%s" % c for c in CASES])
def test_compressed_pages_decode_to_the_uncompressed_ones(engine, tmp_path, kind, size):
    string, page = W.steered(kind, size)
    # the other verbatim columns ride along, a null tag value among them (pages of 64 KiB and more make the commit
    # line longer than K1's 16-bit token offsets: the General walker's)
    side = {} if string is None else {"partitionValues": {"p": string[:700]}, "tags": {"t": string[-300:], "u": None}}
    lp, actions = W.one_add_log(tmp_path / "t", string, **side)
    st = _state(engine, lp)
    try:
        a, n = _part(st, snappy=True)
        b, _ = _part(st, snappy=False)
        again, _ = _part(st, snappy=True)
    finally:
        st.release()
    assert n == 3
    # the levels and the value as the format prescribes them: the spare bits of the last pack group are zero
    assert _leaf_pages(b)["add.stats"][0][3] == page
    assert a == again          # the last fragment's staging reads past the page's end: nothing of it may show
    W.assert_rows(_rows(a), W.expected_rows(actions, 0))
    W.assert_rows(_rows(b), W.expected_rows(actions, 0))
    pa_, pb = _leaf_pages(a), _leaf_pages(b)
    assert list(pa_) == list(pb)
    device = [leaf for leaf in pa_ if pa_[leaf][0][0] == 1]
    assert "add.stats" in device and "add.path" in device and len(device) >= 9
    for leaf in device:
        (codec, nv, usize, body), = pa_[leaf]
        (codec0, nv0, usize0, raw), = pb[leaf]
        assert codec0 == 0 and nv == nv0 and usize == usize0 == len(raw), leaf
        el = _check_body(body, raw)
        if leaf == "add.stats":
            assert raw == page
            _forms(kind, size, el, page)


# ---- our reader reads our writer -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "runs", "slice_literals(1)"])
@pytest.mark.parametrize("size", [8192, 8193, 65536, 65537, 2 * 65536 + 100])
def test_the_reader_reads_the_written_part(engine, tmp_path, capfd, monkeypatch, kind, size):
    from delta_amd.checkpoint import write_last_checkpoint
    string, page = W.steered(kind, size, seed=5)
    lp, actions = W.one_add_log(tmp_path / "t", string, partitionValues={"p": string[:700]},
                                tags={"t": string[:5000], "u": None})
    snap = O.state_reconstruction(O.get_log_segment(lp), 0)
    st = _state(engine, lp)
    try:
        data, n = _part(st, snappy=True)
    finally:
        st.release()
    lp2 = os.path.join(str(tmp_path), "copy", "_delta_log")
    shutil.copytree(lp, lp2)
    with open(os.path.join(lp2, "%020d.checkpoint.parquet" % 0), "wb") as f:
        f.write(data)
    write_last_checkpoint(lp2, {"version": 0, "size": n})
    (_, c, u), = S.snappy_pages(os.path.join(lp2, "%020d.checkpoint.parquet" % 0), "add.stats")
    assert u == size
    snappy_leaves = [leaf for leaf, p in _leaf_pages(data).items() if p[0][0] == 1]
    assert len(snappy_leaves) == 9
    monkeypatch.setenv("DR_SNAP_DEBUG", "1")
    capfd.readouterr()
    staged = engine.stage_log(lp2)
    try:
        assert staged.plan()["checkpoint_rows"] == 3
        st = staged.replay(0)
    finally:
        staged.release()
    try:
        _assert_same(st, snap)
        live = st.export(0)
        assert [a["stats"] for a in live] == [string] and live[0]["tags"] == {"t": string[:5000], "u": None}
    finally:
        st.release()
    pages, bad, codes, _, which = _report(capfd.readouterr().err)
    # the report is there and counts the pages that went through the SNAPPY kernels: the stats page at least, unless it
    # is incompressible (a literals-only page is the planner's copy and is not counted)
    assert kind == "random" or pages >= 1, (pages, bad)
    assert bad == 0 and not codes and not which, (pages, bad, codes, which)


# ---- levels and values -----------------------------------------------------------------------------------------
H, NA, NR = 3, 300, 40


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    lp, actions = W.write_log(tmp_path_factory.mktemp("ckpt_levels"), W.level_table(NA, NR))
    want = W.expected_rows(actions, W.CUTOFF)
    assert [W.kind_of(r) for r in want] == ["protocol", "metaData", "txn"] + ["add"] * NA + ["remove"] * NR
    return lp, actions, want


def _level_count(row, leaf):
    """Levels of one row in `leaf`: one, or one per entry of a non-empty map / list."""
    v = row
    for name in leaf.split("."):
        if name in ("key_value", "list"):
            return max(1, len(v))
        v = v.get(name) if isinstance(v, dict) else None
        if v is None:
            return 1
    return 1


def _check_levels(data, rows):
    """Every page header's num_values (and the footer's) is the count of levels of its row group's rows."""
    import pyarrow.parquet as pq
    md = pq.ParquetFile(io.BytesIO(data)).metadata
    pages = _leaf_pages(data)
    at = 0
    for g in range(md.num_row_groups):
        n = md.row_group(g).num_rows
        for j in range(md.num_columns):
            col = md.row_group(g).column(j)
            want = sum(_level_count(r, col.path_in_schema) for r in rows[at:at + n])
            assert col.num_values == want == pages[col.path_in_schema][g][1], (g, col.path_in_schema)
        at += n
    assert at == len(rows) and all(len(p) == md.num_row_groups for p in pages.values())
    return md


@pytest.mark.parametrize("rg", [1, 7, 8, 9, 255, 256, 257, H, H + 1, H + NA - 1, H + NA, H + NA + 1])
def test_row_group_sizes(engine, big, rg):
    """Row groups of every size around the pack group (8) and the block (256), and row groups that end exactly at the
    head / adds / removes boundaries and one row to either side."""
    lp, actions, want = big
    st = _state(engine, lp, W.CUTOFF)
    try:
        data, n = _part(st, row_group_rows=rg, snappy=(rg == 9))
    finally:
        st.release()
    rows = _rows(data)
    assert n == len(rows) == H + NA + NR
    W.assert_rows(rows, want)
    md = _check_levels(data, rows)
    assert [md.row_group(g).num_rows for g in range(md.num_row_groups)] == [min(rg, len(rows) - r0) for r0 in range(0, len(rows), rg)]


def test_the_table_holds_every_case(big):
    """The level table's own contents: what the parametrised tests above and below compare column by column."""
    want = big[2]
    adds = [r["add"] for r in want if r["add"]]
    rms = [r["remove"] for r in want if r["remove"]]
    for side in (adds, rms):
        for col in ("partitionValues", "tags"):
            maps = [x[col] for x in side]
            assert None in maps and [] in maps and any(m and len(m) == 1 for m in maps), col
            assert {9, 300} <= {len(m) for m in maps if m}, col
            assert any(m and m[0][1] is None and m[-1][1] is not None for m in maps)
            assert any(m and m[-1][1] is None and m[0][1] is not None for m in maps)
            assert any(m and len(m) > 1 and all(v is None for _, v in m) for m in maps)
            assert any(m and m[0][0] == "" for m in maps) and any(m and m[0][1] == "" for m in maps)
    assert {a["size"] for a in adds} == {a["modificationTime"] for a in adds} == set(W.I64)
    assert {r["deletionTimestamp"] for r in rms} == set(W.I64[:5]) | {None}     # -2^63 is never past a cutoff
    assert {r["size"] for r in rms} >= set(W.I64)
    assert {a["stats"] for a in adds} >= {None, ""} and {r["extendedFileMetadata"] for r in rms} == {True, False}
    assert not any(x["dataChange"] for x in adds + rms)


@pytest.mark.parametrize("parts", [2, 3, 86, 115])
def test_parts_of_the_level_table(engine, big, parts):
    """Parts whose windows begin inside each section; 115 parts of 3 rows end at H and at H + NA, 86 of 4 at H + 1 and
    H + NA + 1."""
    lp, actions, want = big
    st = _state(engine, lp, W.CUTOFF)
    try:
        got = [_part(st, k + 1, parts, snappy=(parts == 3)) for k in range(parts)]
    finally:
        st.release()
    rows = []
    for data, n in got:
        mine = _rows(data)
        assert len(mine) == n
        rows += mine
    assert sum(n for _, n in got) == len(want)
    W.assert_rows(rows, want)


SMALL = (3, 5, 6)     # head rows, adds, removes: 14 rows


def _small_log(d, na=SMALL[1], nr=SMALL[2]):
    c0 = W.head(txns=[{"appId": "a", "version": 1, "lastUpdated": 2}])
    c0 += [W.add("s-%02d" % i, partitionValues={"k%d" % j: str(i) for j in range(i % 4)}, size=W.I64[i % 6],
                 tags=None if i % 2 else {"t": None}, stats="s%d" % i) for i in range(na + nr)]
    c1 = [W.remove("s-%02d" % i, deletionTimestamp=5 + i, extendedFileMetadata=bool(i % 3 == 0), size=i,
                   partitionValues={"k": "v"} if i % 2 else {}) for i in range(na, na + nr)]
    return W.write_log(d, [c0, c1] if c1 else [c0])


def test_every_window_of_a_small_table(engine, tmp_path):
    """14 rows (3 head, 5 adds, 6 removes): every row group size and every number of parts up to past the last row.
    Among them a row group, and a part, ends at H, H + 1, H + NA - 1, H + NA and H + NA + 1 (3, 4, 7, 8, 9); parts past
    the last row are empty files pyarrow reads, with the full schema."""
    h, na, nr = SMALL
    total = h + na + nr
    lp, actions = _small_log(tmp_path / "t")
    want = W.expected_rows(actions, 0)
    assert len(want) == total
    st = _state(engine, lp)
    try:
        by_rg = {rg: _part(st, row_group_rows=rg) for rg in range(1, total + 2)}
        by_parts = {p: [_part(st, k + 1, p, row_group_rows=(p % 3)) for k in range(p)] for p in range(1, total + 4)}
    finally:
        st.release()
    import pyarrow.parquet as pq
    schema = pq.read_schema(io.BytesIO(by_rg[1][0]))
    for rg, (data, n) in by_rg.items():
        rows = _rows(data)
        assert n == total
        W.assert_rows(rows, want)
        _check_levels(data, rows)
    ends = set()
    for p, got in by_parts.items():
        rows = []
        for data, n in got:
            mine = _rows(data)
            assert len(mine) == n and pq.read_schema(io.BytesIO(data)).equals(schema)
            rows += mine
            ends.add(len(rows))
        step = -(-total // p)
        assert [n for _, n in got] == [max(0, min(step, total - k * step)) for k in range(p)]
        W.assert_rows(rows, want)
    assert ends >= {h, h + 1, h + na - 1, h + na, h + na + 1}
    assert [n for _, n in by_parts[total + 3]][-3:] == [0, 0, 0]


@pytest.mark.parametrize("state", ["everything removed", "no tombstones", "one add only"])
def test_degenerate_states(engine, tmp_path, state):
    if state == "one add only":
        lp, actions = _small_log(tmp_path / "t", 1, 0)
    elif state == "no tombstones":
        lp, actions = _small_log(tmp_path / "t", 9, 0)
    else:
        lp, actions = _small_log(tmp_path / "t", 0, 9)
    want = W.expected_rows(actions, 0)
    assert [W.kind_of(r) for r in want[3:]] == {"one add only": ["add"], "no tombstones": ["add"] * 9,
                                                 "everything removed": ["remove"] * 9}[state]
    st = _state(engine, lp)
    try:
        whole = [_part(st, snappy=s, row_group_rows=rg) for s in (False, True) for rg in (0, 1, 3)]
        halves = [_part(st, k + 1, 2) for k in range(2)]
    finally:
        st.release()
    for data, n in whole:
        rows = _rows(data)
        W.assert_rows(rows, want)
        _check_levels(data, rows)
    W.assert_rows(_rows(halves[0][0]) + _rows(halves[1][0]), want)


@pytest.mark.parametrize("k", [1, 7, 8, 9])
def test_boolean_leaves_of_k_values(engine, tmp_path, k):
    """k adds and k tombstones in one row group: add.dataChange, remove.dataChange and remove.extendedFileMetadata
    hold k values, bit-packed into one or two bytes whose spare bits are zero."""
    lp, actions = _small_log(tmp_path / "t", k, k)
    want = W.expected_rows(actions, 0)
    st = _state(engine, lp)
    try:
        data, n = _part(st, snappy=False)
    finally:
        st.release()
    rows = _rows(data)
    assert n == 3 + 2 * k
    W.assert_rows(rows, want)
    flags = [r["remove"]["extendedFileMetadata"] for r in rows if r["remove"]]
    assert len(flags) == k and (k == 1 or {True, False} == set(flags))
    packed = sum(1 << i for i, f in enumerate(flags) if f).to_bytes((k + 7) // 8, "little")
    pages = _leaf_pages(data)
    levels = [0] * 3 + [0] * k + [2] * k
    assert pages["remove.extendedFileMetadata"][0][3] == W.page_prefix(levels, 2) + packed
    assert pages["remove.dataChange"][0][3] == W.page_prefix(levels, 2) + bytes((k + 7) // 8)
    assert pages["add.dataChange"][0][3] == W.page_prefix([0] * 3 + [2] * k + [0] * k, 2) + bytes((k + 7) // 8)
