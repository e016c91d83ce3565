"""LZ4-compressed checkpoint pages on the device (k_lz4): replays of checkpoints pyarrow wrote with
compression="lz4" (Parquet codec 7, LZ4_RAW) and of the same files re-framed as codec 5 (Hadoop's units,
tests/lz4_corpus.rewrite) equal the oracle record for record across page sizes, page versions, dictionary
use and compression levels; export, filter, lookup and scan order answer as on the SNAPPY twin; chunks of
one file may mix codecs; page bodies replaced by blocks a steered compressor wrote (short offsets, offset
65,535, long lengths, several units and inner blocks) replay alike; a table of its own, whose stats hold
two- and three-byte periods, puts overlapping matches longer than a wave, matches across the kernel's ring
wrap and sequences cut at its rounds' ends through the kernel;
pages of literals only are copies; malformed bodies -- each refused by the host decoder under the
sanitizers in tests/test_lz4_host.py first -- end in DR_E_PARQUET naming the column; a table without LZ4
pages pays nothing.

The logical table is one (config 3 at scale 0.001, seed 3, about 16 K actions): it is built once, the
oracle reads it once, and each case rewrites only the checkpoint file. pyarrow cuts pages per write
batch, so the 4 KiB cases write batches of 32 rows to get pages that small."""
import os
import re
import shutil

import numpy as np
import pytest

from oracle import delta_oracle as O
from tests import filter_corpus as F
from tests import lz4_corpus as L
from tests.test_gpu_parity import _assert_same
from tests.test_lz4_host import MALFORMED, malformed_bodies

pytestmark = pytest.mark.gpu

HOT = ("add.path", "add.size", "remove.path", "remove.deletionTimestamp")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kernel_constant(name):
    src = open(os.path.join(ROOT, "delta_amd", "csrc", "kernels.h")).read()
    return re.search(r"constexpr uint32_t %s = ([^;]+);" % name, src).group(1)


RING = int(_kernel_constant("LZ4_RING_BYTES"))
assert _kernel_constant("LZ4_ROUND_SPAN") == "LZ4_RING_BYTES - 65536"
SPAN, BATCH = RING - 65536, int(_kernel_constant("LZ4_ROUND_BATCH"))


@pytest.fixture(scope="module")
def engine():
    from delta_amd.delta_log import Engine
    return Engine.get(0)


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    """(log path of the SNAPPY twin, its checkpoint's file name, the checkpoint as a table, cutoff,
    the oracle's snapshot)."""
    import pyarrow.parquet as pq
    from delta_amd.testing import synth as S
    d = str(tmp_path_factory.mktemp("lz_base"))
    exp = S.build_table(d, S.config_spec(3, 0.001), seed=3)
    lp = os.path.join(d, "_delta_log")
    ck = [f for f in os.listdir(lp) if f.endswith(".checkpoint.parquet")]
    assert len(ck) == 1
    cutoff = exp.min_file_retention_timestamp
    return lp, ck[0], pq.read_table(os.path.join(lp, ck[0])), cutoff, O.state_reconstruction(O.get_log_segment(lp), cutoff)


def _variant(base, d, codec=7, compression="lz4", level=None, page_size=1 << 20, version="1.0", dictionary=False):
    """A copy of the base log whose checkpoint is rewritten; (log path, checkpoint path). Codec 5: pyarrow's
    codec-7 file with every LZ4 page re-framed as one Hadoop unit of one inner block."""
    import pyarrow.parquet as pq
    lp0, ck, table = base[:3]
    lp = os.path.join(str(d), "_delta_log")
    shutil.copytree(lp0, lp)
    kw = {"compression_level": level} if level is not None else {}
    if page_size < 65536:
        kw["write_batch_size"] = 32
    pq.write_table(table, os.path.join(lp, ck), compression=compression, use_dictionary=dictionary, version="1.0",
                   data_page_version=version, data_page_size=page_size, write_statistics=False, **kw)
    if codec == 5:
        L.to_hadoop(os.path.join(lp, ck), os.path.join(lp, ck))
    return lp, os.path.join(lp, ck)


def _replay(engine, lp, cutoff, timing=False):
    staged = engine.stage_log(lp)
    try:
        if timing:
            engine.set_timing(True)
        st = staged.replay(cutoff)
        names = {k.split("::")[-1] for k in engine.last_timings()} if timing else set()
        return st, staged.plan(), names
    finally:
        if timing:
            engine.set_timing(False)
        staged.release()


def _check(engine, base, lp):
    st, plan, _ = _replay(engine, lp, base[3])
    try:
        _assert_same(st, base[4])
    finally:
        st.release()
    return plan


def _hot_pages(ck):
    """(pages the kernel decodes, pages the planner turns into copies) of the hot leaves."""
    buf = open(ck, "rb").read()
    pages = [p for leaf in HOT for p in L.lz4_pages(ck, leaf) if p[2] > 0]
    copies = [p for p in pages if L.is_literals_only(buf[p[0]:p[0] + p[1]], p[2], p[3])]
    return [p for p in pages if p not in copies], copies


def _assert_plan(plan, ck):
    pages, _ = _hot_pages(ck)
    assert plan["lz4_pages"] == len(pages) > 0
    assert plan["lz4_in_bytes"] == sum(p[1] for p in pages)
    assert plan["lz4_out_bytes"] == sum(p[2] for p in pages)
    return pages


@pytest.mark.parametrize("dictionary", [False, True])
@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("page_size", [4096, 1 << 20])
@pytest.mark.parametrize("codec", [7, 5])
def test_parity(engine, base, tmp_path, codec, page_size, version, dictionary):
    """Fails on a build without the decoder with DR_E_UNSUPPORTED (checkpoint codec 7 or 5)."""
    lp, ck = _variant(base, tmp_path, codec=codec, page_size=page_size, version=version, dictionary=dictionary)
    assert set(L.codecs_of(ck).values()) == {codec}
    pages = _assert_plan(_check(engine, base, lp), ck)
    if page_size == 4096 and not dictionary:
        assert len(pages) > 100   # pages of a few KiB, not one per leaf


@pytest.mark.parametrize("codec", [7, 5])
def test_parity_level_12(engine, base, tmp_path, codec):
    lp, ck = _variant(base, tmp_path, codec=codec, level=12, page_size=4096, version="2.0")
    _assert_plan(_check(engine, base, lp), ck)


def test_export_filter_lookup_and_scan_order_as_on_the_snappy_twin(engine, base, tmp_path):
    from delta_amd.predicates import build_program, partition_schema
    lp, _ = _variant(base, tmp_path, codec=5, page_size=4096, version="2.0")
    st, _, _ = _replay(engine, lp, base[3])
    ref, _, _ = _replay(engine, base[0], base[3])
    try:
        live = ref.export(0)
        assert st.export(0) == live and st.export(1) == ref.export(1)
        metadata = next(a["metaData"] for a in ref.nonfile if "metaData" in a)
        prog = build_program(partition_schema(metadata), [("<", F.C("p1"), F.L("integer", 40))])
        sel = ref.filter(prog)
        assert 0 < len(sel) < len(live) and st.filter(prog) == sel
        queries = [a["path"] for a in live[:100]] + ["absent/" + a["path"] for a in live[:100]]
        got, want = st.lookup_paths(queries), ref.lookup_paths(queries)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert set(int(h) for h in want[0]) == {0, 1}
        assert list(st.scan_order()) == list(ref.scan_order())
    finally:
        st.release()
        ref.release()


def test_mixed_codecs_in_one_file(engine, base, tmp_path):
    import pyarrow.parquet as pq
    codec = {"add.path": "lz4", "add.size": "snappy", "remove.path": "none", "remove.deletionTimestamp": "gzip",
             "add.stats": "lz4", "add.modificationTime": "zstd", "remove.size": "zstd", "add.dataChange": "lz4"}
    md = pq.ParquetFile(os.path.join(base[0], base[1])).metadata
    names = [md.row_group(0).column(i).path_in_schema for i in range(md.num_columns)]
    lp, ck = _variant(base, tmp_path, compression={n: codec.get(n, ("zstd", "snappy", "gzip", "lz4")[len(n) % 4]) for n in names})
    # add.path stays codec 7; add.stats and the other LZ4 chunks become codec 5; remove.path of the hot
    # leaves too, from a second file that holds it as LZ4
    L.to_hadoop(ck, ck, leaves=[n for n in names if n != "add.path" and L.codecs_of(ck)[n] == 7])
    got = L.codecs_of(ck)
    assert got["add.path"] == 7 and got["add.stats"] == 5 and set(got.values()) == {0, 1, 2, 5, 6, 7}
    hot = _variant(base, tmp_path / "hot", compression={n: {"add.path": "lz4", "add.size": "zstd", "remove.path": "lz4",
                                                            "remove.deletionTimestamp": "gzip"}.get(n, "snappy") for n in names})
    L.to_hadoop(hot[1], hot[1], leaves=["remove.path"])
    assert {L.codecs_of(hot[1])[n] for n in HOT} == {7, 6, 5, 2}
    plan = _check(engine, base, lp)
    assert plan["lz4_pages"] > 0 and plan["gzip_pages"] > 0 and plan["snappy_in_bytes"] > 0 and plan["copy_bytes"] > 0
    plan = _check(engine, base, hot[0])
    assert plan["lz4_pages"] > 0 and plan["gzip_pages"] > 0 and plan["zstd_pages"] > 0 and plan["copy_bytes"] > 0


CRAFTED = {
    # kind: (page size of the variant, compressor options, what the walk must show)
    # the page's bytes decide which short offsets exist: the paths hold runs (offset 1) but no two- or
    # three-byte periods, which test_short_periods_the_ring_wrap_and_round_cuts brings in a table of its own
    "offset 1": (1 << 20, dict(offsets=(1, 2, 3)), lambda s: 1 in {o for _, o, _ in s}),
    "offset 65535": (1 << 20, dict(offsets=(65535,)), lambda s: 65535 in {o for _, o, _ in s}),
    "lengths with one to three extension bytes": (1 << 20, dict(min_ll=600), lambda s: any(len(l) >= 15 + 510 for l, _, _ in s)
                                                  and any(15 <= len(l) < 270 for l, _, _ in s) and any(m >= 19 for _, _, m in s)),
    "matches of four bytes": (4096, dict(max_ml=4), lambda s: len(s) > 2 * BATCH and {m for _, _, m in s if m} == {4}),
    # a page of several rings and many rounds (where they end is asserted in
    # test_short_periods_the_ring_wrap_and_round_cuts, on bytes made for it)
    "many rounds and ring wraps": (1 << 20, dict(), lambda s: sum(len(l) + m for l, _, m in s) > 10 * RING and len(s) > 8 * BATCH),
}


def _crafted_body(kind, codec, data):
    """The body for `data`; what the kind shows is asserted on the sequences of the body that is sent."""
    _, opts, shows = CRAFTED[kind]
    if codec == 7:
        body = L.encode(L.compress(data, **opts))
        blocks = [body]
    else:   # codec 5: three units, the middle one of two inner blocks, each piece compressed on its own
        n = len(data)
        cuts = [0, n // 4, n // 2, 3 * n // 4, n]
        blocks = [L.encode(L.compress(data[a:b], **opts)) for a, b in zip(cuts, cuts[1:])]
        body = L.hadoop([[blocks[0]], [blocks[1], blocks[2]], [blocks[3]]])
    assert shows([q for b in blocks for q in L.seqs_of(b)]), kind
    assert L.reference(body, len(data), L.HADOOP if codec == 5 else L.BARE) == data
    return body


@pytest.mark.parametrize("codec", [7, 5])
@pytest.mark.parametrize("kind", sorted(CRAFTED))
def test_crafted_pages_replay_alike(engine, base, tmp_path, kind, codec):
    """The first page of add.path and of add.stats, replaced by a body built here from the page's own bytes."""
    lp, ck = _variant(base, tmp_path, codec=codec, page_size=CRAFTED[kind][0])
    buf = open(ck, "rb").read()
    bodies = {}
    for leaf in ("add.path", "add.stats"):
        at, c, u, _ = L.lz4_pages(ck, leaf)[0]
        data = L.reference(buf[at:at + c], u, L.HADOOP if codec == 5 else L.BARE)
        assert data is not None and len(data) == u
        if leaf == "add.stats" and kind != "matches of four bytes":
            continue   # what the kind shows is asserted on add.path; add.stats takes the plain compressor
        bodies[(leaf, 0)] = (codec, _crafted_body(kind, codec, data))
    L.rewrite(ck, ck, bodies)
    _check(engine, base, lp)
    st, _, _ = _replay(engine, lp, base[3])
    ref, _, _ = _replay(engine, base[0], base[3])
    try:
        assert st.export(0) == ref.export(0)
    finally:
        st.release()
        ref.release()


def _periodic_table(table):
    """The checkpoint with add.stats replaced: every row's stats holds a run of "ab" and a run of "xyz", each
    longer than a wave, behind a number of its own."""
    import pyarrow as pa
    col = table.schema.get_field_index("add")
    add = table.column(col).combine_chunks()
    valid = add.is_valid().to_pylist()
    stats = pa.array(['{"numRecords":%07d,"tags":"%s%s"}' % (i, "ab" * 60, "xyz" * 40) if v else None
                      for i, v in enumerate(valid)], pa.string())
    k = add.type.get_field_index("stats")
    children = [stats if j == k else add.field(j) for j in range(add.type.num_fields)]
    new = pa.StructArray.from_arrays(children, fields=list(add.type), mask=pa.array([not v for v in valid]))
    return table.set_column(col, table.schema.field(col), new)


def _rounds(seqs, upto):
    """The kernel's rounds over [(literals, offset, length)] while every round ends because its span is full:
    [(sequences queued, input bytes walked, what is cut at the round's end: "match", "literals" or None)] for
    the rounds that start below output position `upto`. A round that fills SPAN bytes of output ends exactly
    there whatever the phase of its input, provided it queues fewer than BATCH sequences and walks less input
    than the window holds behind any 16-byte phase (4096 - 32 - 16)."""
    out, op, k, queued, walked = [], 0, 1, 0, 0
    for lits, off, ml in seqs:
        for part, n in (("literals", len(lits)), ("match", ml)):
            while op + n >= k * SPAN:          # this part reaches the round's end
                queued += 1
                out.append((queued, walked, part if op + n > k * SPAN else None))
                n -= k * SPAN - op
                op, k, queued, walked = k * SPAN, k + 1, 0, 0
                if op >= upto:
                    return out
            op += n
        queued += 1
        walked += len(L.encode([(lits, off, ml), (b"", 0, 0)])) - 1
    return out


@pytest.mark.parametrize("codec", [7, 5])
def test_short_periods_the_ring_wrap_and_round_cuts(engine, base, tmp_path, codec):
    """A table of its own: the checkpoint's add.stats holds "abab..." and "xyzxyz..." runs. Its first page is
    replaced by one block in which, asserted here on the block that is sent, (1) matches at offsets 2 and 3
    are longer than the 64 lanes, so the source index steps modulo the offset with a step that is not 0;
    (2) one match is written across the output positions [RING - 16, RING], where the ring index wraps for
    every 16-byte phase of the arena slot, and one match's source spans them; (3) the rounds up to there each
    end because their span of SPAN bytes is full, with a sequence cut in two at the end of every one of them,
    matches at offsets 2 and 3 among the ones cut. Export equals the SNAPPY twin's."""
    import pyarrow.parquet as pq
    table = _periodic_table(base[2])
    twin = base[:2] + (table,) + base[3:]
    lp0 = os.path.join(str(tmp_path), "snappy", "_delta_log")
    shutil.copytree(base[0], lp0)
    pq.write_table(table, os.path.join(lp0, base[1]), compression="snappy", use_dictionary=False, version="1.0",
                   write_statistics=False)
    lp, ck = _variant(twin, tmp_path / "lz4", codec=codec)
    at, c, u, _ = L.lz4_pages(ck, "add.stats")[0]
    data = L.reference(open(ck, "rb").read()[at:at + c], u, L.HADOOP if codec == 5 else L.BARE)
    assert data is not None and len(data) > RING + 2 * SPAN
    block = L.encode(L.compress(data, offsets=(2, 3), far_from=RING + 1))
    seqs = L.seqs_of(block)
    assert L.reference(block, len(data), L.BARE) == data
    # (1)
    assert any(off == 2 and ml > 64 for _, off, ml in seqs) and any(off == 3 and ml > 64 for _, off, ml in seqs)
    # (2)
    op, writes, reads = 0, False, False
    for lits, off, ml in seqs:
        op += len(lits)
        writes |= op < RING - 16 and op + ml > RING
        reads |= off >= 17 and op - off < RING - 16 and op - off + min(off, ml) > RING
        op += ml
    assert writes and reads
    # (3)
    rounds = _rounds(seqs, RING + SPAN)
    assert len(rounds) >= RING // SPAN + 1
    assert all(q < BATCH and walked < 4096 - 48 and cut for q, walked, cut in rounds), rounds
    assert {"match", "literals"} >= {cut for _, _, cut in rounds} and "match" in {cut for _, _, cut in rounds}
    op, cut_offsets = 0, set()
    for lits, off, ml in seqs:
        op += len(lits)
        if ml and op // SPAN != (op + ml - 1) // SPAN and (op + ml) % SPAN and op < RING + SPAN:
            cut_offsets.add(off)
        op += ml
    assert cut_offsets & {2, 3}, cut_offsets
    L.rewrite(ck, ck, {("add.stats", 0): (codec, block if codec == 7 else L.hadoop([[block]]))})
    st, _, _ = _replay(engine, lp, base[3])
    ref, _, _ = _replay(engine, lp0, base[3])
    try:
        live = ref.export(0)
        assert st.export(0) == live and st.export(1) == ref.export(1)
        assert sum("ab" * 60 + "xyz" * 40 in (a.get("stats") or "") for a in live) > 1000
    finally:
        st.release()
        ref.release()


@pytest.mark.parametrize("codec", [7, 5])
def test_incompressible_pages_become_copies(engine, base, tmp_path, codec):
    """Pages stored as one literal run per block -- what a compressor writes when it cannot shrink a page;
    add.size is given that form here, since LZ4 does shrink this table's sizes -- report under copy_bytes,
    not lz4_pages."""
    lp, ck = _variant(base, tmp_path, codec=codec, page_size=4096)
    before = _hot_pages(ck)
    buf = open(ck, "rb").read()
    stored = {}
    for k, (at, c, u, _) in enumerate(L.lz4_pages(ck, "add.size")):
        data = L.reference(buf[at:at + c], u, L.HADOOP if codec == 5 else L.BARE)
        half = len(data) // 2
        stored[("add.size", k)] = (codec, L.encode([(data, 0, 0)]) if codec == 7 else
                                   L.hadoop([[L.encode([(data[:half], 0, 0)])], [L.encode([(data[half:], 0, 0)])]]))
    L.rewrite(ck, ck, stored)
    pages, copies = _hot_pages(ck)
    size = [p for p in L.lz4_pages(ck, "add.size") if p[2] > 0]
    assert len(size) > 10 and all(p in copies for p in size) and len(pages) == len(before[0]) + len(before[1]) - len(copies)
    plan = _check(engine, base, lp)
    _assert_plan(plan, ck)
    assert plan["copy_bytes"] >= sum(p[2] for p in copies)


def _refused(engine, base, lp):
    from delta_amd.delta_log import DeltaError
    with pytest.raises(DeltaError) as e:
        staged = engine.stage_log(lp)
        try:
            staged.replay(base[3]).release()
        finally:
            staged.release()
    assert e.value.code == "DR_E_PARQUET" and "lz4 page in add.path" in str(e.value), str(e.value)


@pytest.mark.parametrize("framing", [L.BARE, L.HADOOP])
def test_malformed_pages_are_refused(engine, base, tmp_path, framing):
    """One page per refusal of lz4_fmt.h, each in a table of its own: the first page of add.path, replaced by a
    body made for that page's size."""
    codec = 5 if framing == L.HADOOP else 7
    lp0, ck0 = _variant(base, tmp_path / "good", codec=codec, page_size=4096)
    size = L.lz4_pages(ck0, "add.path")[0][2]
    assert size > 340
    bodies = malformed_bodies(framing, size)
    assert sorted(bodies) == MALFORMED[framing] and len(bodies) >= 11
    for k, kind in enumerate(MALFORMED[framing]):
        assert L.reference(bodies[kind], size, framing) is None or kind == "offset 0"
        lp = os.path.join(str(tmp_path), "bad%d" % k, "_delta_log")
        shutil.copytree(lp0, lp)
        L.rewrite(ck0, os.path.join(lp, os.path.basename(ck0)), {("add.path", 0): (codec, bodies[kind])})
        _refused(engine, base, lp)
    _check(engine, base, lp0)   # the engine replays a good table afterwards


def test_nothing_for_tables_without_lz4(engine, base, tmp_path):
    st, plan, names = _replay(engine, base[0], base[3], timing=True)
    st.release()
    assert "k_snap_exec" in names and not [k for k in names if k.startswith("k_lz4")], sorted(names)
    assert plan["lz4_pages"] == 0 and plan["lz4_in_bytes"] == 0 and plan["lz4_out_bytes"] == 0
    lp, _ = _variant(base, tmp_path)
    st, plan, names = _replay(engine, lp, base[3], timing=True)
    st.release()
    assert "k_lz4" in names and plan["lz4_pages"] > 0, sorted(names)
