"""ZSTD-compressed checkpoint pages on the device (k_zstd): replays of checkpoints pyarrow wrote with
compression="zstd" equal the oracle record for record across page sizes, page versions, dictionary use
and compression levels; export, filter, lookup and scan order answer as on the SNAPPY twin; chunks of
one file may mix codecs; page bodies replaced in place by re-framed streams (several frames, skippable
frames, a Window_Descriptor without a content size, a content checksum, Raw and RLE blocks in front of
compressed ones, every Frame_Content_Size width) replay alike; malformed bodies -- each refused by the
host decoder under the sanitizers in tests/test_zstd_host.py first -- end in DR_E_PARQUET naming the
column; a table without ZSTD pages pays nothing.

The logical table is one (config 3 at scale 0.001, seed 3, about 16 K actions): it is built once, the
oracle reads it once, and each case rewrites only the checkpoint file. pyarrow cuts pages per write
batch, so the 4 KiB cases write batches of 32 rows to get pages that small."""
import os
import shutil

import numpy as np
import pytest

from oracle import delta_oracle as O
from tests import filter_corpus as F
from tests import zstd_corpus as Z
from tests.test_gpu_parity import _assert_same
from tests.test_zstd_host import MALFORMED, malformed_bodies

pytestmark = pytest.mark.gpu

HOT = ("add.path", "add.size", "remove.path", "remove.deletionTimestamp")


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
    d = str(tmp_path_factory.mktemp("zs_base"))
    exp = S.build_table(d, S.config_spec(3, 0.001), seed=3)
    lp = os.path.join(d, "_delta_log")
    ck = [f for f in os.listdir(lp) if f.endswith(".checkpoint.parquet")]
    assert len(ck) == 1
    cutoff = exp.min_file_retention_timestamp
    return lp, ck[0], pq.read_table(os.path.join(lp, ck[0])), cutoff, O.state_reconstruction(O.get_log_segment(lp), cutoff)


def _variant(base, d, compression="zstd", level=None, page_size=1 << 20, version="1.0", dictionary=False):
    """A copy of the base log whose checkpoint is rewritten; (log path, checkpoint path)."""
    import pyarrow.parquet as pq
    lp0, ck, table = base[:3]
    lp = os.path.join(str(d), "_delta_log")
    shutil.copytree(lp0, lp)
    kw = {"compression_level": level} if level is not None else {}
    if page_size < 65536:
        kw["write_batch_size"] = 32
    pq.write_table(table, os.path.join(lp, ck), compression=compression, use_dictionary=dictionary, version="1.0",
                   data_page_version=version, data_page_size=page_size, write_statistics=False, **kw)
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


@pytest.mark.parametrize("level", [1, 19])
@pytest.mark.parametrize("dictionary", [False, True])
@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("page_size", [4096, 1 << 20])
def test_parity(engine, base, tmp_path, page_size, version, dictionary, level):
    """Fails on a build without the decoder with DR_E_UNSUPPORTED (checkpoint codec 6)."""
    lp, ck = _variant(base, tmp_path, level=level, page_size=page_size, version=version, dictionary=dictionary)
    plan = _check(engine, base, lp)
    pages = [p for leaf in HOT for p in Z.zstd_pages(ck, leaf)]
    assert plan["zstd_pages"] == len([p for p in pages if p[1] or p[2]]) > 0
    assert plan["zstd_out_bytes"] == sum(u for _, _, u in pages)
    assert plan["zstd_in_bytes"] == sum(c for _, c, _ in pages)
    if page_size == 4096 and not dictionary:
        assert len(pages) > 100   # pages of a few KiB, not one per leaf


def test_export_filter_lookup_and_scan_order_as_on_the_snappy_twin(engine, base, tmp_path):
    from delta_amd.predicates import build_program, partition_schema
    lp, _ = _variant(base, tmp_path, page_size=4096, version="2.0")
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
    codec = {"add.path": "zstd", "add.size": "snappy", "remove.path": "none", "remove.deletionTimestamp": "gzip",
             "add.stats": "zstd", "add.modificationTime": "gzip"}
    md = pq.ParquetFile(os.path.join(base[0], base[1])).metadata
    names = [md.row_group(0).column(i).path_in_schema for i in range(md.num_columns)]
    lp, ck = _variant(base, tmp_path, compression={n: codec.get(n, ("zstd", "snappy", "gzip")[len(n) % 3]) for n in names})
    plan = _check(engine, base, lp)
    assert plan["zstd_pages"] > 0 and plan["gzip_pages"] > 0 and plan["snappy_in_bytes"] > 0 and plan["copy_bytes"] > 0


def _l19(data):
    return Z.one_shot(data, 19)


def _fcs(width):
    return lambda data: Z.reheader(_l19(data), data, fcs=width, single=width != 0)


def _front(width, n):
    """A first frame of n bytes of `data` as Raw blocks whose Frame_Content_Size field is `width` bytes
    wide (1: up to 255 bytes; 2: 256 to 65,791, stored minus 256), then a level-19 frame of the rest."""
    return lambda data: Z.frame(Z.raw_blocks(data[:n]), data[:n], fcs=width, single=True) + _l19(data[n:])


CRAFTED = {
    "two frames": lambda data: _l19(data[:len(data) // 3]) + _l19(data[len(data) // 3:]),
    "skippable frames": lambda data: Z.skippable(b"abc") + _l19(data[:len(data) // 3]) + Z.skippable(b"", 5) +
    Z.skippable(b"\0" * 20, 15) + _l19(data[len(data) // 3:]) + Z.skippable(b"tail"),
    "window descriptor, no content size": lambda data: Z.reheader(_l19(data), data, fcs=0),
    "checksum": lambda data: Z.reheader(_l19(data), data, fcs=0, checksum=True),
    "raw and rle blocks, then compressed": Z.raw_rle_then_compressed,
    "fcs 1": _front(1, 200),
    "fcs 2": _front(2, 3000),
    "fcs 4": _fcs(4),
    "fcs 8": _fcs(8),
}
# what each crafted body must show when walked, so that no case falls back to another silently
SHOWS = {"two frames": {"frame:single"}, "skippable frames": {"frame:skippable"},
         "window descriptor, no content size": {"fcs:0", "frame:window"}, "checksum": {"frame:checksum"},
         "raw and rle blocks, then compressed": {"block:raw", "block:rle", "block:compressed"},
         "fcs 1": {"fcs:1"}, "fcs 2": {"fcs:2"}, "fcs 4": {"fcs:4"}, "fcs 8": {"fcs:8"}}


def crafted_page(kind, data, size):
    body = Z.refit(CRAFTED[kind](data), data, size)
    frames, feats, _ = Z.walk(body)
    assert SHOWS[kind] <= feats, (kind, sorted(feats))
    if kind == "two frames":
        assert len([f for f in frames if not f["skippable"]]) == 2
    return body


@pytest.mark.parametrize("kind", sorted(CRAFTED))
def test_crafted_pages_replay_alike(engine, base, tmp_path, kind):
    """The first page of add.path and of add.stats, replaced at equal size (level-19 output is shorter
    than the level-1 body it replaces; a skippable frame absorbs the difference)."""
    lp, ck = _variant(base, tmp_path, level=1)
    for leaf in ("add.path", "add.stats"):
        Z.replace_page(ck, ck, leaf, 0, lambda data, size: crafted_page(kind, data, size))
    _check(engine, base, lp)
    st, _, _ = _replay(engine, lp, base[3])
    ref, _, _ = _replay(engine, base[0], base[3])
    try:
        assert st.export(0) == ref.export(0)
    finally:
        st.release()
        ref.release()


def malformed_page(kind, data, size):
    body = malformed_bodies(size)[kind]
    assert len(body) == size and Z.reference(body, len(data)) is None
    return body


@pytest.mark.parametrize("kind", MALFORMED)
def test_malformed_pages_are_refused(engine, base, tmp_path, kind):
    from delta_amd.delta_log import DeltaError
    lp, ck = _variant(base, tmp_path, level=1)
    Z.replace_page(ck, ck, "add.path", 0, lambda data, size: malformed_page(kind, data, size))
    with pytest.raises(DeltaError) as e:
        staged = engine.stage_log(lp)
        try:
            staged.replay(base[3]).release()
        finally:
            staged.release()
    assert e.value.code == "DR_E_PARQUET" and "zstd page in add.path" in str(e.value), str(e.value)
    _check(engine, base, base[0])   # the engine replays a good table afterwards


def wrong_checksum_page(data, size):
    """The page's own content under a content checksum with one bit flipped: right in length and in every
    byte, so that only the checksum comparison can refuse it."""
    good = Z.refit(Z.reheader(_l19(data), data, fcs=4, single=True, checksum=True), data, size)
    body = good[:-1] + bytes([good[-1] ^ 0x10])
    assert Z.walk(good)[0][-1]["checksum"] and Z.reference(body, len(data)) is None
    return body


def test_a_wrong_checksum_on_a_page_of_the_right_length_is_refused(engine, base, tmp_path):
    from delta_amd.delta_log import DeltaError
    lp, ck = _variant(base, tmp_path, level=1)
    Z.replace_page(ck, ck, "add.path", 0, wrong_checksum_page)
    with pytest.raises(DeltaError) as e:
        staged = engine.stage_log(lp)
        try:
            staged.replay(base[3]).release()
        finally:
            staged.release()
    assert e.value.code == "DR_E_PARQUET" and "zstd page in add.path" in str(e.value), str(e.value)


def test_nothing_for_tables_without_zstd(engine, base, tmp_path):
    st, plan, names = _replay(engine, base[0], base[3], timing=True)
    st.release()
    assert "k_snap_exec" in names and not [k for k in names if k.startswith("k_zstd")], sorted(names)
    assert plan["zstd_pages"] == 0 and plan["zstd_in_bytes"] == 0 and plan["zstd_out_bytes"] == 0
    lp, _ = _variant(base, tmp_path)
    st, plan, names = _replay(engine, lp, base[3], timing=True)
    st.release()
    assert "k_zstd" in names and plan["zstd_pages"] > 0, sorted(names)
