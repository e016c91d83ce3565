"""GZIP-compressed checkpoint pages on the device (k_inflate): replays of checkpoints pyarrow wrote
with compression="gzip" equal the oracle record for record across page sizes, page versions,
dictionary use and compression levels; export, filter, lookup and scan order answer as on the SNAPPY
twin; chunks of one file may mix codecs; page bodies replaced in place by hand-built streams (several
members, optional header fields, the fixed code, a full flush, a stored block followed by a
continuation that reaches back into it) replay alike; malformed bodies -- each refused by the host
inflater under the sanitizers in tests/test_inflate_host.py first -- end in DR_E_PARQUET naming the
column; a table without GZIP pages pays nothing.

The logical table is one (config 3 at scale 0.001, seed 3, about 16 K actions): it is built once, the
oracle reads it once, and each case rewrites only the checkpoint file. pyarrow cuts pages per write
batch, so the 4 KiB cases write batches of 32 rows to get pages that small (well over a hundred in the hot leaves)."""
import os
import shutil
import zlib

import numpy as np
import pytest

from oracle import delta_oracle as O
from tests import filter_corpus as F
from tests import inflate_corpus as I
from tests.test_gpu_parity import _assert_same
from tests.test_inflate_host import malformed_bodies

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
    d = str(tmp_path_factory.mktemp("gz_base"))
    exp = S.build_table(d, S.config_spec(3, 0.001), seed=3)
    lp = os.path.join(d, "_delta_log")
    ck = [f for f in os.listdir(lp) if f.endswith(".checkpoint.parquet")]
    assert len(ck) == 1
    cutoff = exp.min_file_retention_timestamp
    return lp, ck[0], pq.read_table(os.path.join(lp, ck[0])), cutoff, O.state_reconstruction(O.get_log_segment(lp), cutoff)


def _variant(base, d, compression="gzip", level=None, page_size=1 << 20, version="1.0", dictionary=False):
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


@pytest.mark.parametrize("level", [1, 9])
@pytest.mark.parametrize("dictionary", [False, True])
@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("page_size", [4096, 1 << 20])
def test_parity(engine, base, tmp_path, page_size, version, dictionary, level):
    """Fails on a build without the inflater with DR_E_UNSUPPORTED (checkpoint codec 2)."""
    lp, ck = _variant(base, tmp_path, level=level, page_size=page_size, version=version, dictionary=dictionary)
    plan = _check(engine, base, lp)
    pages = [p for leaf in HOT for p in I.gzip_pages(ck, leaf)]
    assert plan["gzip_pages"] == len([p for p in pages if p[1] or p[2]]) > 0
    assert plan["gzip_out_bytes"] == sum(u for _, _, u in pages)
    assert plan["gzip_in_bytes"] == sum(c for _, c, _ in pages)
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
    codec = {"add.path": "gzip", "add.size": "snappy", "remove.path": "none", "remove.deletionTimestamp": "gzip",
             "add.stats": "snappy", "add.modificationTime": "gzip"}
    names = [c.path_in_schema for c in (pq.ParquetFile(os.path.join(base[0], base[1])).metadata.row_group(0).column(i)
                                        for i in range(pq.ParquetFile(os.path.join(base[0], base[1])).metadata.num_columns))]
    lp, ck = _variant(base, tmp_path, compression={n: codec.get(n, "gzip" if len(n) % 2 else "snappy") for n in names})
    plan = _check(engine, base, lp)
    assert plan["gzip_pages"] > 0 and plan["snappy_in_bytes"] + plan["copy_bytes"] > 0


def _fixed_then_l9(data, extra):
    cut = len(data) // 8
    return I.member(data[:cut], flags=I.FEXTRA, extra=extra, strategy=zlib.Z_FIXED) + I.member(data[cut:], level=9)


CRAFTED = {
    "two members": lambda data, extra: I.member(data[:len(data) // 3], flags=I.FEXTRA, extra=extra, level=9) +
    I.member(data[len(data) // 3:], level=9),
    "fname+fhcrc+fextra": lambda data, extra: I.member(data, flags=I.FEXTRA | I.FNAME | I.FHCRC, extra=extra, level=9),
    "fixed code": _fixed_then_l9,
    "full flush": lambda data, extra: I.member(data, flags=I.FEXTRA, extra=extra, full_flush=True, level=9),
    "stored+zdict": lambda data, extra: I.member(data, flags=I.FEXTRA, extra=extra,
                                                 raw=I.stored_then_zdict(data, level=9, cut=64)),
}


@pytest.mark.parametrize("kind", sorted(CRAFTED))
def test_crafted_pages_replay_alike(engine, base, tmp_path, kind):
    """The first page of add.path and of add.stats, replaced at equal size (level-9 output is shorter
    than the level-1 body it replaces; a FEXTRA field absorbs the difference)."""
    lp, ck = _variant(base, tmp_path, level=1)
    for leaf in ("add.path", "add.stats"):
        I.replace_page(ck, ck, leaf, 0, lambda data, size: I.refit(lambda extra: CRAFTED[kind](data, extra), data, size))
    _check(engine, base, lp)
    st, _, _ = _replay(engine, lp, base[3])
    ref, _, _ = _replay(engine, base[0], base[3])
    try:
        assert st.export(0) == ref.export(0)
    finally:
        st.release()
        ref.release()


MALFORMED = ["block type 3", "stored NLEN mismatch", "over-subscribed code lengths", "distance before the member's start",
             "ISIZE off by one", "last 16 bytes zeroed", "bad magic", "zlib wrapper", "trailer cut", "reserved flag",
             "second member bad", "distance code 30"]


@pytest.mark.parametrize("kind", MALFORMED)
def test_malformed_pages_are_refused(engine, base, tmp_path, kind):
    from delta_amd.delta_log import DeltaError
    lp, ck = _variant(base, tmp_path, level=1)

    def make(data, size):   # the body keeps the page's length: a FEXTRA field absorbs the difference
        base_len = len(malformed_bodies(data, b"")[kind])
        assert base_len <= size, (base_len, size)
        body = malformed_bodies(data, b"\0" * (size - base_len))[kind]
        assert len(body) == size and I.reference(body, len(data)) is None
        return body

    I.replace_page(ck, ck, "add.path", 0, make)
    with pytest.raises(DeltaError) as e:
        staged = engine.stage_log(lp)
        try:
            staged.replay(base[3]).release()
        finally:
            staged.release()
    assert e.value.code == "DR_E_PARQUET" and "gzip page in add.path" in str(e.value), str(e.value)
    _check(engine, base, base[0])   # the engine replays a good table afterwards


def test_nothing_for_tables_without_gzip(engine, base, tmp_path):
    st, plan, names = _replay(engine, base[0], base[3], timing=True)
    st.release()
    assert "k_snap_exec" in names and not [k for k in names if k.startswith("k_inflate")], sorted(names)
    assert plan["gzip_pages"] == 0 and plan["gzip_in_bytes"] == 0 and plan["gzip_out_bytes"] == 0
    lp, _ = _variant(base, tmp_path)
    st, plan, names = _replay(engine, lp, base[3], timing=True)
    st.release()
    assert "k_inflate" in names and plan["gzip_pages"] > 0, sorted(names)
