"""DELTA_BINARY_PACKED, DELTA_LENGTH_BYTE_ARRAY and DELTA_BYTE_ARRAY checkpoint pages on the device
(k_dl_scan, k_dl_fc_last, k_dl_fc_fill, k_pq_data_dl): replays of checkpoints whose leaves pyarrow wrote
with those encodings equal the oracle record for record, across page versions, codecs and page sizes;
the export decode, dr_filter and dr_state_lookup_paths answer as on the PLAIN twin of the table; a
PLAIN checkpoint pays nothing for the feature; malformed pages end in DR_E_PARQUET."""
import os

import numpy as np
import pytest

from oracle import delta_oracle as O
from tests import delta_pages_corpus as C
from tests import filter_corpus as F
from tests.test_gpu_parity import _assert_same

pytestmark = pytest.mark.gpu

PATHS7 = {"add.path": "DELTA_BYTE_ARRAY", "remove.path": "DELTA_BYTE_ARRAY"}
PATHS6 = {"add.path": "DELTA_LENGTH_BYTE_ARRAY", "remove.path": "DELTA_LENGTH_BYTE_ARRAY"}
INTS5 = {k: "DELTA_BINARY_PACKED" for k in ("add.size", "add.modificationTime", "remove.deletionTimestamp", "remove.size",
                                            "txn.version", "txn.lastUpdated", "metaData.createdTime",
                                            "protocol.minReaderVersion", "protocol.minWriterVersion")}
MAPS = ("partitionValues", "tags")
EVERY = dict(PATHS7, **INTS5)
EVERY.update({"add.stats": "DELTA_BYTE_ARRAY", "metaData.schemaString": "DELTA_LENGTH_BYTE_ARRAY",
              "metaData.id": "DELTA_BYTE_ARRAY", "txn.appId": "DELTA_BYTE_ARRAY"})
for side in ("add", "remove"):
    for m in MAPS:
        EVERY["%s.%s.key_value.key" % (side, m)] = "DELTA_BYTE_ARRAY"
        EVERY["%s.%s.key_value.value" % (side, m)] = "DELTA_LENGTH_BYTE_ARRAY"


@pytest.fixture(scope="module")
def engine():
    from delta_amd.delta_log import Engine
    return Engine.get(0)


def _replay(engine, lp, cutoff, timing=False):
    """(state, the staged plan's figures after the replay, kernel names launched when timing)."""
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


def _table(d, enc, **kw):
    from delta_amd.testing import synth as S
    exp = S.build_table(d, S.config_spec(3, 0.001), seed=3, use_dictionary=False, column_encoding=enc, **kw)
    return os.path.join(d, "_delta_log"), exp


def _check(engine, lp, cutoff, delta_pages=True):
    st, plan, _ = _replay(engine, lp, cutoff)
    try:
        _assert_same(st, O.state_reconstruction(O.get_log_segment(lp), cutoff))
        assert plan["delta_pages_serial"] == 0
        assert (plan["delta_pages"] > 0) == delta_pages
    finally:
        st.release()
    return plan


@pytest.mark.parametrize("page_size", [4096, 1 << 20])
@pytest.mark.parametrize("codec", ["snappy", "none"])
@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("enc", [PATHS7, PATHS6, INTS5], ids=["paths7", "paths6", "ints5"])
def test_parity(engine, tmp_path, enc, version, codec, page_size):
    lp, exp = _table(str(tmp_path), enc, data_page_version=version, compression=codec, data_page_size=page_size)
    plan = _check(engine, lp, exp.min_file_retention_timestamp)
    assert plan["delta_sizing_passes"] == (1 if enc is PATHS7 else 0)


def test_export_filter_and_lookup_as_on_the_plain_twin(engine, tmp_path):
    from delta_amd.predicates import build_program, partition_schema
    lp, exp = _table(str(tmp_path / "delta"), EVERY, data_page_version="2.0", data_page_size=4096)
    lp0, _ = _table(str(tmp_path / "plain"), None, data_page_version="2.0", data_page_size=4096)
    cutoff = exp.min_file_retention_timestamp
    _check(engine, lp, cutoff)
    st, _, _ = _replay(engine, lp, cutoff)
    ref, _, _ = _replay(engine, lp0, cutoff)
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
    finally:
        st.release()
        ref.release()


def _log_around(d, ckpt_writer, version=1):
    """A _delta_log holding one checkpoint (written by ckpt_writer(path) -> rows) and its commit."""
    from delta_amd.testing import synth as S
    lp = os.path.join(d, "_delta_log")
    os.makedirs(lp)
    rows = ckpt_writer(os.path.join(lp, "%020d.checkpoint.parquet" % version))
    with open(os.path.join(lp, "_last_checkpoint"), "w") as f:
        f.write('{"version":%d,"size":%d}\n' % (version, rows))
    with open(os.path.join(lp, S.delta_name(version)), "w") as f:
        f.write(S.commit_info_line(version) + "\n")
    return lp


def _records(n_adds):
    from delta_amd.testing import synth as S
    def size(i):   # 0, 2^31 and (once: the sum stays inside 64 bits) 2^62 among ordinary sizes
        return (1 << 62) if i == 5 else (1 << 31) + i if i % 3 == 1 else 0 if i % 3 == 0 else i
    adds, removes = [], []
    for i in range(n_adds):
        if 1200 <= i < 1300:   # a run without any shared prefix
            path = "%c%c-%05d.parquet" % (chr(48 + i % 10), chr(97 + (i // 10) % 26), i)
        else:                  # one prefix over far more than 1,025 consecutive values
            path = "p0=2020-01-01/p1=3/part-%05d-c000.snappy.parquet" % i
        adds.append({"path": path, "partitionValues": {"p0": "2020-01-01", "p1": "3"}, "size": size(i),
                     "modificationTime": 1_600_000_000_000 + i, "stats": '{"numRecords":%d}' % i})
        removes.append({"path": "gone/" + path, "deletionTimestamp": 1_600_000_000_000 + 7 * i, "size": i})
    protocol = {"minReaderVersion": 1, "minWriterVersion": 2}
    return protocol, S.metadata_dict(2), adds, removes


def test_page_shapes(engine, tmp_path):
    """Pages of exactly 1, 64, 65, 1024 and 1025 values (the 64-value group and 1024-level segment
    edges) and a longer one, adds and removes interleaved row by row (each path column half null),
    sizes 0, 2^31 and 2^62, a prefix shared by more than 1,025 values in a row, a run of prefix 0."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from delta_amd.testing import synth as S
    shapes = [1, 64, 65, 1024, 1025, 1400]
    n = sum(shapes)
    protocol, metadata, adds, removes = _records(n)

    def writer(path):
        tmp = str(tmp_path / "flat.parquet")
        S.write_checkpoint_records(tmp, protocol, metadata, adds, removes, use_dictionary=False)
        t = pq.read_table(tmp)
        order = [0, 1] + [2 + i + k * n for i in range(n) for k in (0, 1)]
        t = t.take(pa.array(order))
        with pq.ParquetWriter(path, t.schema, version="1.0", compression="snappy", use_dictionary=False,
                              write_statistics=False, data_page_size=1 << 22, column_encoding=EVERY) as w:
            at = 0
            for k, adds_here in enumerate(shapes):   # one row group, so one page per leaf, per shape
                rows = 2 * adds_here + (2 if k == 0 else 0)
                w.write_table(t.slice(at, rows), row_group_size=rows)
                at += rows
        md = pq.ParquetFile(path).metadata
        assert [md.row_group(g).num_rows for g in range(md.num_row_groups)] == [4, 128, 130, 2048, 2050, 2800]
        return t.num_rows

    lp = _log_around(str(tmp_path / "t"), writer)
    plan = _check(engine, lp, 0)
    assert plan["delta_sizing_passes"] == 1 and plan["delta_arena_bytes"] > 0


def test_mixed_parts(engine, tmp_path):
    """Part 1 PLAIN + dictionary pages, part 2 delta pages, one checkpoint."""
    import dataclasses
    import pyarrow.parquet as pq
    from delta_amd.testing import synth as S
    d = str(tmp_path)
    spec = dataclasses.replace(S.config_spec(3, 0.001), ckpt_parts=2)
    exp = S.build_table(d, spec, seed=5)
    lp = os.path.join(d, "_delta_log")
    part2 = [f for f in sorted(os.listdir(lp)) if ".checkpoint.0000000002." in f]
    assert len(part2) == 1
    t = pq.read_table(os.path.join(lp, part2[0]))
    pq.write_table(t, os.path.join(lp, part2[0]), compression="snappy", use_dictionary=False, version="1.0",
                   data_page_version="2.0", write_statistics=False, column_encoding=EVERY)
    _check(engine, lp, exp.min_file_retention_timestamp)


def test_plain_checkpoint_pays_nothing(engine, tmp_path):
    """No delta kernel is launched and no sizing read-back made for a checkpoint without delta pages."""
    lp, exp = _table(str(tmp_path / "plain"), None)
    st, plan, names = _replay(engine, lp, exp.min_file_retention_timestamp, timing=True)
    st.release()
    assert "k_pq_data" in names and not [k for k in names if k.startswith("k_dl_") or k == "k_pq_data_dl"], sorted(names)
    assert plan["delta_pages"] == 0 and plan["delta_sizing_passes"] == 0 and plan["delta_arena_bytes"] == 0
    lp7, exp7 = _table(str(tmp_path / "delta"), PATHS7)
    st, plan, names = _replay(engine, lp7, exp7.min_file_retention_timestamp, timing=True)
    st.release()
    assert {"k_dl_scan", "k_dl_fc_last", "k_dl_fc_fill", "k_pq_data_dl"} <= names, sorted(names)


def test_sizing_runs_once_per_staged_segment(engine, tmp_path):
    lp, exp = _table(str(tmp_path), PATHS7)
    staged = engine.stage_log(lp)
    try:
        assert staged.plan()["delta_sizing_passes"] == 0
        sums = []
        for _ in range(3):
            st = staged.replay(exp.min_file_retention_timestamp)
            sums.append(st.record_sums())
            st.release()
        assert staged.plan()["delta_sizing_passes"] == 1 and sums[0] == sums[1] == sums[2]
    finally:
        staged.release()


@pytest.mark.parametrize("kind", ["width65", "count+1", "prefix>prev"])
def test_malformed_pages_are_refused(engine, tmp_path, kind):
    from delta_amd.delta_log import DeltaError
    from delta_amd.testing import synth as S
    protocol, metadata, adds, _ = _records(40)

    def writer(path):
        good = str(tmp_path / "good.parquet")
        rows = S.write_checkpoint_records(good, protocol, metadata, adds, use_dictionary=False, compression="none",
                                          column_encoding=PATHS7)
        C.patch(good, path, "add.path", kind, 40, 0)
        return rows

    lp = _log_around(str(tmp_path / "t"), writer)
    staged = engine.stage_log(lp)
    try:
        with pytest.raises(DeltaError) as e:
            staged.replay(0).release()
        assert e.value.code == "DR_E_PARQUET"
    finally:
        staged.release()


def test_byte_stream_split_is_still_refused(engine, tmp_path):
    import pyarrow.parquet as pq
    from delta_amd.delta_log import DeltaError
    lp, _ = _table(str(tmp_path), None)
    ck = [f for f in os.listdir(lp) if f.endswith(".checkpoint.parquet")][0]
    t = pq.read_table(os.path.join(lp, ck))
    pq.write_table(t, os.path.join(lp, ck), compression="snappy", use_dictionary=False, version="1.0",
                   write_statistics=False, column_encoding={"add.size": "BYTE_STREAM_SPLIT"})
    with pytest.raises(DeltaError) as e:
        engine.stage_log(lp).release()
    assert e.value.code == "DR_E_UNSUPPORTED"
