"""The writer-shape matcher in the bulk K1 kernel (k_json_lines<false>, walk_line): lanes whose line
match_writer_line accepts skip the DFA, the others step it over the same tokens, and a wave that
flushed its token buffer mid-line keeps the DFA for every lane.

Three commits, each replayed behind a 320-line first commit (five whole waves, so the segment takes
the bulk kernel and the commit under test starts a wave):
 * 65 writer-shaped adds and removes with two partition columns: one whole wave on the matcher and
   one lane of the next;
 * 130 lines of which every eighth is one the matcher declines (a reordered member, a duplicate
   key, an escaped key that k_json_hard decides, metaData, commitInfo, a blank line, a malformed line):
   accepted and declined lanes in one wave;
 * 64 lines whose lane 17 has six partition columns (more than the 22 tokens of the flush mark): the
   whole wave flushes mid-line and takes the DFA.
Each is compared with the oracle through the normal Engine path (full records, counters, record
hashes, malformed_lines), line by line with the PERMISSIVE-reader restatement (tests/test_json_lane.py
`expected`), and again with the context option json_staged=1 (the staged instantiation). A line
with "path":null is only in the line-by-line comparison: the oracle, like the reference's AddFile,
does not take a null path.
"""

import numpy as np
import pytest

from oracle import delta_oracle as O

pytestmark = pytest.mark.gpu

HEAD = [b'{"protocol":{"minReaderVersion":1,"minWriterVersion":2}}',
        b'{"metaData":{"id":"shape","format":{"provider":"parquet","options":{}},"schemaString":"{}",'
        b'"partitionColumns":["p0","p1"],"configuration":{}}}']
FILL = 318  # HEAD + FILL = 320 lines = 5 waves


@pytest.fixture(scope="module")
def engine():
    from delta_amd.delta_log import Engine
    return Engine.get(0)


@pytest.fixture(scope="module")
def writer():
    """(adds, removes): 700 writer lines each over one file pool, two partition columns."""
    from delta_amd.testing import synth as S
    pool = S.FilePool(np.random.default_rng(11), 700, 2)
    ids = np.arange(700)
    adds = S._text_bytes(S.add_lines(pool, ids, 1700000000000 + ids)).split(b"\n")[:-1]
    rms = S._text_bytes(S.remove_lines(pool, ids, 1700000100000 + ids)).split(b"\n")[:-1]
    return adds, rms


def _pure(writer):
    adds, rms = writer
    # removes of files the first commit added, and new adds, interleaved
    return [rms[i] if i % 3 == 0 else adds[FILL + i] for i in range(65)]


def _mixed(writer, with_null_path):
    from tests.test_json_shape import members, _join
    adds, rms = writer
    lines = [rms[100 + i] if i % 2 else adds[FILL + 100 + i] for i in range(130)]

    def reordered(x):
        h, m, t = members(x)
        m[2], m[3] = m[3], m[2]
        return _join(h, m, t)

    odd = [reordered(lines[0]),
           lines[8].replace(b',"modificationTime"', b',"size":77,"modificationTime"'),
           lines[16].replace(b'"path":"', b'"path":null,"x":"') if with_null_path else lines[16],
           lines[24].replace(b'"path"', b'"p\\u0061th"'),
           HEAD[1].replace(b'"configuration":{}', b'"configuration":{"k":"v"}'),
           b'{"commitInfo":{"timestamp":1700000000000,"operation":"WRITE"}}',
           b"",
           b'{"add":{"path":"broken.parquet","size":1']
    for k, x in enumerate(odd * 3):
        if 8 * k < len(lines):
            lines[8 * k] = x
    return lines


def _flushed(writer):
    adds, _ = writer
    lines = [adds[FILL + 300 + i] for i in range(64)]
    lines[17] = lines[17].replace(b'"partitionValues":{', b'"partitionValues":{"a":"1","b":null,"c":"3","d":"4",')
    return lines


CASES = {"pure": _pure, "mixed": lambda w: _mixed(w, False), "flushed": _flushed}


def _write_log(tmp_path, writer, lines):
    lp = tmp_path / "_delta_log"
    lp.mkdir()
    (lp / ("%020d.json" % 0)).write_bytes(b"\n".join(HEAD + writer[0][:FILL]) + b"\n")
    (lp / ("%020d.json" % 1)).write_bytes(b"\n".join(lines) + b"\n")
    return str(lp)


@pytest.fixture(params=[0, 1], ids=["bulk", "staged"])
def staged_option(request, engine):
    engine.set_option("json_staged", request.param)
    request.addfinalizer(lambda: engine.set_option("json_staged", 0))
    return request.param


@pytest.mark.parametrize("case", sorted(CASES))
def test_replay_equals_the_oracle(engine, writer, tmp_path, staged_option, case):
    from delta_amd import _native as N
    from tests.test_gpu_parity import _assert_same, _gpu_replay
    lines = CASES[case](writer)
    assert len(lines) == {"pure": 65, "mixed": 130, "flushed": 64}[case]
    lp = _write_log(tmp_path, writer, lines)
    snap = O.state_reconstruction(O.get_log_segment(lp), 0)
    malformed = sum(1 for a in O.read_json_actions(b"\n".join(lines)) if a is None)
    st = _gpu_replay(engine, lp, 0)
    try:
        _assert_same(st, snap)
        broken = sum(1 for x in lines if x.startswith(b'{"add":{"path":"broken'))
        assert st.counts["malformed_lines"] == malformed == broken and (broken == 2) == (case == "mixed")
        for side, recs in ((N.DR_LIVE, snap.all_files), (N.DR_TOMBSTONES, snap.tombstones)):
            want = np.sort(np.array([O.record_hash(r, side) for r in recs], dtype=np.uint64))
            assert np.array_equal(np.sort(st.record_hashes(side)), want), (case, side)
    finally:
        st.release()


@pytest.mark.parametrize("case", ["pure", "mixed", "flushed"])
def test_lines_equal_the_reader_restatement(engine, writer, staged_option, case):
    """Record for record, with the "path":null line among the declined ones."""
    from tests.test_gpu_edge_cases import _device_view
    from tests.test_json_lane import expected
    lines = _mixed(writer, True) if case == "mixed" else CASES[case](writer)
    body = b"\n".join(HEAD + writer[0][:FILL] + lines) + b"\n"
    staged = engine.stage_files([(0, 0, 0, body)])
    try:
        got = staged.parse_lines()
    finally:
        staged.release()
    want = HEAD + writer[0][:FILL] + lines
    assert len(got) == len(want)
    for line, rec in zip(want, got):
        assert rec["line"] == line
        assert _device_view(rec) == expected(line), line
