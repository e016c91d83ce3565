"""The checkpoint writer's corpus checks itself (tests/ckpt_writer_corpus.py): every body kind holds the forms
it is named for -- in the steered compressor's output at 8 KiB fragments and 64-byte copies where the form does
not depend on the 64-byte slices, in the restated algorithm's output (model_elements) where it does --, the
colliding groups collide under the constants read from k_encode.hip, and expected_rows agrees with pyarrow's
reading of a checkpoint that pyarrow wrote from the same actions. A builder that drifts fails here instead of
testing nothing on the GPU."""
import os

import pytest

from oracle import delta_oracle as O
from tests import ckpt_writer_corpus as W
from tests import snappy_corpus as S

F = W.FRAG


def _page(kind, size, seed=1):
    return W.steered(kind, size, seed)[1]


def _lits(el):
    return [e for e in el if e[0] == "lit"]


def _copies(el):
    return [e for e in el if e[0] == "copy"]


def keeps_8k(el):
    """The writer's rule: no element straddles an 8 KiB fragment end, no copy reaches before its fragment."""
    return all(op // F == (op + n - 1) // F and (e[0] == "lit" or e[1] <= op % F) for op, n, e in S.spans(el))


@pytest.mark.parametrize("kind", sorted(W.KINDS))
def test_the_model_is_a_compressor(kind):
    for size in (8192, 16384) if kind in ("copy_lengths", "collide") else (197, 253, 8193, 16384, 65537):
        page = _page(kind, size)
        assert len(page) == size
        el = W.model_elements(page)
        body = S.encode(el)
        assert S.reference(body, size) == page and S.pyarrow_decode(body, size) == page and keeps_8k(el)
        assert S.keeps_fragments(el)
        for f0 in range(0, size, F):
            assert sum(len(S.encode_element(e)) for op, _, e in S.spans(el) if op // F == f0 // F) <= W.SLOT


def test_smallest_page_and_prefix():
    assert W.ONE_ADD_SKIP == 11
    assert W.one_add_page(None) == bytes([3, 0, 0, 0, 3, 0x10, 0])
    assert W.one_add_page(b"ab") == bytes([3, 0, 0, 0, 3, 0x20, 0, 2, 0, 0, 0]) + b"ab"
    assert all(size % 64 in (0, 1, 3, 4, 5, 60, 61) for size in W.TAILS)


def test_literal_lengths():
    ref = {L: S.compress(_page("slice_literals(%d)" % L, 8192), fragment=F, max_copy=64) for L in (59, 60)}
    # (a slice's last fresh byte recurs among the 127 slices before it, and then the match begins one byte early:
    # about half of the slices show the exact length)
    assert sum(len(e[1]) == 59 and e[2] == 0 for e in _lits(ref[59])) >= 30
    assert sum(len(e[1]) == 60 and e[2] == 0 for e in _lits(ref[60])) >= 30
    assert {e[2] for e in _copies(ref[59])} >= {5} and {e[2] for e in _copies(ref[60])} >= {4}
    mod = {L: W.model_elements(_page("slice_literals(%d)" % L, 8192)) for L in (1, 59, 60, 61, 63)}
    for L in (1, 59, 60):
        assert sum(len(e[1]) == L and e[2] == 0 for e in _lits(mod[L])) >= 30, L
        assert sum(e[2] == 64 - L for e in _copies(mod[L])) >= 30, L
    for L in (61, 63):       # no room for a copy behind the fresh bytes: literals of the whole slice, 60 << 2 and a length byte
        assert sum(len(e[1]) == 64 and e[2] == 1 for e in _lits(mod[L])) >= 30
    # the tag boundary itself: tails of 60 and 61 bytes
    assert W.model_elements(_page("random", 252))[-1] == ("lit", _page("random", 252)[-60:], 0)
    assert W.model_elements(_page("random", 253))[-1] == ("lit", _page("random", 253)[-61:], 1)
    # tails of 1 to 3 bytes are literals of their own
    for size, tail in ((193, 1), (195, 3)):
        assert len(W.model_elements(_page("random", size))[-1][1]) == tail


def test_copy_tags_at_each_boundary():
    page = _page("copy_lengths", 16384)
    ref = _copies(S.compress(page, fragment=F, max_copy=64))
    assert {(e[2], e[3]) for e in ref if e[1] < 2048} >= {(4, 1), (11, 1), (12, 2)}
    assert {(e[2], e[3]) for e in ref if e[1] >= 2048} >= {(4, 2)}
    mod = _copies(W.model_elements(page))
    planned = {(t - s, n) for s, t, n in W.COPY_PLAN}
    for f in range(2):
        got = {(e[1], e[2]): e[3] for op, _, e in S.spans(W.model_elements(page)) if e[0] == "copy" and op // F == f}
        assert set(got) >= planned, planned - set(got)
        for (off, n), tag in got.items():
            assert tag == (1 if n <= 11 and off < 2048 else 2)
    assert {(off, n) for off, n in planned if off in (2047, 2048)} == {(o, n) for o in (2047, 2048) for n in (4, 11, 12)}
    assert max(off for off, _ in planned) > 8000 and len(mod) >= 2 * len(planned)


def test_overlapping_copies():
    page = _page("runs", 8192)
    for el in (S.compress(page, fragment=F, max_copy=64), W.model_elements(page)):
        for off in (1, 2, 3):
            assert any(e[1] == off and e[2] > off for e in _copies(el)), off
    # inside the run of one byte a slice is at most a literal and a copy
    el = W.model_elements(page)
    per = {}
    for op, n, e in S.spans(el):
        per[op // 64] = per.get(op // 64, 0) + 1
    inside = [s for s in range(1, W.RUN // 64)]
    assert inside and max(per[s] for s in inside) <= 2


def test_periodic_and_random_bounds_hold_for_the_model():
    for size in (8192, 16384, 65536, 2 * 65536 + 100):
        el = W.model_elements(_page("periodic64", size))
        for f in range(size // F):
            mine = [e for op, _, e in S.spans(el) if op // F == f]
            assert len(mine) <= 128 and sum(len(S.encode_element(e)) for e in mine) <= 66 + 127 * 3, (size, f, len(mine))
        el = W.model_elements(_page("random", size))
        n_in = sum(len(S.encode_element(e)) for e in el)
        assert n_in <= size + 2 * -(-size // 64) and sum(e[2] for e in _copies(el)) <= size // 100


def test_utf8_has_high_bytes_in_every_slice():
    page = _page("utf8", 8195)
    assert all(any(b >= 0x80 for b in page[s:s + 64]) for s in range(64, len(page) - 64, 64))
    page[W.ONE_ADD_SKIP:].decode("utf-8")


def test_collide_really_collides():
    groups = W.colliding_groups()
    assert len(set(groups)) == W.COLLIDE_GROUPS
    assert len({W.sc_hash(int.from_bytes(g, "little")) for g in groups}) == 1
    # the constants are the source's
    src = open(os.path.join(W.ROOT, "delta_amd", "csrc", "k_encode.hip")).read()
    assert "0x%xu" % W.MULT in src and "SC_TBITS = %d;" % W.TBITS in src
    page = _page("collide", 16384)
    for f0 in (0, F):
        last, rep = W.collide_repeat(f0)
        assert page[rep:rep + 4] == page[last:last + 4] == groups[-1] and page[rep + 4] != page[last + 4]
        # the most-recent-occurrence compressor finds the repeat, the earliest-position table cannot
        assert any(e == ("copy", 16, 4, 1) and op == rep for op, _, e in S.spans(S.compress(page, fragment=F, max_copy=64)))
        assert covered_by_literals(W.model_elements(page), rep, 4)


def covered_by_literals(el, at, n):
    return all(e[0] == "lit" for op, ln, e in S.spans(el) if op < at + n and op + ln > at)


def test_expected_rows_agree_with_pyarrow(tmp_path):
    import pyarrow.parquet as pq
    from delta_amd.testing import synth
    commits = W.level_table(n_adds=60, n_removes=25, txns=2)
    actions = [a for c in commits for a in c]
    want = W.expected_rows(actions, W.CUTOFF)
    adds = [r["add"] for r in actions if "add" in r]
    live = [a for a in adds if int(a["path"][2:7]) < 60]
    removes = [dict(r["remove"], size=r["remove"].get("size", 0)) for r in actions
               if "remove" in r and O.del_timestamp(O.make_remove(r["remove"])) > W.CUTOFF]
    assert any(a["partitionValues"] is None for a in live) and any(a["partitionValues"] == {} for a in live)
    assert any(a.get("tags") and None in a["tags"].values() for a in live)
    assert any("stats" not in a for a in live) and any(a.get("stats") == "" for a in live)
    path = str(tmp_path / "ck.parquet")
    md = next(a["metaData"] for a in actions if "metaData" in a)
    synth.write_checkpoint_records(path, W.PROTOCOL, md, live, removes, txns=[a["txn"] for a in actions if "txn" in a])
    got = pq.read_table(path).to_pylist()
    assert len(got) == len(want) == 4 + 60 + 25
    W.assert_rows(got, want)
    assert [W.kind_of(r) for r in got] == ["protocol", "metaData", "txn", "txn"] + ["add"] * 60 + ["remove"] * 25
    # the retention rule: a tombstone at the cutoff is gone
    assert len(W.expected_rows(actions + [W.remove("late", deletionTimestamp=-2 ** 63)], W.CUTOFF)) == len(want)
    assert len(W.expected_rows(actions + [W.remove("late", deletionTimestamp=-2 ** 63 + 1)], W.CUTOFF)) == len(want) + 1
