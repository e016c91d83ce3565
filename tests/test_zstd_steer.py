"""The steered ZSTD encoder and the strict block reader of tests/zstd_steer.py, and the host decoder over what
they write: every steered body decodes under pyarrow's libzstd to the intended bytes and reads back as exactly
the sequences that went in; the reader decodes libzstd's own frames; the stand-alone ASan + UBSan host program
of tests/test_zstd_host.py gives the same bytes for the small steered corpus and for the page bodies that
tests/test_gpu_zstd_blocks.py sends to the device, and refuses the bodies that file expects to be refused;
mutations of the steered corpus are judged as the reference judges them."""
import re

import pytest

from tests import zstd_corpus as Z
from tests import zstd_steer as T
from tests.test_zstd_host import decode_all, exe  # noqa: F401  (exe: the fixture that builds the program)


@pytest.fixture(scope="module")
def corpus():
    return T.corpus()


def test_the_reader_decodes_what_libzstd_writes():
    """A second writer: levels 1, 3 and 19 of every payload; the forms agree with the walker's."""
    for name, data in Z.payloads().items():
        for level in (1, 3, 19):
            s = Z.one_shot(data, level)
            p = T.sequences(s)
            assert p.data == data, (name, level)
            assert T.forms(p) & Z.FEATURES == Z.walk(s)[1], (name, level)
    for name, s, data in Z.streams(small=True):
        assert T.sequences(s).data == data and T.forms(T.sequences(s)) & Z.FEATURES == Z.walk(s)[1], name


def test_steered_bodies_decode_and_read_back(corpus):
    assert len(corpus) >= 9
    for name, s, data in corpus:
        assert Z.reference(s, len(data)) == data, name   # a body libzstd refuses is a failure of the corpus
        assert T.sequences(s).data == data, name


def test_sequences_returns_what_went_in():
    data = Z.text(4000, 3)
    blocks = T.parse(data, offsets=(1, 2), max_ml=40, cut_every=50)
    seqs = [q for _, s in blocks for q in s]
    assert len(blocks) > 2 and any(o < 0 for _, _, o in seqs) and any(o > 0 for _, _, o in seqs)
    o = dict(ll=T.fitted(seqs, 0, 7), of=T.fitted(seqs, 1, 6), ml=T.fitted(seqs, 2, 8), lit="compressed", streams=4)
    s, content = T.encode_frame(T.steer(blocks[:1], **o) + T.steer(blocks[1:], ll=T.REPEAT, of=T.REPEAT, ml=T.REPEAT, lit="treeless"))
    p = T.sequences(s)
    assert content == data == p.data == Z.reference(s, len(data))
    rep = [1, 4, 8]
    for (lits, want), b in zip(blocks, p.frames[0]["blocks"]):
        assert b["literals"]["regen"] == len(lits) and len(b["seqs"]) == len(want)
        for (ll, ml, off), got in zip(want, b["seqs"]):
            d, rep = T.resolve(rep, off + 3 if off > 0 else -off, ll)
            assert got == (ll, ml, d, T.offset_code(off + 3 if off > 0 else -off)[0], T.code_of(ll, T.LL_BASE)[0], T.code_of(ml, T.ML_BASE)[0])
    assert p.frames[0]["blocks"][0]["modes"] == (T.FSE,) * 3 and p.frames[0]["blocks"][0]["logs"] == (7, 6, 8)
    assert p.frames[0]["blocks"][1]["modes"] == (T.REPEAT,) * 3 and p.frames[0]["blocks"][1]["literals"]["type"] == "treeless"


def test_table_descriptions_hold_less_than_one_and_zero_runs():
    """The count writer against the count reader, on distributions with -1 entries and with zero runs that need
    the repeat flag 3 (three or more zeros behind a zero), no flag at all, and a run at the very front."""
    cases = [([0, 0, 0, 0, 0, 30, 1, -1], 5), ([1, 0, 0, 0, 0, 0, 0, 0, -1, 30], 5), ([-1] * 8 + [0] * 9 + [504], 9),
             ([0, 1, 0, 2, 0, 0, 29], 5), (T.DEFAULT[0][0], 6), (T.DEFAULT[1][0], 5), (T.DEFAULT[2][0], 6),
             (T.distribution({2, 30, 52}, 9, less_than_one=(52,)), 9)]
    for norm, log in cases:
        d = T.write_distribution(norm, log)
        assert T.read_distribution(d + b"\0\0", 0, len(d), 255) == (list(norm), log, len(d)), norm
    d = T.write_distribution(cases[1][0], 5)
    bits = int.from_bytes(d, "little") >> 4
    # 1 + 1 in five bits, 0 + 1 in five bits, then six more zeros: the flags 3, 3 and 0
    assert bits & 31 == 2 and bits >> 5 & 31 == 1 and bits >> 10 & 3 == 3 and bits >> 12 & 3 == 3 and bits >> 14 & 3 == 0


def test_the_host_program_decodes_the_steered_corpus(exe, tmp_path, corpus):  # noqa: F811
    got = decode_all(exe, tmp_path, [(len(data), s) for _, s, data in corpus])
    for (name, s, data), out in zip(corpus, got):
        assert out == data, name


def test_refused_bodies_are_refused_on_the_host(exe, tmp_path):  # noqa: F811
    bodies = T.refused_bodies()
    assert sorted(bodies) == sorted(T.REFUSALS)
    for n_out in (572250, 704, 0):
        assert [Z.reference(s, n_out) for s in bodies.values()] == [None] * len(bodies)
        assert decode_all(exe, tmp_path, [(n_out, s) for s in bodies.values()]) == [None] * len(bodies)
    for kind, s in bodies.items():   # refused in the second frame for the one reason it is named for: the first is good
        with pytest.raises(T.Malformed, match="^%s$" % re.escape(T.REASONS[kind])):
            T.sequences(s)
        first = T.sequences(s[:Z.walk(s[:s.index(Z.MAGIC.to_bytes(4, "little"), 4)])[0][0]["end"]])
        assert len(first.data) == 320


def test_the_refused_treeless_and_repeat_blocks_are_good_inside_one_frame():
    """The same two blocks behind the first frame's block, in that frame: libzstd decodes them. So in a frame of their
    own nothing refuses them but the tree and the tables that a frame's start takes away."""
    text = Z.text(600, 4)
    head = ("seq", text[:200], [(150, 20, 100)], dict(lit="compressed", streams=1, weights=T.huffman_weights(text),
                                                     ll=T.fitted([(150, 3, 1)], 0, 6, pad=(0, 18))))
    s, content = T.encode_frame([head, ("seq", text[340:400], [(20, 4, 10)], dict(ll=T.REPEAT, of=T.REPEAT, ml=T.REPEAT)),
                                 ("seq", text[340:400], [], dict(lit="treeless"))])
    assert Z.reference(s, len(content)) == content == T.sequences(s).data


def test_the_host_program_decodes_the_page_bodies_of_the_gpu_suite(exe, tmp_path):  # noqa: F811
    """The bodies tests/test_gpu_zstd_blocks.py sends to the device, built here without one: each shows its forms,
    decodes under libzstd (asserted where it is built) and under the host program to the page's bytes."""
    from tests import test_gpu_zstd_blocks as G
    base = G.build_base(str(tmp_path / "base"))
    _, ck = G.zstd_variant(base, tmp_path / "good")
    P = G.page_of(ck)
    bodies = {name: G.parsed_body(P, name) for name in G.BODIES}
    for form, (name, shows) in G.FORMS.items():
        assert shows(bodies[name][1]), form
    got = decode_all(exe, tmp_path, [(len(P.D), body) for body, _ in bodies.values()])
    assert [g == P.D for g in got] == [True] * len(bodies), [n for n, g in zip(bodies, got) if g != P.D]


def test_mutations_of_the_steered_corpus_are_judged_as_the_reference_judges_them(exe, tmp_path, corpus):  # noqa: F811
    """100 seeded mutations per steered body, half of them at the header offsets, under the rule of
    tests/test_zstd_host.py: ours succeeds exactly when the reference does, with the same bytes; a stream we accept
    and the reference refuses is tolerated only in the classes that file names, and in at most 2 % of the cases."""
    items = [(len(data), m) for k, (_, s, data) in enumerate(corpus) for m in Z.mutations(s, 100, seed=900 + k)]
    want = [Z.reference(m, n) for n, m in items]
    got = decode_all(exe, tmp_path, items)
    assert 0 < sum(w is not None for w in want) < len(items)
    loose = Z.reference_is_loose()
    differ = [i for i in range(len(items)) if got[i] != want[i]]
    tolerated = [i for i in differ if want[i] is None and got[i] is not None and
                 (Z.two_symbol_eligible(items[i][1]) or (not loose and Z.loose_eligible(items[i][1])))]
    bad = [i for i in differ if i not in tolerated]
    assert not bad, "%d of %d verdicts differ, first: mutation %d of %s (ours %s)" % (
        len(bad), len(items), bad[0] % 100, corpus[bad[0] // 100][0], "accepts" if got[bad[0]] is not None else "refuses")
    assert len(tolerated) <= len(items) // 50
