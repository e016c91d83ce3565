"""The steered DEFLATE writer and the independent reader of tests/deflate_steer.py, and the host inflater over what
they write: every steered stream inflates under zlib's raw inflate to the intended bytes and reads back through walk()
as the forms it was built for (each form is a predicate over what walk() reads from the bytes); the stand-alone
ASan + UBSan host program of tests/test_inflate_host.py gives the same bytes for the catalogue and for the page bodies
that tests/test_gpu_deflate_blocks.py sends to the device, and refuses the bodies that file expects to be refused;
mutations of the steered streams are judged as zlib judges them."""
import pytest

from tests import deflate_steer as T
from tests import inflate_corpus as I
from tests.test_inflate_host import exe, inflate_all  # noqa: F401  (exe: the fixture that builds the program)


@pytest.fixture(scope="module")
def corpus():
    return {name: (raw, data) for name, raw, data in T.corpus()}


@pytest.fixture(scope="module")
def walked(corpus):
    return {name: T.walk(raw) for name, (raw, _) in corpus.items()}


def _lengths_seen(blocks):
    return {(t[2], t[0]) for t in T.matches(blocks)}


def _every_length(blocks):
    want = {(257 + k, v) for k in range(28) for v in (T.LEN_BASE[k], T.LEN_BASE[k] + (1 << T.LEN_EXTRA[k]) - 1)}
    return want | {(284, 258), (285, 258)} <= _lengths_seen(blocks)


def _every_distance(blocks):
    want = {(k, v) for k in range(30) for v in (T.DIST_BASE[k], T.DIST_BASE[k] + (1 << T.DIST_EXTRA[k]) - 1)}
    return want <= {(t[4], t[1]) for t in T.matches(blocks)} and {(29, 32768), (29, 24577)} <= want


def _runs(blocks):
    """{(symbol, repeat count)} of the code-length symbols sent, and whether a 16 repeats a zero."""
    seen, zero = set(), False
    for b in blocks:
        prev = None
        for s, rep in b.get("cl_syms", ()):
            if rep is not None:
                seen.add((s, rep))
                zero |= s == 16 and prev == 0
            prev = s if s < 16 else prev if s == 16 else 0
    return seen, zero


FORMS = {
    # form: (stream of the corpus, predicate over walk()'s blocks)
    "29 length symbols at both ends, 258 both ways": ("lengths", _every_length),
    "the same under the fixed code": ("lengths fixed", lambda bl: bl[0]["kind"] == "fixed" and _every_length(bl)),
    "30 distance symbols at both ends": ("distances", _every_distance),
    "literal/length codes of 10, 11 and 15 bits in use": ("slow codes", lambda bl: {10, 11, 15} <= {t[3] for t in T.literals(bl)}),
    "distance codes of 8, 9 and 15 bits in use": ("slow codes", lambda bl: {8, 9, 15} <= {t[5] for t in T.matches(bl)}),
    "one one-bit distance code alone": ("lone distance code", lambda bl: bl[0]["hdist"] == 0 and bl[0]["dist_lengths"] == [1]
                                        and len(T.matches(bl)) >= 4 and {284, 285} <= {t[2] for t in T.matches(bl)}),
    "literals only, every distance length 0": ("literals only", lambda bl: bl[0]["dist_lengths"] == [0] and not T.matches(bl)
                                               and len(T.literals(bl)) == 400),
    "HLIT 0 and HDIST 0": ("literals only", lambda bl: bl[0]["hlit"] == 0 and bl[0]["hdist"] == 0),
    "an empty block whose only code is 256 at one bit": ("empty dynamic", lambda bl: bl[0]["tokens"] == [] and bl[0]["eob_bits"] == 1
                                                         and [l for l in bl[0]["lit_lengths"] if l] == [1] and bl[0]["n_out"] == 0),
    "HLIT 29 with 285 in use": ("hlit 29 hdist 29", lambda bl: bl[0]["hlit"] == 29 and 285 in {t[2] for t in T.matches(bl)}),
    "HDIST 29 with 29 in use": ("hlit 29 hdist 29", lambda bl: bl[0]["hdist"] == 29 and 29 in {t[4] for t in T.matches(bl)}),
    "HCLEN 15": ("hclen 15", lambda bl: bl[0]["hclen"] == 15 and bl[0]["cl_lengths"][15] > 0 and 15 in {t[3] for t in T.literals(bl)}),
    "code-length runs at both ends of their ranges": ("code-length runs", lambda bl: {(16, 3), (16, 6), (17, 3), (17, 10), (18, 11),
                                                                                      (18, 138)} <= _runs(bl)[0]),
    "16 repeats a zero": ("code-length runs", lambda bl: _runs(bl)[1]),
    "16 crosses into the distance lengths": ("16 crosses", lambda bl: 16 in T.crossings(bl[0]) and bl[0]["dist_lengths"][0] == 6),
    "18 crosses into the distance lengths": ("18 crosses", lambda bl: 18 in T.crossings(bl[0]) and bl[0]["hlit"] == 29),
    "fixed literals of 8 and 9 bits, lengths of 7 and 8": ("fixed 7 8 9 bits", lambda bl: bl[0]["kind"] == "fixed" and {8, 9} == {
        t[3] for t in T.literals(bl)} and {7, 8} == {t[3] for t in T.matches(bl)} and set(range(280, 286)) <= {t[2] for t in T.matches(bl)}),
    "stored blocks of 0 bytes, final and not": ("stored empty", lambda bl: {(b["final"], b["length"]) for b in bl if b["kind"] == "stored"}
                                                == {(0, 0), (1, 0)}),
    "a stored block of 65,535 bytes": ("stored 65535", lambda bl: bl[0]["kind"] == "stored" and bl[0]["length"] == 65535),
}
for _k in range(8):
    FORMS["a stored header at bit %d" % _k] = ("stored at bit %d" % _k, lambda bl, k=_k: bl[-1]["kind"] == "stored" and bl[-1]["bit"] % 8 == k)


def test_every_stream_has_a_form(corpus):
    assert {name for name, _ in FORMS.values()} == set(corpus)


def test_zlib_and_the_walker_agree_on_every_steered_stream(corpus, walked):
    for name, (raw, data) in corpus.items():
        assert I.reference(I.member(data, raw=raw), len(data)) == data, name
        blocks, bit, out = walked[name]
        assert bytes(out) == data and (bit + 7) // 8 == len(raw), name
    for level in (1, 9):   # a second writer: the walker reads zlib's own streams
        for name, data in I.payloads(small=True).items():
            raw = I.raw_deflate(data, level=level)
            assert bytes(T.walk(raw)[2]) == data, name


@pytest.mark.parametrize("form", sorted(FORMS))
def test_form(walked, form):
    name, shows = FORMS[form]
    assert shows(walked[name][0]), form


def test_the_writer_refuses_a_code_that_is_not_complete():
    lits = list(b"abc")
    with pytest.raises(AssertionError, match="incomplete"):
        T.write([("dynamic", lits, [0] * 97 + [2, 2, 2] + [0] * 156 + [3], [0], {}, True)])
    with pytest.raises(AssertionError, match="over-subscribed"):
        T.write([("dynamic", lits, [0] * 97 + [1, 1, 2] + [0] * 156 + [2], [0], {}, True)])
    for forced in ({97: 10, 98: 11, 99: 15}, {}):
        lens = T.steered_lengths(T.frequencies(lits)[0], 286, forced)
        assert T.kraft(lens) == T.FULL and all(lens[s] == l for s, l in forced.items())
    assert max(T.limited_lengths([1 << k for k in range(30)], 7)) == 7


def test_a_match_reaches_exactly_its_members_first_byte():
    body, data = T.two_members()
    assert I.reference(body, len(data)) == data
    members, out = T.walk_body(body)
    assert out == data and len(members) == 2
    (m,) = T.matches(members[1][1])
    assert m[7] - m[1] == members[1][2] > 0    # the source starts where the member's output starts
    with pytest.raises(T.Malformed, match="beyond the start"):
        T.walk_body(T.two_members(1)[0])


def test_the_host_program_inflates_the_catalogue(exe, tmp_path, corpus):  # noqa: F811
    items = [(len(data), I.member(data, raw=raw)) for raw, data in corpus.values()] + [(len(T.two_members()[1]), T.two_members()[0])]
    got = inflate_all(exe, tmp_path, items)
    want = [data for _, data in corpus.values()] + [T.two_members()[1]]
    assert [g == w for g, w in zip(got, want)] == [True] * len(items), [n for n, g, w in zip(list(corpus) + ["two"], got, want) if g != w]


def _refusals_on(exe, tmp_path, data):  # noqa: F811
    """Each refused body is refused by zlib and by the host program; its repaired twin -- the same blocks with the one
    fault taken out -- is accepted by both with the page's bytes: the fault is the only reason."""
    bodies, twins = T.refused_bodies(data), T.refused_bodies(data, repaired=True)
    assert list(bodies) == T.REFUSALS == list(twins) and len(bodies) == 8
    n = len(data)
    assert [I.reference(s, n) for s in bodies.values()] == [None] * 8
    assert [I.reference(s, n) == data for s in twins.values()] == [True] * 8
    got = inflate_all(exe, tmp_path, [(n, s) for s in bodies.values()] + [(n, s) for s in twins.values()])
    assert got == [None] * 8 + [data] * 8, [k for k, g in zip(T.REFUSALS * 2, got[:8] + [None if g == data else g for g in got[8:]]) if g]
    for kind in T.REFUSALS:
        with pytest.raises(T.Malformed):
            T.walk_body(bodies[kind])
        assert T.walk_body(twins[kind])[1] == data, kind
    return bodies


def test_refusals(exe, tmp_path):  # noqa: F811
    from tests import delta_pages_corpus as C
    data = "\n".join(C.config3_paths(200, 3)).encode()
    _refusals_on(exe, tmp_path, data)
    twice, out = T.two_members(1)
    assert I.reference(twice, len(out)) is None and inflate_all(exe, tmp_path, [(len(out), twice)]) == [None]


def test_mutations_of_the_steered_streams_are_judged_as_zlib_judges_them(exe, tmp_path, corpus):  # noqa: F811
    """The rule of test_inflate_host.test_mutations_are_judged_as_zlib_judges_them, over streams whose dynamic headers
    zlib's deflate does not write."""
    items, want = [], []
    for k, name in enumerate(["slow codes", "16 crosses", "18 crosses", "code-length runs", "lone distance code", "hclen 15",
                              "empty dynamic", "lengths"]):
        raw, data = corpus[name]
        for m in I.mutations(I.member(data, raw=raw), 200, seed=700 + k):
            items.append((len(data), m))
            want.append(I.reference(m, len(data)))
    got = inflate_all(exe, tmp_path, items)
    assert 0 < sum(w is not None for w in want) < len(items)
    bad = [i for i in range(len(items)) if got[i] != want[i]]
    assert not bad, "%d of %d verdicts differ, first: mutation %d (ours %s)" % (
        len(bad), len(items), bad[0], "accepts" if got[bad[0]] is not None else "refuses")


def test_the_page_bodies_of_the_gpu_suite(exe, tmp_path):  # noqa: F811
    """The bodies tests/test_gpu_deflate_blocks.py sends to the device, built here without one: each shows its forms on
    the committed table and seed, inflates under zlib (asserted where it is built) and under the host program to the
    page's bytes; the bodies that file expects to be refused are refused."""
    import zlib
    from tests import test_gpu_deflate_blocks as G
    base = G.build_base(str(tmp_path / "base"), G.rows_of)
    _, ck = G.gzip_variant(base, tmp_path / "good")
    P = G.page_of(ck)
    shown = [a.get("stats") or "" for a in base[4].all_files]   # the steered rows are rows the live state shows
    assert all(sum(v in s for s in shown) == k for v, k in ((G.STRETCH, 1), ("Z" * G.ZRUN, 1), (G.MARKER, 2), (G.PERIODS_ROW, 1),
                                                            (G.UTF8, 1)))
    walked = {name: G.walked_body(P, name) for name in G.BODIES}
    for form, (name, shows) in G.FORMS.items():
        assert shows(walked[name], P), form
    got = inflate_all(exe, tmp_path, [(len(P.D), w.body) for w in walked.values()])
    assert [g == P.D for g in got] == [True] * len(walked), [n for n, g in zip(walked, got) if g != P.D]
    # the 4 KiB variant: sixteen input phases, tiny members
    _, ck4 = G.gzip_variant(base, tmp_path / "k4", page_size=4096)
    pages = G.phased_file(ck4, ck4)
    assert len(pages) > 100 and {at % 16 for at, c, u in pages if c} == set(range(16))
    buf = open(ck4, "rb").read()
    items = [(u, buf[at:at + c]) for at, c, u in pages]
    want = [I.reference(s, n) for n, s in items]
    assert None not in want and inflate_all(exe, tmp_path, items) == want
    assert set(G.TINY) <= {m[3] for _, s in items[:8] for m in T.walk_body(s)[0]}
    # the refusals, on the page they are sent in
    at, c, u = I.gzip_pages(ck, "add.path")[0]
    _refusals_on(exe, tmp_path, zlib.decompress(open(ck, "rb").read()[at:at + c], 31))
