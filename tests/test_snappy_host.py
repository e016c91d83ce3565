"""The host SNAPPY decoder (snappy_host.cpp) against the strict reference of tests/snappy_corpus.py, and that
reference against pyarrow's libsnappy. A stand-alone program (tests/native/snappy_host_main.cpp), built under
AddressSanitizer + UndefinedBehaviorSanitizer, decodes the corpus -- streams pyarrow wrote and crafted ones
holding what that compressor never writes (tag-3 copies, literal lengths in more bytes than they need, copies
shorter than 4, elements that ignore the 64 KiB fragments): its output must equal the reference's, and over
10,000 seeded mutations it must accept exactly what the reference accepts, with the same bytes. The reference
and pyarrow must agree on every one of those mutations too: no class of disagreement is tolerated.

MALFORMED / malformed_bodies() hold one body per refusal; tests/test_gpu_snappy_pages.py sends the same
bodies to the device."""
import os
import shutil
import subprocess

import pytest

from tests import snappy_corpus as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "delta_amd", "csrc")
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def _build(tmp, name, srcs):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "include"), "-I", CSRC] + ASAN + srcs +
                       ["-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("snappy"), "snappy_host_main",
                  [os.path.join(ROOT, "tests", "native", "snappy_host_main.cpp"), os.path.join(CSRC, "snappy_host.cpp")])


def decode_all(exe, tmp_path, items):
    """[bytes or None] of the program over (n_out, stream) items; the sanitizers must stay silent."""
    path = str(tmp_path / "records.bin")
    with open(path, "wb") as f:
        f.write(S.records([(n_out, 0, s) for n_out, s in items]))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(items)
    return [None if ln.startswith("error") else b"" if ln == "-" else bytes.fromhex(ln) for ln in lines]


@pytest.fixture(scope="module")
def corpus():
    return S.corpus()


def test_corpus_equals_the_reference_and_pyarrow(exe, tmp_path, corpus):
    assert len(corpus) >= 50
    got = decode_all(exe, tmp_path, [(len(data), s) for _, s, data in corpus])
    for (name, s, data), out in zip(corpus, got):
        assert S.reference(s, len(data)) == data, name
        assert S.pyarrow_decode(s, len(data)) == data, name
        assert S.encode(S.elements_of(s), preamble=S.preamble_of(s)[1]) == s, name   # elements_of inverts encode
        assert out == data, name


def test_what_pyarrow_writes():
    """What the crafted streams are for: the forms this compressor does not write."""
    for name, data in S.payloads().items():
        body = S.pyarrow_body(data)
        el = S.elements_of(body)
        assert S.keeps_fragments(el), name
        assert all(e[3] != 4 and e[2] >= 4 for e in el if e[0] == "copy"), name
        assert all(e[2] == S.min_nb(len(e[1])) for e in el if e[0] == "lit"), name


def test_the_crafted_streams_show_what_they_are_named_for():
    c = {k: (S.elements_of(b), S.layout(b)[0], b, d) for k, (b, d) in S.crafted().items()}
    copies = lambda k: [e for e in c[k][0] if e[0] == "copy"]   # noqa: E731
    lits = lambda k: [e for e in c[k][0] if e[0] == "lit"]      # noqa: E731
    assert len(copies("every copy tag 3")) > 500 and {e[3] for e in copies("every copy tag 3")} == {4}
    assert {e[3] for e in copies("every copy tag 2")} == {2}
    assert any(4 <= e[2] <= 11 and e[1] < 2048 for e in copies("every copy tag 2"))   # where tag 1 would do
    for nb in (1, 2, 3, 4):
        ls = lits("literals in %d length bytes" % nb)
        assert len(ls) > 100 and all(e[2] == max(nb, S.min_nb(len(e[1]))) for e in ls) and any(S.min_nb(len(e[1])) < nb for e in ls)
    assert any(len(e[1]) == 1 and e[2] == 4 for e in lits("literals of one byte in 4 length bytes"))
    for n in (60, 61, 64, 65, 256, 257, 65536):
        assert [len(e[1]) for e in lits("literal of %d" % n) if len(e[1]) == n] == [n]
    for n in (1, 2, 3, 64):
        assert {e[2] for e in copies("copies of %d" % n)} == {n} and len(copies("copies of %d" % n)) > 10
    for off in (1, 2, 3):
        assert any(e[1] == off and e[2] == 64 for e in copies("offset %d length 64" % off))
    assert [e[1] for e in copies("offset 65535")] == [65535]
    assert all(e[1] == op for op, _, e in S.spans(c["offset equal to the position in the fragment"][0]) if e[0] == "copy")
    for k in ("every copy tag 3", "every copy tag 2", "offset 65535", "offset equal to the position in the fragment",
              "copies of 1", "literal of 257"):
        assert S.keeps_fragments(c[k][0]), k
    # the four ways to break the writers' fragment rules
    sp = S.spans(c["copy reaching before its fragment"][0])
    assert any(e[0] == "copy" and e[1] > op % 65536 and op // 65536 == (op + n - 1) // 65536 for op, n, e in sp)
    assert any(e[0] == "copy" and e[1] >= 65536 and e[3] == 4 for _, _, e in sp)
    sp = S.spans(c["copy straddling a fragment end"][0])
    assert [e[0] for op, n, e in sp if op < 65536 < op + n] == ["copy"]
    sp = S.spans(c["literal straddling a fragment end"][0])
    assert [e[0] for op, n, e in sp if op < 65536 < op + n] == ["lit"]
    assert all(e[3] == 4 and e[1] >= 65536 for e in copies("tag 3 offset of 65536 and more"))
    assert len(c["two blocks of 65537 bytes"][3]) == 65537 and not S.keeps_fragments(c["two blocks of 65537 bytes"][0])
    for n in (1, 2, 3, 4, 5):
        assert len(c["page of %d" % n][3]) == n and S.preamble_of(c["page of %d" % n][2])[1] == 1
        assert S.preamble_of(c["page of %d in a 3-byte preamble" % n][2]) == (n, 3)
    assert S.preamble_of(c["5-byte preamble"][2])[1] == 5
    assert len(lits("copies only after one byte")) == 1


def test_the_output_length_is_part_of_the_contract(exe, tmp_path):
    data = S.payloads()["text"][:2500]
    s = S.pyarrow_body(data)
    items = [(len(data), s), (len(data) - 1, s), (len(data) + 1, s), (0, s), (len(data), s + b"\0"), (len(data), s[:-1]),
             (0, b"\0"), (0, b""), (1, b"\0"), (0, b"\x80\0"), (0, b"\x80\x80\x80\x80\0"), (0, b"\x80\x80\x80\x80\x80\0"),
             (0, b"\x80\x80\x80\x80\x10"), (0, b"\0\0")]
    want = [S.reference(m, n) for n, m in items]
    assert want == [data, None, None, None, None, None, b"", None, None, b"", b"", None, None, None]
    assert [S.pyarrow_decode(m, n) for n, m in items] == want
    assert decode_all(exe, tmp_path, items) == want


def test_mutations_are_judged_as_the_reference_and_pyarrow_judge_them(exe, tmp_path, corpus):
    """Ours succeeds exactly when the reference does, and then with the same bytes; the reference succeeds
    exactly when pyarrow does, with the same bytes. No disagreement is tolerated on either side."""
    items = []
    small = [c for c in corpus if 0 < len(c[1]) < 30000]
    per = 10000 // len(small) + 1
    for k, (name, s, data) in enumerate(small):
        for m in S.mutations(s, per, seed=k):
            items.append((len(data), m))
    assert len(items) >= 10000
    want = [S.reference(m, n) for n, m in items]
    lib = [S.pyarrow_decode(m, n) for n, m in items]
    got = decode_all(exe, tmp_path, items)
    accepted = sum(w is not None for w in want)
    print("%d mutations, %d accepted by the reference" % (len(items), accepted))
    assert len(items) // 20 < accepted < len(items) * 19 // 20   # both verdicts occur, neither rarely
    differ = [i for i in range(len(items)) if lib[i] != want[i]]
    assert not differ, "the reference and pyarrow differ on %d of %d, first: mutation %d (reference %s)" % (
        len(differ), len(items), differ[0], "accepts" if want[differ[0]] is not None else "refuses")
    differ = [i for i in range(len(items)) if got[i] != want[i]]
    assert not differ, "%d of %d verdicts differ, first: mutation %d (ours %s, reference %s)" % (
        len(differ), len(items), differ[0], "accepts" if got[differ[0]] is not None else "refuses",
        "accepts" if want[differ[0]] is not None else "refuses")


def malformed_bodies(size=400):
    """{class: body}: the fixed malformed page bodies for a page of `size` bytes, one per refusal. Each is
    refused by the host decoder here, under the sanitizers, before any of them reaches the device. Where the
    refusal is a missing byte, the bytes that are there would decode if the decoder read on past the input."""
    n = size
    assert n >= 400
    data = (b"0123456789abcdefghij" * (n // 20 + 1))[:n]   # period 20: a copy at offset 20 k continues the data
    E, lit = S.encode, S.literal
    far = 260 if n >= 600 else 20                           # an offset whose upper bits sit in the copy-1 tag
    out = {}
    out["truncated copy-1 header"] = E(lit(data[:n - 8]) + [("copy", far, 8, 1)])[:-1]
    out["truncated copy-2 header"] = E(lit(data[:n - 8]) + [("copy", 20, 8, 2)])[:-1]
    out["truncated copy-4 header"] = E(lit(data[:n - 8]) + [("copy", 20, 8, 4)])[:-1]
    out["truncated literal length field"] = E(lit(data[:n - 8]) + [("lit", data[n - 8:], 2)])[:-9]
    out["literal past the input"] = E(lit(data[:n - 30]) + lit(data[n - 30:]))[:-1]
    for kind in (1, 2, 4):
        out["offset 0 in a copy-%d" % kind] = E(lit(data[:n - 8]) + [("copy", 0, 8, kind)])
    out["copy as the first element"] = E([("copy", 1, 4, 1)] + lit(data[4:]))
    out["offset one past the output"] = E(lit(data[:100]) + [("copy", 101, 8, 2)] + lit(data[108:]))
    out["output overrun by a literal"] = E(lit(data[:n - 30]) + lit(data[n - 30:] + b"x"), n_out=n)
    out["output overrun by a copy"] = E(lit(data[:n - 4]) + [("copy", 20, 5, 2)], n_out=n)
    out["stream ends short of n_out"] = E(lit(data[:n - 30]) + [("copy", 20, 29, 2)], n_out=n)
    out["preamble too large"] = E(lit(data), n_out=n + 1)
    out["preamble too small"] = E(lit(data), n_out=n - 1)
    # every byte of the page is there; behind it a literal of 2^32 bytes, which 32-bit arithmetic turns into 0
    out["literal length 0xffffffff"] = E(lit(data[:n - 8]) + [("copy", 20, 8, 2)]) + bytes([63 << 2]) + b"\xff" * 4
    return out


MALFORMED = sorted(malformed_bodies())


@pytest.mark.parametrize("size", [400, 4500, 70000])
def test_malformed_classes_are_refused(exe, tmp_path, size):
    """The host decoder and the reference refuse every class; pyarrow refuses every class but one, named by
    its structure: a literal whose 4-byte length field holds 0xffffffff. libsnappy adds the 1 in 32 bits and
    takes the literal for an empty one; the format's length is 2^32, which no input holds."""
    bodies = malformed_bodies(size)
    assert len(bodies) == 16 and sorted(bodies) == MALFORMED
    got = decode_all(exe, tmp_path, [(size, s) for s in bodies.values()])
    assert got == [None] * len(bodies), [k for k, g in zip(bodies, got) if g is not None]
    for k, s in bodies.items():
        assert S.reference(s, size) is None, k
        wraps = S.preamble_of(s) is not None and S.wrapping_literal(s)
        assert wraps == (k == "literal length 0xffffffff")
        assert S.pyarrow_decode(s, size) is None or wraps, k
    # each class is its own refusal: the bytes that are missing or wrong put back, the body decodes
    data = (b"0123456789abcdefghij" * (size // 20 + 1))[:size]
    for k, tail in (("truncated copy-1 header", bytes([(260 if size >= 600 else 20) & 0xff])), ("truncated copy-2 header", b"\0"),
                    ("truncated copy-4 header", b"\0"), ("truncated literal length field", b"\0" + data[-8:]),
                    ("literal past the input", data[-1:])):
        assert S.reference(bodies[k] + tail, size) == data, k
    assert S.reference(bodies["literal length 0xffffffff"][:-5], size) == data
    assert S.layout(bodies["literal length 0xffffffff"])[1] is False
