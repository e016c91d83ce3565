"""The host LZ4 decoder (lz4_host.cpp) through the rules of lz4_fmt.h that the device kernel (k_lz4.hip)
walks too. A stand-alone program (tests/native/lz4_host_main.cpp), built under AddressSanitizer +
UndefinedBehaviorSanitizer, decodes the corpus of tests/lz4_corpus.py -- bare blocks (Parquet codec 7) and
Hadoop-framed bodies (codec 5): its output must equal the reference's (the liblz4 inside pyarrow, one call
per block), and over 10,000 seeded mutations it must accept exactly what the reference accepts, with the
same bytes. One class is tolerated under a structural predicate capped at 1 %: a sequence with offset 0,
which liblz4 does not look at and lz4_fmt.h refuses."""
import os
import shutil
import subprocess

import pytest

from tests import lz4_corpus as L

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
    return _build(tmp_path_factory.mktemp("lz4"), "lz4_host_main",
                  [os.path.join(ROOT, "tests", "native", "lz4_host_main.cpp"), os.path.join(CSRC, "lz4_host.cpp")])


@pytest.fixture(scope="module")
def column_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("dph"), "delta_pages_host",
                  [os.path.join(ROOT, "tests", "native", "delta_pages_host.cpp"), os.path.join(CSRC, "parquet_meta.cpp"),
                   os.path.join(CSRC, "snappy_host.cpp")])


def decode_all(exe, tmp_path, items):
    """[bytes or None] of the program over (n_out, framing, stream) items; the sanitizers must stay silent."""
    path = str(tmp_path / "records.bin")
    with open(path, "wb") as f:
        f.write(L.records(items))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(items)
    return [None if ln.startswith("error") else b"" if ln == "-" else bytes.fromhex(ln) for ln in lines]


def error_codes(exe, tmp_path, items):
    """[lz4::Err code or None for an accepted item]"""
    path = str(tmp_path / "records_codes.bin")
    with open(path, "wb") as f:
        f.write(L.records(items))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return [int(ln.split()[1]) if ln.startswith("error") else None for ln in r.stdout.splitlines()]


@pytest.fixture(scope="module")
def corpus():
    return L.corpus()


def test_corpus_equals_the_reference(exe, tmp_path, corpus):
    assert len(corpus) >= 60
    got = decode_all(exe, tmp_path, [(len(data), framing, s) for _, s, framing, data in corpus])
    for (name, s, framing, data), out in zip(corpus, got):
        assert L.reference(s, len(data), framing) == data, name
        assert out == data, name


def test_the_crafted_blocks_show_what_they_are_named_for():
    c = L.crafted()
    for off in (1, 2, 3, 65535):
        assert any(s[2] == off for s in L.walk(c["offset %d" % off][0])["seqs"])
    for name, (block, data) in c.items():
        w = L.walk(block)
        if name.startswith("literal length"):
            v, ext = int(name.split()[2]), int(name.split("(")[1].split()[0])
            assert w["seqs"][0][1] == v and w["seqs"][0][0] == 1 + ext, name
            assert ext != 3 or v != 15 + 510 or block[3] == 0     # a final extension byte of exactly 0
        if name.startswith("match length"):
            v, ext = int(name.split()[2]), int(name.split("(")[1].split()[0])
            assert w["seqs"][0][3] == v and w["seqs"][1][0] == 2 + 40 + 2 + ext + 1, name
    block, data = c["match ends at the last permitted position"]
    lit, ll, off, ml = L.walk(block)["seqs"][0]
    assert ll + ml == len(data) - 5 and ll <= len(data) - 12
    # one byte further and the reference refuses: the last five bytes are literals
    over = L.encode([(data[:ll], off, ml + 1), (data[-5:][1:], 0, 0)])
    assert L.walk(over)["size"] == len(data) and L.reference(over, len(data), L.BARE) is None


def test_the_output_length_is_part_of_the_contract(exe, tmp_path):
    data = L.payloads()["text"][:2500]
    s = L.pyarrow_block(data)
    h = L.hadoop([[s]])
    items = [(len(data), 0, s), (len(data) - 1, 0, s), (len(data) + 1, 0, s), (0, 0, s), (len(data), 0, s + b"\0"),
             (len(data), 0, s[:-1]), (0, 0, b""), (1, 0, b""), (0, 0, b"\0"), (0, 0, b"\0\0"),
             (len(data), 1, h), (len(data) - 1, 1, h), (len(data) + 1, 1, h), (len(data), 1, h + b"\0"), (len(data), 1, h[:-1]),
             (len(data), 1, s), (0, 1, b""), (1, 1, b"")]
    got = decode_all(exe, tmp_path, items)
    assert got == [data] + [None] * 7 + [b"", None] + [data] + [None] * 5 + [b"", None]
    assert [L.reference(m, n, f) for n, f, m in items] == got


def test_mutations_are_judged_as_the_reference_judges_them(exe, tmp_path, corpus):
    """Ours succeeds exactly when the reference does, and then with the same bytes. A must-accept failure
    is never tolerated. A stream the reference accepts and we refuse is tolerated only under
    L.zero_offset, and at most 1 % of the mutations may fall under it."""
    items = []
    small = [c for c in corpus if 0 < len(c[1]) < 30000]
    per = 10000 // len(small) + 1
    for k, (name, s, framing, data) in enumerate(small):
        for m in L.mutations(s, per, seed=k, framing=framing):
            items.append((len(data), framing, m))
    assert len(items) >= 10000
    want = [L.reference(m, n, f) for n, f, m in items]
    got = decode_all(exe, tmp_path, items)
    accepted = sum(w is not None for w in want)
    assert len(items) // 20 < accepted < len(items) * 19 // 20   # both verdicts occur, neither rarely
    differ = [i for i in range(len(items)) if got[i] != want[i]]
    tolerated = [i for i in differ if got[i] is None and L.zero_offset(items[i][2], items[i][1])]
    bad = [i for i in differ if i not in tolerated]
    print("%d mutations, %d accepted by the reference, %d verdicts differ, %d of them tolerated (offset 0)"
          % (len(items), accepted, len(differ), len(tolerated)))
    assert not bad, "%d of %d verdicts differ, first: mutation %d of framing %d (ours %s, reference %s)" % (
        len(bad), len(items), bad[0], items[bad[0]][1], "accepts" if got[bad[0]] is not None else "refuses",
        "accepts" if want[bad[0]] is not None else "refuses")
    assert len(tolerated) <= len(items) // 100, (len(tolerated), len(items))


def malformed_bodies(framing, size=400):
    """{class: body}: the fixed malformed page bodies for a page of `size` bytes, one per refusal of
    lz4_fmt.h. Each is refused by the host decoder here, under the sanitizers, before any of them reaches
    the device."""
    E = L.encode
    n = size
    assert n > 340   # below that the two length-extension classes have no room and turn into other refusals
    pre, tail = (b"0123456789abcdefghij" * (n // 20 + 1))[:n - 32], b"TAIL-OF-12-B"
    good = [(pre, 5, 20), (tail, 0, 0)]
    assert len(L.decode_seqs(good)) == n
    cut = len(E([(pre, 0, 0)]))          # token, length bytes and literals of the first sequence
    out = {}
    out["offset 0"] = E([(pre, 0, 20), (tail, 0, 0)])
    out["offset beyond the block's output"] = E([(pre, len(pre) + 1, 20), (tail, 0, 0)])
    out["literal run off the input"] = E(good)[:-3]
    head = len(E([(pre[:-300], 0, 0)]))   # token, length bytes and literals of a first sequence 300 bytes shorter
    # ... offset, one match length byte, the last token (literal nibble 15) and 20 of its 30 length bytes 0xff:
    # the run of length bytes starts in front of liblz4's limit for it (15 bytes before the end) and crosses it
    out["literal length extension off the input"] = E([(pre[:-300], 5, 20), (b"x" * (15 + 255 * 30), 0, 0)])[:head + 2 + 1 + 1 + 20]
    # ... offset and 10 of the match length's 30 length bytes 0xff (limit: 4 bytes before the end)
    out["match length extension off the input"] = E([(pre[:-300], 5, 4 + 15 + 255 * 30), (tail, 0, 0)])[:head + 2 + 10]
    out["truncated offset"] = E(good)[:cut + 1]
    out["write past n_out"] = E([(pre, 5, 21), (tail, 0, 0)])
    out["input left over after the final literals"] = E(good) + b"\0"
    out["output short of n_out"] = E([(pre, 5, 19), (tail, 0, 0)])
    out["last five bytes are not literals"] = E([(pre, 5, 28), (tail[:4], 0, 0)])
    out["match starts in the last twelve bytes"] = E([(pre + b"x" * 21, 5, 4), (tail[:7], 0, 0)])
    if framing == L.BARE:
        return out
    H = L.hadoop
    blk = E(good)
    short = E([(pre[:-20], 5, 20), (tail, 0, 0)])
    out = {k: H([(n, [b])]) for k, b in out.items()}
    out["C larger than the remaining input"] = H([(n, [blk])])[:-1]
    out["fewer than 8 bytes where a unit starts"] = H([(n, [blk])]) + b"\0\0\0\1\0\0\0"
    out["inner block produces more than is left of U"] = H([(n - 1, [blk])])
    out["U = 0"] = H([(n, [blk])]) + b"\0" * 8
    out["U larger than the page"] = H([(n + 5, [blk])])
    out["units do not add up to n_out"] = H([(n - 20, [short])])
    out["the input ends before the unit has its U bytes"] = H([(n, [short])])
    k = n - 52 - 32
    out["an offset reaches below its inner block"] = H([(n, [E([(pre[:20], 5, 20), (tail, 0, 0)]),
                                                             E([(pre[:k], k + 5, 20), (tail, 0, 0)])])])
    return out


MALFORMED = {f: sorted(malformed_bodies(f)) for f in (L.BARE, L.HADOOP)}


@pytest.mark.parametrize("size", [400, 4500])
@pytest.mark.parametrize("framing", [L.BARE, L.HADOOP])
def test_malformed_classes_are_refused(exe, tmp_path, framing, size):
    bodies = malformed_bodies(framing, size)
    assert len(bodies) == (11 if framing == L.BARE else 19)
    got = decode_all(exe, tmp_path, [(size, framing, s) for s in bodies.values()])
    assert got == [None] * len(bodies), [k for k, g in zip(bodies, got) if g is not None]
    for k, s in bodies.items():
        assert L.reference(s, size, framing) is None or k == "offset 0", k
    # the length-extension classes are refused for what they are named for (lz4::E_INPUT), and end in 0xff
    codes = error_codes(exe, tmp_path, [(size, framing, s) for s in bodies.values()])
    for k, s, code in zip(bodies, bodies.values(), codes):
        if "length extension" in k:
            assert code == 1 and s[-1] == 0xff, (k, code)
    assert codes[list(bodies).index("offset 0")] == 2
    # each class is its own refusal: the good body it was made from decodes
    pre = (b"0123456789abcdefghij" * (size // 20 + 1))[:size - 32]
    good = L.encode([(pre, 5, 20), (b"TAIL-OF-12-B", 0, 0)])
    assert decode_all(exe, tmp_path, [(size, L.BARE, good), (size, L.HADOOP, L.hadoop([[good]]))]) == \
        [L.decode_seqs([(pre, 5, 20), (b"TAIL-OF-12-B", 0, 0)])] * 2


def _table(n):
    import pyarrow as pa
    from tests import delta_pages_corpus as C
    paths = C.config3_paths(n, 3)
    return {"path": pa.array([None if i % 7 == 0 else p for i, p in enumerate(paths)], pa.string()),
            "size": pa.array([(i * 7919) % 100003 for i in range(n)], pa.int64()),
            "few": pa.array(["v%d" % (i % 5) for i in range(n)], pa.string())}


@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("dictionary", [False, True])
def test_rewritten_codec_5_files_read_back_in_pyarrow(tmp_path, version, dictionary):
    """The helper before anything else: pyarrow reads every rewritten codec-5 file back to the original
    table when each unit holds one inner block, and several units of one inner block each."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    t = pa.table(_table(3000))
    src, one, many = (str(tmp_path / n) for n in ("raw.parquet", "one.parquet", "many.parquet"))
    pq.write_table(t, src, compression="lz4", use_dictionary=dictionary, data_page_version=version, data_page_size=4096,
                   write_statistics=False, row_group_size=1700)
    assert set(L.codecs_of(src).values()) == {7}
    L.to_hadoop(src, one)
    L.to_hadoop(src, many, split=lambda leaf, k, data: [[data[:len(data) // 3]], [data[len(data) // 3:]]] if len(data) > 3
                else [[data]])
    for p in (one, many):
        assert set(L.codecs_of(p).values()) == {5}
        assert pq.ParquetFile(p).metadata.num_row_groups == 2
        assert pq.read_table(p).equals(t)
    L.rewrite(src, one)   # nothing replaced: the same pages under re-serialised headers
    assert pq.read_table(one).equals(t)


@pytest.mark.parametrize("codec", [7, 5, "5 split"])
@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_host_decoder_reads_lz4_files_as_pyarrow(column_exe, tmp_path, codec, version):
    import pyarrow as pa
    import pyarrow.parquet as pq
    from tests.test_delta_pages_host import _parse
    cols = _table(3000)
    path = str(tmp_path / "lz.parquet")
    pq.write_table(pa.table(cols), path, compression="lz4", use_dictionary=False, data_page_version=version,
                   data_page_size=4096, write_statistics=False)
    t = pq.read_table(path)
    if codec != 7:
        split = None if codec == 5 else (lambda leaf, k, data: [[data[:100], data[100:300]], [data[300:]]] if len(data) > 300
                                         else [[data]])
        L.to_hadoop(path, path, split=split)
        assert set(L.codecs_of(path).values()) == {5}
    r = subprocess.run([column_exe, path] + list(cols), capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0, r.stderr[-3000:]
    got = _parse(r.stdout)
    for k in cols:
        want = [v.encode() if isinstance(v, str) else v for v in t.column(k).to_pylist()]
        assert [v for _, _, v in got[k]] == want, k
