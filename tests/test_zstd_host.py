"""The host ZSTD decoder (zstd_host.cpp) through the rules of zstd_fmt.h that the device kernel
(k_zstd.hip) walks too. A stand-alone program (tests/native/zstd_host_main.cpp), built under
AddressSanitizer + UndefinedBehaviorSanitizer, decodes the corpus of tests/zstd_corpus.py: its output
must equal the reference's (the libzstd inside pyarrow), and over thousands of single-bit and
single-byte mutations it must accept exactly what the reference accepts, with the same bytes. The host
column decoder reads ZSTD files pyarrow wrote as pyarrow reads them.

The reference is libzstd 1.5.7 on a CPU with BMI2: four Huffman streams of eight bytes or more each go
through its loop that does not look for a stream's end, which zst::huf_loose4 reproduces (DESIGN
section 2). Measured there: 0 of the 11,200 mutations of the small streams and 0 of the mutations of the
large streams drawn below differ, in verdict or in bytes; none falls under the tolerated class."""
import os
import shutil
import subprocess

import pytest

from tests import delta_pages_corpus as C
from tests import zstd_corpus as Z
from tests.test_delta_pages_host import _parse

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
    return _build(tmp_path_factory.mktemp("zst"), "zstd_host_main",
                  [os.path.join(ROOT, "tests", "native", "zstd_host_main.cpp"), os.path.join(CSRC, "zstd_host.cpp")])


@pytest.fixture(scope="module")
def column_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("dph"), "delta_pages_host",
                  [os.path.join(ROOT, "tests", "native", "delta_pages_host.cpp"), os.path.join(CSRC, "parquet_meta.cpp"),
                   os.path.join(CSRC, "snappy_host.cpp")])


def decode_all(exe, tmp_path, items):
    """[bytes or None] of the program over (n_out, stream) items; the sanitizers must stay silent."""
    path = str(tmp_path / "records.bin")
    with open(path, "wb") as f:
        f.write(Z.records(items))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(items)
    return [None if ln.startswith("error") else b"" if ln == "-" else bytes.fromhex(ln) for ln in lines]


@pytest.fixture(scope="module")
def corpus():
    return Z.streams()


def test_corpus_equals_the_reference(exe, tmp_path, corpus):
    assert len(corpus) >= 60
    got = decode_all(exe, tmp_path, [(len(data), s) for _, s, data in corpus])
    for (name, s, data), out in zip(corpus, got):
        assert Z.reference(s, len(data)) == data and out == data, name


def test_the_corpus_uses_every_feature_of_the_format(corpus):
    feats = set()
    for _, s, _ in corpus:
        feats |= Z.walk(s)[1]
    assert not Z.FEATURES - feats, sorted(Z.FEATURES - feats)
    # what libzstd itself supplies, not only the hand-assembled frames
    own = set()
    for name, s, _ in corpus:
        if "hand/" not in name and "crafted/" not in name and "raw+rle" not in name:
            own |= Z.walk(s)[1]
    assert {"block:raw", "block:rle", "literals:raw", "literals:compressed", "literals:treeless", "streams:1", "streams:4",
            "weights:fse", "mode:predefined", "mode:rle", "mode:fse", "mode:repeat"} <= own, sorted(own)


def test_the_output_length_is_part_of_the_contract(exe, tmp_path):
    data = Z.payloads(small=True)["text"]
    s = Z.one_shot(data)
    items = [(len(data), s), (len(data) - 1, s), (len(data) + 1, s), (0, s), (len(data), s + b"\0"), (len(data), s[:-1]),
             (0, b""), (1, b"")]
    got = decode_all(exe, tmp_path, items)
    assert got == [data] + [None] * 5 + [b"", None]
    assert [Z.reference(m, n) for n, m in items] == got


def _environment():
    """What decides which of libzstd's Huffman decoders the reference runs: for the failure message."""
    try:
        bmi2 = "bmi2" in open("/proc/cpuinfo").read().split()
    except OSError:
        bmi2 = None
    import pyarrow as pa
    return "pyarrow %s, CPU BMI2: %s, reference decodes four streams without an end check: %s" % (
        pa.__version__, bmi2, Z.reference_is_loose())


def test_mutations_are_judged_as_the_reference_judges_them(exe, tmp_path, corpus):
    """Ours succeeds exactly when the reference does, and then with the same bytes: 100 mutations of
    each small stream, and 4 of each large corpus stream (5-byte literals headers, Treeless literals,
    Repeat tables, literals sections of tens of KiB). A must-accept failure is never tolerated. A stream
    we accept and the reference refuses is tolerated only in a class a structural predicate recognises,
    and at most 2 % of the mutations may fall under it:
      - Z.two_symbol_eligible: libzstd may decode the section with its two-symbol decoder, whose loop's
        own refusals are not reproduced;
      - where the reference turns out not to run its four-stream loop at all (another libzstd, or a CPU
        without BMI2: probed, not assumed), Z.loose_eligible: the sections that loop would decode."""
    items, want = [], []
    for k, (name, s, data) in enumerate(Z.streams(small=True)):
        for m in Z.mutations(s, 100, seed=k):
            items.append((len(data), m))
    small = len(items)
    assert small >= 5000
    for k, (name, s, data) in enumerate(corpus):
        if 2000 < len(s) < 400000:
            for m in Z.mutations(s, 4, seed=5000 + k):
                items.append((len(data), m))
    assert len(items) - small >= 200
    want = [Z.reference(m, n) for n, m in items]
    got = decode_all(exe, tmp_path, items)
    accepted = sum(w is not None for w in want)
    assert 0 < accepted < len(items)   # both verdicts occur
    loose = Z.reference_is_loose()
    differ = [i for i in range(len(items)) if got[i] != want[i]]
    tolerated = [i for i in differ if want[i] is None and got[i] is not None and
                 (Z.two_symbol_eligible(items[i][1]) or (not loose and Z.loose_eligible(items[i][1])))]
    bad = [i for i in differ if i not in tolerated]
    print("%d mutations (%d of large streams), %d accepted by the reference, %d verdicts differ, %d of them tolerated; %s"
          % (len(items), len(items) - small, accepted, len(differ), len(tolerated), _environment()))
    assert not bad, "%d of %d verdicts differ, first: mutation %d (ours %s, reference %s); %s" % (
        len(bad), len(items), bad[0], "accepts" if got[bad[0]] is not None else "refuses",
        "accepts" if want[bad[0]] is not None else "refuses", _environment())
    assert len(tolerated) <= len(items) // 50, (len(tolerated), len(items), _environment())


def malformed_bodies(size=None):
    """{class: stream}: the fixed malformed page bodies the GPU suite patches into a table. Each is
    refused by the host decoder here, under the sanitizers, before any of them reaches the device. A
    body is an empty frame (so that the first frame header, which the page planner checks on the host,
    is good), a skippable frame that brings it to `size` bytes, and the malformed part."""
    import struct
    F = Z.frame
    good = b"hello, hello, hello"
    out = {}
    out["block type 3"] = F(Z.block(3, b"abc", last=True), b"abc", fcs=0)
    out["block size beyond the input"] = F(Z.block(0, b"abc", size=100, last=True), b"abc", fcs=0)
    out["block size over 128 KiB"] = F(Z.block(2, b"\0" * (128 * 1024 + 1), last=True), b"", fcs=0)
    out["block size over the window"] = F(Z.block(2, Z.rle_sequences(b"abcdefghabcdefgh", [(4, 2, 1, 2)]), last=True),
                                          b"abcdefghij", fcs=1)
    out["reserved descriptor bit"] = F(Z.raw_blocks(good), good, descriptor_or=0x08)
    out["bad magic"] = b"\x29" + F(Z.raw_blocks(good), good)[1:]
    out["non-zero dictionary ID"] = F(Z.raw_blocks(good), good, dict_id=7)
    lit = Z.huffman_literals(b"abba" * 5)
    assert lit[3 + 1 + 48] == 0x01            # the byte that holds the weights of symbols 96 and 97
    out["Huffman weights do not sum to a power of two"] = F(Z.block(2, lit[:52] + b"\x31" + lit[53:], last=True), b"", fcs=0)
    out["FSE accuracy log over the limit"] = F(Z.block(2, b"\0\x01\x80\x05\0\0\0\x01", last=True), b"", fcs=0)
    out["offset before the start of the output"] = F(Z.block(2, Z.rle_sequences(b"abcd", [(4, 4, 0, 2)]), last=True), b"", fcs=0)
    body = Z.rle_sequences(b"abcdefgh", [(4, 2, 1, 2)])
    out["sequence bitstream ends in a zero byte"] = F(Z.block(2, body[:-1] + b"\0", last=True), b"", fcs=0)
    out["literal length beyond the literals"] = F(Z.block(2, Z.rle_sequences(b"ab", [(4, 2, 0, 2)]), last=True), b"", fcs=0)
    out["content size off by one"] = F(Z.raw_blocks(good), good + b"!", fcs=4)
    b = bytearray(F(Z.raw_blocks(good), good, checksum=True))
    b[-1] ^= 1
    out["checksum mismatch"] = bytes(b)
    out["Treeless literals in a frame's first block"] = F(Z.block(2, struct.pack("<I", 3 | 4 << 4 | 2 << 14)[:3] +
                                                                  b"\x01\x01\0", last=True), b"", fcs=0)
    out["Repeat table in a frame's first block"] = F(Z.block(2, b"\0\x01\xc0\x01", last=True), b"", fcs=0)
    out["trailing bytes after the last frame"] = F(Z.raw_blocks(good), good) + b"\0"
    empty = F(Z.block(0, b"", last=True), b"")
    if size is not None:
        out = {k: Z.pad_to(empty, size - len(v), front=False) + v for k, v in out.items() if len(v) + 17 <= size}
    return out


MALFORMED = ["block type 3", "block size beyond the input", "block size over 128 KiB", "block size over the window",
             "reserved descriptor bit", "bad magic", "non-zero dictionary ID", "Huffman weights do not sum to a power of two",
             "FSE accuracy log over the limit", "offset before the start of the output",
             "sequence bitstream ends in a zero byte", "literal length beyond the literals", "content size off by one",
             "checksum mismatch", "Treeless literals in a frame's first block", "Repeat table in a frame's first block",
             "trailing bytes after the last frame"]


@pytest.mark.parametrize("size", [None, 200000])
def test_malformed_classes_are_refused(exe, tmp_path, size):
    bodies = malformed_bodies(size)
    assert sorted(bodies) == sorted(MALFORMED) and len(bodies) >= 16
    for n_out in (19, 0, 13):
        got = decode_all(exe, tmp_path, [(n_out, s) for s in bodies.values()])
        assert got == [None] * len(bodies), [k for k, g in zip(bodies, got) if g is not None]
        assert all(Z.reference(s, n_out) is None for s in bodies.values())


@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("dictionary", [False, True])
def test_host_decoder_reads_zstd_files_as_pyarrow(column_exe, tmp_path, version, dictionary):
    import pyarrow as pa
    import pyarrow.parquet as pq
    n = 3000
    paths = C.config3_paths(n, 3)
    cols = {"path": pa.array([None if i % 7 == 0 else p for i, p in enumerate(paths)], pa.string()),
            "size": pa.array([(i * 7919) % 100003 for i in range(n)], pa.int64()),
            "few": pa.array(["v%d" % (i % 5) for i in range(n)], pa.string())}
    path = str(tmp_path / "zs.parquet")
    pq.write_table(pa.table(cols), path, compression="zstd", use_dictionary=dictionary, data_page_version=version,
                   data_page_size=4096, write_statistics=False)
    md = pq.ParquetFile(path).metadata
    assert md.row_group(0).column(0).compression == "ZSTD"
    r = subprocess.run([column_exe, path] + list(cols), capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0, r.stderr[-3000:]
    got = _parse(r.stdout)
    t = pq.read_table(path)
    for k in cols:
        want = [v.encode() if isinstance(v, str) else v for v in t.column(k).to_pylist()]
        assert [v for _, _, v in got[k]] == want, k
