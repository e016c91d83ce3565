"""The host GZIP inflater (inflate_host.cpp) through the rules of deflate_fmt.h that the device kernel
(k_inflate.hip) walks too. A stand-alone program (tests/native/inflate_host_main.cpp), built under
AddressSanitizer + UndefinedBehaviorSanitizer, inflates the corpus of tests/inflate_corpus.py: its
output must equal Python's zlib, and over thousands of single-bit and single-byte mutations it must
accept exactly what a CRC-blind reader on top of zlib's raw inflate accepts, with the same bytes. The
host column decoder reads GZIP files pyarrow wrote as pyarrow reads them."""
import os
import shutil
import subprocess
import zlib

import pytest

from tests import delta_pages_corpus as C
from tests import inflate_corpus as I
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
    return _build(tmp_path_factory.mktemp("inf"), "inflate_host_main",
                  [os.path.join(ROOT, "tests", "native", "inflate_host_main.cpp"), os.path.join(CSRC, "inflate_host.cpp")])


@pytest.fixture(scope="module")
def column_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("dph"), "delta_pages_host",
                  [os.path.join(ROOT, "tests", "native", "delta_pages_host.cpp"), os.path.join(CSRC, "parquet_meta.cpp"),
                   os.path.join(CSRC, "snappy_host.cpp")])


def inflate_all(exe, tmp_path, items):
    """[bytes or None] of the program over (n_out, stream) items; the sanitizers must stay silent."""
    path = str(tmp_path / "records.bin")
    with open(path, "wb") as f:
        f.write(I.records(items))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(items)
    return [None if ln.startswith("error") else b"" if ln == "-" else bytes.fromhex(ln) for ln in lines]


def test_corpus_equals_zlib(exe, tmp_path):
    corpus = I.streams()
    assert len(corpus) >= 60
    got = inflate_all(exe, tmp_path, [(len(data), s) for _, s, data in corpus])
    for (name, s, data), out in zip(corpus, got):
        if "/two" in name or "/three" in name:   # member by member
            want, rest = b"", s
            while rest:
                d = zlib.decompressobj(31)
                want += d.decompress(rest)
                assert d.eof
                rest = d.unused_data
        else:
            want = zlib.decompress(s, 31)
        assert want == data and out == want, name


def test_the_output_length_is_part_of_the_contract(exe, tmp_path):
    data = I.payloads(small=True)["text"]
    s = I.member(data)
    got = inflate_all(exe, tmp_path, [(len(data), s), (len(data) - 1, s), (len(data) + 1, s), (0, s), (len(data), s + b"\0"),
                                      (len(data), s[:-1]), (0, b""), (len(data), zlib.compress(data))])
    assert got == [data] + [None] * 7


def test_mutations_are_judged_as_zlib_judges_them(exe, tmp_path):
    """Ours succeeds exactly when the CRC-blind reference reaches the end of every member with the
    expected length and ISIZE, and then with the same bytes."""
    items, want = [], []
    for k, (name, s, data) in enumerate(I.streams(small=True)):
        for m in I.mutations(s, 100, seed=k):
            items.append((len(data), m))
            want.append(I.reference(m, len(data)))
    assert len(items) >= 5000
    got = inflate_all(exe, tmp_path, items)
    accepted = sum(w is not None for w in want)
    assert 0 < accepted < len(items)   # both verdicts occur
    bad = [i for i in range(len(items)) if got[i] != want[i]]
    assert not bad, "%d of %d verdicts differ, first: mutation %d (ours %s, zlib %s)" % (
        len(bad), len(items), bad[0], "accepts" if got[bad[0]] is not None else "rejects",
        "accepts" if want[bad[0]] is not None else "rejects")


def _bits(fields):
    """(value, width) fields packed LSB first, as DEFLATE packs header fields (Huffman codes go in
    bit-reversed: see _code)."""
    bits = n = 0
    for v, w in fields:
        bits |= v << n
        n += w
    return bits.to_bytes((n + 7) // 8, "little")


def _code(v, w):
    return int(format(v, "0%db" % w)[::-1], 2), w


def _fixed_match(dist_symbol):
    """A final fixed-code block: literal 'a' (code 0x30 + 97, 8 bits), length 3 (symbol 257: 7 bits),
    the distance symbol (5 bits), then zeros."""
    return _bits([(1, 1), (1, 2), _code(0x30 + 97, 8), _code(1, 7), _code(dist_symbol, 5), (0, 7)])


def malformed_bodies(data, extra=None):
    """{class: stream}: the fixed malformed page bodies the GPU suite patches into a table. Each is
    refused by the host inflater here, under the sanitizers, before any of them reaches the device.
    `extra`: a FEXTRA field for the first member's header (the GPU suite sizes the body with it)."""
    import struct
    kw = {} if extra is None else {"flags": I.FEXTRA, "extra": extra}
    start = 10 if extra is None else 12 + len(extra)      # of the first member's DEFLATE stream
    good = I.member(data, level=9, **kw)
    out = {}
    b = bytearray(good)
    b[start] |= 6                                # BTYPE = 3 in the first block header
    out["block type 3"] = bytes(b)
    st = b"\0" + struct.pack("<HH", 16, (16 ^ 0xffff) ^ 1) + data[:16]
    out["stored NLEN mismatch"] = I.member(data, raw=st + I.raw_deflate(data[16:], level=9, zdict=data[:16]), **kw)
    # a dynamic header (HLIT 0, HDIST 0, HCLEN 15) whose code-length code has three codes of one bit
    over = _bits([(1, 1), (2, 2), (0, 5), (0, 5), (15, 4)] + [(1, 3)] * 3 + [(0, 3)] * 16)
    out["over-subscribed code lengths"] = I.member(data, raw=over + b"\0" * 8, **kw)
    out["distance before the member's start"] = I.member(b"aaaa", raw=_fixed_match(1), **kw)   # distance 2 after 1 byte
    b = bytearray(good)
    b[-4] ^= 1
    out["ISIZE off by one"] = bytes(b)
    out["last 16 bytes zeroed"] = good[:-16] + b"\0" * 16
    out["bad magic"] = b"\x1f\x8c" + good[2:]
    out["zlib wrapper"] = zlib.compress(data, 9) + b"\0" * (0 if extra is None else len(extra))
    out["trailer cut"] = good[:-3] + b"\x1f\x8b\x08"
    out["reserved flag"] = good[:3] + bytes([good[3] | 0x20]) + good[4:]
    out["second member bad"] = good + good[:12]
    out["distance code 30"] = I.member(b"aaaa", raw=_fixed_match(30), **kw)
    return out


def test_malformed_classes_are_refused(exe, tmp_path):
    data = "\n".join(C.config3_paths(200, 3)).encode()
    bodies = malformed_bodies(data)
    assert len(bodies) >= 12
    sizes = {k: 4 if "distance" in k else len(data) for k in bodies}
    got = inflate_all(exe, tmp_path, [(sizes[k], s) for k, s in bodies.items()])
    assert got == [None] * len(bodies), [k for k, g in zip(bodies, got) if g is not None]
    assert all(I.reference(s, sizes[k]) is None for k, s in bodies.items())


@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("dictionary", [False, True])
def test_host_decoder_reads_gzip_files_as_pyarrow(column_exe, tmp_path, version, dictionary):
    import pyarrow as pa
    import pyarrow.parquet as pq
    n = 3000
    paths = C.config3_paths(n, 3)
    cols = {"path": pa.array([None if i % 7 == 0 else p for i, p in enumerate(paths)], pa.string()),
            "size": pa.array([(i * 7919) % 100003 for i in range(n)], pa.int64()),
            "few": pa.array(["v%d" % (i % 5) for i in range(n)], pa.string())}
    path = str(tmp_path / "gz.parquet")
    pq.write_table(pa.table(cols), path, compression="gzip", use_dictionary=dictionary, data_page_version=version,
                   data_page_size=4096, write_statistics=False)
    md = pq.ParquetFile(path).metadata
    assert md.row_group(0).column(0).compression == "GZIP"
    r = subprocess.run([column_exe, path] + list(cols), capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0, r.stderr[-3000:]
    got = _parse(r.stdout)
    t = pq.read_table(path)
    for k in cols:
        want = [v.encode() if isinstance(v, str) else v for v in t.column(k).to_pylist()]
        assert [v for _, _, v in got[k]] == want, k
