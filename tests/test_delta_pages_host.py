"""The host decoder (parquet_meta.cpp) on DELTA_BINARY_PACKED, DELTA_LENGTH_BYTE_ARRAY and
DELTA_BYTE_ARRAY pages, through the rules of delta_enc.h that the device kernels run too. A
stand-alone program (tests/native/delta_pages_host.cpp) prints leaves of files pyarrow wrote here; its
output must equal pyarrow's own read of them. The program is built under AddressSanitizer +
UndefinedBehaviorSanitizer, so a read out of range on a malformed page fails the run."""
import os
import shutil
import subprocess

import pytest

from tests import delta_pages_corpus as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "delta_amd", "csrc")
SRCS = [os.path.join(ROOT, "tests", "native", "delta_pages_host.cpp"), os.path.join(CSRC, "parquet_meta.cpp"),
        os.path.join(CSRC, "snappy_host.cpp")]
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
FRAMINGS = [(v, c) for v in ("1.0", "2.0") for c in ("snappy", "none")]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dph") / "delta_pages_host")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "include")] + ASAN + SRCS + ["-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _run(exe, path, leaves):
    return subprocess.run([exe, path] + list(leaves), capture_output=True, text=True, timeout=120, env=ENV)


def _parse(stdout):
    """{leaf: [(def, rep, value)]}: value None, int or bytes."""
    out, cur, it = {}, None, iter(stdout.splitlines())
    for line in it:
        if line.startswith("leaf "):
            cur = out.setdefault(line[5:], [])
            assert next(it).startswith("levels ")
        elif line != "ok":
            d, r, v = line.split(" ")
            cur.append((int(d), int(r), None if v == "-" else bytes.fromhex(v[1:]) if v[0] == "x" else int(v)))
    return out


def _write(path, cols, encodings, version, codec, **kw):
    import pyarrow as pa
    import pyarrow.parquet as pq
    table = pa.table(cols)
    pq.write_table(table, path, compression=codec, use_dictionary=False, data_page_version=version,
                   data_page_size=4096, column_encoding=encodings, write_statistics=False, **kw)
    return table


def _values(got):
    return [v for _, _, v in got]


@pytest.mark.parametrize("version,codec", FRAMINGS)
def test_delta_binary_packed_matches_pyarrow(exe, tmp_path, version, codec):
    import pyarrow as pa
    import pyarrow.parquet as pq
    for n in C.INT_COUNTS:
        spec = C.int_columns(n, seed=n)
        if n == 0:  # a sequence of no value: a page of nulls only
            spec = {k: (t, [None] * 5) for k, (t, _) in spec.items()}
        rows = max(n, 5) if n == 0 else n
        cols = {k: pa.array(v, getattr(pa, t)()) for k, (t, v) in spec.items()}
        # one leaf below a nullable struct: definition levels above 1
        inner = pa.array(spec["rand64"][1], pa.int64())
        cols["s"] = pa.StructArray.from_arrays([inner], names=["a"],
                                               mask=pa.array([i % 3 == 0 for i in range(rows)], pa.bool_()))
        enc = {k: "DELTA_BINARY_PACKED" for k in spec}
        enc["s.a"] = "DELTA_BINARY_PACKED"
        path = str(tmp_path / ("ints_%d.parquet" % n))
        _write(path, cols, enc, version, codec)
        r = _run(exe, path, list(enc))
        assert r.returncode == 0, (n, r.stderr[-2000:])
        got = _parse(r.stdout)
        back = pq.read_table(path)
        for k in spec:
            assert _values(got[k]) == back.column(k).to_pylist(), (n, k)
        want = [None if s is None else s["a"] for s in back.column("s").to_pylist()]
        assert _values(got["s.a"]) == want, n


@pytest.mark.parametrize("encoding", ["DELTA_LENGTH_BYTE_ARRAY", "DELTA_BYTE_ARRAY"])
@pytest.mark.parametrize("version,codec", FRAMINGS)
def test_delta_strings_match_pyarrow(exe, tmp_path, version, codec, encoding):
    import pyarrow as pa
    import pyarrow.parquet as pq
    n = 3000
    spec = C.string_columns(n, seed=11)
    cols = {k: pa.array(v, pa.string()) for k, v in spec.items()}
    cols["keys"] = pa.array([[spec["paths"][i], spec["utf8"][i]][:i % 3] for i in range(n)], pa.list_(pa.string()))
    enc = {k: encoding for k in spec}
    enc["keys.list.element"] = encoding
    path = str(tmp_path / "strings.parquet")
    # every column but one spans many 4 KiB pages; "oneprefix" keeps its 3,000 values in one page
    _write(path, cols, enc, version, codec, write_batch_size=64)
    one = str(tmp_path / "one.parquet")
    pq.write_table(pa.table({"oneprefix": cols["oneprefix"]}), one, compression=codec, use_dictionary=False,
                   data_page_version=version, column_encoding={"oneprefix": encoding}, write_statistics=False)
    assert pq.ParquetFile(one).metadata.row_group(0).column(0).total_uncompressed_size > 3000
    r = _run(exe, path, list(enc))
    assert r.returncode == 0, r.stderr[-2000:]
    got = _parse(r.stdout)
    back = pq.read_table(path)
    for k in spec:
        want = [None if v is None else v.encode() for v in back.column(k).to_pylist()]
        assert _values(got[k]) == want, k
    flat = [v.encode() for row in back.column("keys").to_pylist() for v in row]
    assert [v for v in _values(got["keys.list.element"]) if v is not None] == flat
    r = _run(exe, one, ["oneprefix"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert _values(_parse(r.stdout)["oneprefix"]) == [v.encode() for v in spec["oneprefix"]]


def _required(name, typ):
    import pyarrow as pa
    return pa.schema([pa.field(name, typ, nullable=False)])


def _small_file(path, name, values, typ, encoding):
    """One required column in one uncompressed v1 page: the page body is the value region."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    table = pa.Table.from_arrays([pa.array(values, typ)], schema=_required(name, typ))
    pq.write_table(table, path, compression="none", use_dictionary=False, data_page_version="1.0",
                   column_encoding={name: encoding}, write_statistics=False)


def _refused(exe, path, leaf):
    r = _run(exe, path, [leaf])
    assert r.returncode == 3 and r.stderr.startswith("DR_E_PARQUET: "), (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


def test_malformed_pages_are_refused(exe, tmp_path):
    import pyarrow as pa
    ints = [1000 + 37 * i * i for i in range(40)]
    strs = ["p=1/part-%03d" % (i * i) for i in range(40)]
    fi, fs = str(tmp_path / "i.parquet"), str(tmp_path / "s.parquet")
    _small_file(fi, "v", ints, pa.int64(), "DELTA_BINARY_PACKED")
    _small_file(fs, "v", strs, pa.string(), "DELTA_BYTE_ARRAY")
    for f in (fi, fs):
        assert _run(exe, f, ["v"]).returncode == 0
    bad = str(tmp_path / "bad.parquet")
    for src, kind, first in ((fi, "width65", ints[0]), (fi, "count+1", ints[0]), (fs, "width65", 0), (fs, "count+1", 0),
                             (fs, "prefix0=1", 0), (fs, "prefix>prev", 0)):
        C.patch(src, bad, "v", kind, 40, first)
        _refused(exe, bad, "v")


@pytest.mark.parametrize("encoding", ["DELTA_BINARY_PACKED", "DELTA_LENGTH_BYTE_ARRAY", "DELTA_BYTE_ARRAY"])
def test_every_truncation_of_a_small_page_is_refused(exe, tmp_path, encoding):
    import pyarrow as pa
    src, bad = str(tmp_path / "t.parquet"), str(tmp_path / "bad.parquet")
    if encoding == "DELTA_BINARY_PACKED":
        _small_file(src, "v", [5, 9, 2, 40, 41, 7], pa.int32(), encoding)
    else:
        _small_file(src, "v", ["ab", "abc", "abd", "b"], pa.string(), encoding)
    size = C.truncate_page(src, bad, "v", 0)
    assert _run(exe, bad, ["v"]).returncode == 0   # the patch itself keeps a whole page readable
    for cut in range(1, size + 1):   # cut = 1: the last block loses its last byte
        C.truncate_page(src, bad, "v", cut)
        _refused(exe, bad, "v")
