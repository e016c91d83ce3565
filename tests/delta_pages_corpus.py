"""Shared by the DELTA_* page tests (host and GPU): value sets, and byte patches that turn a valid
uncompressed single-page column chunk into a malformed one. A patch finds the chunk's packed
sequence by the header pyarrow writes (block size, 4 miniblocks, the count, the first value) and
changes single bytes; the file keeps its length, so the footer stays valid."""
import numpy as np

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
INT_COUNTS = (0, 1, 2, 32, 33, 127, 128, 129, 1025)


def uleb(v):
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def zigzag(v):
    return uleb(((v << 1) ^ (v >> 63)) & ((1 << 64) - 1))


def read_uleb(buf, pos):
    v = s = 0
    while True:
        b = buf[pos]
        pos += 1
        v |= (b & 0x7F) << s
        s += 7
        if not b & 0x80:
            return v, pos


def int_columns(n, seed):
    """{name: (arrow type name, values with None for nulls)} of n rows each."""
    rng = np.random.default_rng(seed)
    cols = {}
    for bits, lo, hi, t0 in ((64, I64_MIN, I64_MAX, 1_700_000_000_000), (32, I32_MIN, I32_MAX, 1_700_000_000)):
        t = "int%d" % bits
        cols["const%d" % bits] = (t, [7] * n)
        cols["asc%d" % bits] = (t, [t0 + 1000 * i + int(x) for i, x in enumerate(rng.integers(0, 900, n))]
                                if bits == 64 else [t0 + i for i in range(n)])
        cols["minmax%d" % bits] = (t, [lo if i % 2 == 0 else hi for i in range(n)])
        if bits == 64:
            cols["minmax32in64"] = (t, [I32_MIN if i % 2 == 0 else I32_MAX for i in range(n)])
        cols["rand%d" % bits] = (t, [int(x) for x in rng.integers(lo, hi, n, dtype=np.int64, endpoint=True)])
        vals = [int(x) for x in rng.integers(-10**6, 10**6, n)]
        nulls = rng.random(n) < 0.7
        cols["nulls%d" % bits] = (t, [None if z else v for v, z in zip(vals, nulls)])
    return cols


def config3_paths(n, seed):
    """Sorted config-3 style paths over several partition directories: the shared prefix falls at a
    partition change and rises again inside the partition."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        d, p1 = i * 9 // max(n, 1), (i * 63 // max(n, 1)) % 7
        out.append("p0=2020-01-%02d/p1=%d/part-%05d-%08x-c000.snappy.parquet" % (d + 1, p1, i, int(rng.integers(0, 1 << 32))))
    return sorted(out)


def string_columns(n, seed):
    rng = np.random.default_rng(seed)
    words = ["", "a", "é", "éa", "日本", "日本語", "日本誤", "日x", "éé", "\U0001F600", "\U0001F601"]
    cols = {
        "empty": [""] * n,
        "equal": ["part-00000-same-value.parquet"] * n,
        "noshare": ["%c%06d" % (chr(33 + (i * 7) % 90), int(x)) for i, x in enumerate(rng.integers(0, 10**6, n))],
        "oneprefix": ["part-shared-prefix-of-the-whole-page/%07d.parquet" % i for i in range(n)],
        "paths": config3_paths(n, seed),
        # neighbours share a byte prefix that ends inside a multi-byte character
        "utf8": sorted(words[int(a)] + words[int(b)] for a, b in rng.integers(0, len(words), (n, 2))),
    }
    nulls = rng.random(n) < 0.5
    cols["nulls"] = [None if z else v for v, z in zip(cols["paths"], nulls)]
    return cols


# ---- malformed pages ---------------------------------------------------------------------------------
def find_sequence(buf, lo, hi, count, first):
    """Offset of the packed sequence header (block size, 4, count, first) inside buf[lo:hi], and of
    the byte after it; exactly one. pyarrow's blocks hold 128 INT32 or 256 INT64 values."""
    found = []
    for block in (128, 256):
        hdr = uleb(block) + uleb(4) + uleb(count) + zigzag(first)
        at = buf.find(hdr, lo, hi)
        while at >= 0:
            found.append((at, at + len(hdr)))
            at = buf.find(hdr, at + 1, hi)
    assert len(found) == 1, "sequence header found %d times" % len(found)
    return found[0]


def chunk_range(path, leaf):
    import pyarrow.parquet as pq
    md = pq.ParquetFile(path).metadata
    assert md.num_row_groups == 1
    rg = md.row_group(0)
    for c in range(rg.num_columns):
        col = rg.column(c)
        if col.path_in_schema == leaf:
            assert col.compression == "UNCOMPRESSED"
            return col.data_page_offset, col.data_page_offset + col.total_compressed_size
    raise KeyError(leaf)


def patch(path, out, leaf, kind, count, first):
    """Writes `out`: `path` with one rule of the packed sequence of `leaf` broken. count / first: the
    values of the leaf's first packed sequence (for DELTA_BYTE_ARRAY the prefix lengths: first = 0)."""
    buf = bytearray(open(path, "rb").read())
    lo, hi = chunk_range(path, leaf)
    at, body = find_sequence(buf, lo, hi, count, first)
    assert count < 127 and count > 1
    if kind == "width65":          # the first miniblock's width byte
        _, w = read_uleb(buf, body)
        buf[w] = 65
    elif kind == "count+1":
        buf[at + 3] += 1
    elif kind == "prefix0=1":      # the first prefix length
        assert first == 0
        buf[at + 4] = 2            # zigzag(1)
    elif kind == "prefix>prev":    # min delta of the prefix lengths' block: +60 on every prefix
        assert buf[body] < 0x80
        buf[body] = 120            # zigzag(60)
    else:
        raise ValueError(kind)
    open(out, "wb").write(bytes(buf))


def truncate_page(path, out, leaf, cut):
    """Writes `out`: the leaf's single v1 page declares `cut` bytes fewer than it holds (its body is
    under 64 bytes and has no levels, so both sizes are one-byte varints in the page header)."""
    buf = bytearray(open(path, "rb").read())
    lo, hi = chunk_range(path, leaf)
    assert buf[lo:lo + 3] == b"\x15\x00\x15" and buf[lo + 4] == 0x15, bytes(buf[lo:lo + 8])
    size = buf[lo + 3] // 2
    assert buf[lo + 3] == buf[lo + 5] == 2 * size and size < 64 and 0 <= cut <= size
    buf[lo + 3] = buf[lo + 5] = 2 * (size - cut)
    open(out, "wb").write(bytes(buf))
    return size
