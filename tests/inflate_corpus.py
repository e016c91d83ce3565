"""Shared by the GZIP page tests (host and GPU): payloads, gzip members built by hand around zlib's
raw DEFLATE output (levels, Z_FIXED, Z_FULL_FLUSH, a stored block followed by a zdict continuation,
several members, every optional header field), a CRC-blind reference inflater on top of Python's
zlib, deterministic mutations, and the in-place replacement of a page body in a Parquet file."""
import struct
import zlib

import numpy as np

from tests import delta_pages_corpus as C

FEXTRA, FNAME, FCOMMENT, FHCRC = 4, 8, 16, 2


def text(n, seed):
    rng = np.random.default_rng(seed)
    words = [b"add", b"remove", b"path", b"partitionValues", b"size", b"modificationTime", b"dataChange", b"stats",
             b"numRecords", b"minValues", b"maxValues", b"nullCount", b"part-", b".snappy.parquet", b"2020-01-"]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, len(words)))] + (b"%d" % int(rng.integers(0, 10 ** int(rng.integers(1, 9)))))
        out.append(b' ":,{}'[int(rng.integers(0, 6))])
    return bytes(out[:n])


def far_repeat():
    """300 KiB whose second half repeats the first at distance exactly 32,768 -- in 32 KiB periods."""
    period = text(32768, 11)
    return period * 9 + period[:300 * 1024 - 9 * 32768]


def payloads(small=False):
    rng = np.random.default_rng(7)
    if small:
        return {"empty": b"", "one": b"x", "run": b"a" * 3000, "paths": "\n".join(C.config3_paths(40, 3)).encode(),
                "random": rng.integers(0, 256, 600, dtype=np.uint8).tobytes(), "text": text(2500, 5)}
    return {"empty": b"", "one": b"x", "run": b"\x07" * 65536, "paths": "\n".join(C.config3_paths(3000, 3)).encode(),
            "random": rng.integers(0, 256, 100 * 1024, dtype=np.uint8).tobytes(), "far": far_repeat()}


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, full_flush=False, zdict=None):
    kw = {"zdict": zdict} if zdict is not None else {}
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy, **kw)
    if not full_flush:
        return c.compress(data) + c.flush()
    half = len(data) // 2
    return c.compress(data[:half]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[half:]) + c.flush()


def member(data, raw=None, flags=0, extra=b"", name=b"name", comment=b"a comment", **kw):
    """One gzip member around `raw` (default: raw_deflate(data, **kw)). An `extra` beyond XLEN's 65,535
    bytes continues as a comment of the same total length (refit() pads pages with it)."""
    raw = raw_deflate(data, **kw) if raw is None else raw
    if flags & FEXTRA and len(extra) > 65535:
        assert not flags & FCOMMENT
        flags, comment, extra = flags | FCOMMENT, b"c" * (len(extra) - 65536), extra[:65535]
    head = b"\x1f\x8b\x08" + bytes([flags]) + b"\0\0\0\0\0\xff"
    if flags & FEXTRA:
        head += struct.pack("<H", len(extra)) + extra
    if flags & FNAME:
        head += name + b"\0"
    if flags & FCOMMENT:
        head += comment + b"\0"
    if flags & FHCRC:
        head += struct.pack("<H", zlib.crc32(head) & 0xffff)
    return head + raw + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def stored_then_zdict(data, level=6, cut=None):
    """A non-final stored block holding the first part, then a raw stream compressed with that part as
    its dictionary: matches reach back across the block boundary."""
    cut = min(len(data) // 3, 30000) if cut is None else min(cut, len(data))
    prefix, rest = data[:cut], data[cut:]
    return b"\0" + struct.pack("<HH", cut, cut ^ 0xffff) + prefix + raw_deflate(rest, level=level, zdict=prefix)


def variants(data):
    """{name: stream} of one payload: every framing the page tests replay. Each inflates to `data`."""
    third = len(data) // 3
    out = {"l%d" % lv: member(data, level=lv) for lv in (1, 6, 9)}
    out["fixed"] = member(data, strategy=zlib.Z_FIXED)
    out["flush"] = member(data, full_flush=True)
    out["stored+zdict"] = member(data, raw=stored_then_zdict(data))
    out["two"] = member(data[:third], level=9) + member(data[third:], level=1)
    out["three"] = member(data[:third]) + member(data[third:2 * third], strategy=zlib.Z_FIXED) + member(data[2 * third:])
    out["fields"] = member(data, flags=FEXTRA | FNAME | FCOMMENT | FHCRC, extra=b"ab\x03\x00xyz", level=9)
    out["fname+fhcrc+fextra"] = member(data, flags=FEXTRA | FNAME | FHCRC, extra=b"\0" * 300)
    return out


def streams(small=False):
    """[(name, stream, expected output)]"""
    return [("%s/%s" % (p, v), s, data) for p, data in payloads(small).items() for v, s in variants(data).items()]


def _header_end(s, pos):
    """Offset of the DEFLATE stream of the member at `pos`, or None (mirrors RFC 1952)."""
    if len(s) - pos < 10 or s[pos:pos + 3] != b"\x1f\x8b\x08" or s[pos + 3] & 0xe0:
        return None
    flg, pos = s[pos + 3], pos + 10
    if flg & FEXTRA:
        if len(s) - pos < 2:
            return None
        pos += 2 + struct.unpack_from("<H", s, pos)[0]
    for f in (FNAME, FCOMMENT):
        if flg & f:
            z = s.find(b"\0", pos)
            if z < 0:
                return None
            pos = z + 1
    if flg & FHCRC:
        pos += 2
    return pos if pos < len(s) else None


def reference(stream, n_out):
    """The bytes a CRC-blind gzip reader gives for `stream` when it must fill exactly n_out bytes, or
    None: every member's framing is stripped here and its body goes through zlib's raw inflate."""
    out, pos = bytearray(), 0
    while True:
        at = _header_end(stream, pos)
        if at is None:
            return None
        d = zlib.decompressobj(-15)
        try:
            got = d.decompress(stream[at:], n_out + 1 - len(out))
        except zlib.error:
            return None
        if not d.eof or len(d.unused_data) < 8:
            return None
        if struct.unpack("<I", d.unused_data[4:8])[0] != len(got) & 0xffffffff:
            return None
        out += got
        if len(out) > n_out:
            return None
        pos = len(stream) - len(d.unused_data) + 8
        if pos == len(stream):
            return bytes(out) if len(out) == n_out else None


def mutations(stream, count, seed):
    """`count` copies of `stream` with one bit flipped or one byte replaced: half of them in the first
    96 bytes (the headers) or the last 12 (the trailer), the others anywhere."""
    rng = np.random.default_rng(seed)
    n = len(stream)
    for k in range(count):
        edge = k % 2 == 0
        at = int(rng.integers(0, min(n, 96))) if edge and k % 8 else int(rng.integers(max(n - 12, 0), n)) if edge \
            else int(rng.integers(0, n))
        b = bytearray(stream)
        b[at] = b[at] ^ (1 << int(rng.integers(0, 8))) if k % 3 else int(rng.integers(0, 256))
        yield bytes(b)


def records(items):
    """The stand-alone program's input: <u32 n_out> <u32 n_in> <stream> per item (n_out, stream)."""
    return b"".join(struct.pack("<II", n_out, len(s)) + s for n_out, s in items)


# ---- page bodies of a Parquet file -----------------------------------------------------------------
def gzip_pages(path, leaf):
    """[(offset, compressed length, uncompressed length)] of the GZIP-compressed part of every page of
    `leaf` (all row groups): found by walking the Thrift page headers."""
    import pyarrow.parquet as pq
    md = pq.ParquetFile(path).metadata
    buf = open(path, "rb").read()
    out = []
    for g in range(md.num_row_groups):
        rg = md.row_group(g)
        for c in range(rg.num_columns):
            col = rg.column(c)
            if col.path_in_schema != leaf:
                continue
            assert col.compression == "GZIP"
            pos = col.dictionary_page_offset if col.has_dictionary_page else col.data_page_offset
            end = pos + col.total_compressed_size
            while pos < end:
                h, pos = _page_header(buf, pos)
                lv = 0
                if h["type"] == 3:   # v2: the levels stay uncompressed, and so may the values (is_compressed)
                    lv = h["v2"].get(5, 0) + h["v2"].get(6, 0)
                if h["type"] != 3 or h["v2"].get(7, 1):
                    out.append((pos + lv, h["csize"] - lv, h["usize"] - lv))
                pos += h["csize"]
    return out


def _page_header(buf, pos):
    """A Thrift compact PageHeader at pos: {type, usize, csize, v2: {field: int}} and the body's offset."""
    def struct_(pos, depth):
        fields, last = {}, 0
        while True:
            b = buf[pos]
            pos += 1
            if b == 0:
                return fields, pos
            t, delta = b & 15, b >> 4
            if delta:
                fid = last + delta
            else:
                z, pos = C.read_uleb(buf, pos)
                fid = (z >> 1) ^ -(z & 1)
            last = fid
            if t in (1, 2):
                fields[fid] = int(t == 1)
            elif t in (3,):
                fields[fid] = buf[pos]
                pos += 1
            elif t in (4, 5, 6):
                z, pos = C.read_uleb(buf, pos)
                fields[fid] = (z >> 1) ^ -(z & 1)
            elif t == 8:
                n, pos = C.read_uleb(buf, pos)
                pos += n
            elif t == 12:
                fields[fid], pos = struct_(pos, depth + 1)
            else:
                raise ValueError("thrift type %d in a page header" % t)
    f, pos = struct_(pos, 0)
    return {"type": f[1], "usize": f[2], "csize": f[3], "v2": f.get(8, {})}, pos


def refit(stream_of, data, size):
    """A stream of exactly `size` bytes that inflates to `data`: stream_of(extra) builds it with a
    FEXTRA field of `extra`, which absorbs the difference. Asserts that it fits."""
    base = len(stream_of(b""))
    assert base <= size, "the replacement (%d bytes) does not fit the page's %d" % (base, size)
    s = stream_of(b"\0" * (size - base))
    assert len(s) == size and reference(s, len(data)) == data
    return s


def replace_page(path, out, leaf, index, make):
    """Writes `out`: `path` with the GZIP body of page `index` of `leaf` replaced by make(data, size) --
    a stream of exactly the body's length, so that every header and the footer stay valid."""
    buf = bytearray(open(path, "rb").read())
    at, csize, usize = gzip_pages(path, leaf)[index]
    data = zlib.decompress(bytes(buf[at:at + csize]), 31)
    assert len(data) == usize
    new = make(data, csize)
    assert len(new) == csize
    buf[at:at + csize] = new
    open(out, "wb").write(bytes(buf))
    return data
