"""Shared by the LZ4 page tests (host and GPU): payloads, bare LZ4 blocks built from explicit sequence
lists, a small greedy compressor whose choices the tests steer, Hadoop's unit framing (Parquet codec 5),
a format walk, the reference (pyarrow's liblz4 per block, the unit grammar applied here), deterministic
mutations, and a Parquet file rewriter that replaces page bodies of any length and re-serialises the
page headers and the footer (a Thrift compact reader / writer)."""
import struct

import numpy as np

from tests import delta_pages_corpus as C
from tests.inflate_corpus import text

BARE, HADOOP = 0, 1


# ---- blocks ----------------------------------------------------------------------------------------
def _length(v):
    """The extension bytes of a length whose nibble is 15: v is the length minus 15."""
    return b"\xff" * (v // 255) + bytes([v % 255])


def encode(seqs):
    """A bare block from [(literals, offset, match length)]; the last entry's offset and match length
    are 0 (literals only)."""
    out = bytearray()
    for k, (lits, off, ml) in enumerate(seqs):
        last = k == len(seqs) - 1
        assert (off == 0 and ml == 0) if last else (ml >= 4 and 0 <= off <= 65535)
        ll, m = len(lits), 0 if last else ml - 4
        out.append(min(ll, 15) << 4 | min(m, 15))
        if ll >= 15:
            out += _length(ll - 15)
        out += lits
        if not last:
            out += struct.pack("<H", off)
            if m >= 15:
                out += _length(m - 15)
    return bytes(out)


def decode_seqs(seqs):
    """What [(literals, offset, match length)] stands for."""
    out = bytearray()
    for lits, off, ml in seqs:
        out += lits
        for _ in range(ml):
            out.append(out[-off])
    return bytes(out)


def compress(data, offsets=(), max_ml=None, min_ll=0, last=5, far_from=0):
    """A greedy compressor: [(literals, offset, match length)] for `data`. At every position it tries the
    distances of `offsets` first (so that a block shows them wherever the data allows), then the most
    recent earlier occurrence of the next four bytes -- the latter only from position `far_from` on, so
    that a block can hold period matches first and far matches behind them. liblz4's end conditions hold:
    no match starts in the last 12 bytes or reaches into the last `last` (5)."""
    n, seqs, table, i, anchor = len(data), [], {}, 0, 0
    while i + 12 <= n:
        cand = [i - d for d in offsets if 0 < d <= i] + ([table[data[i:i + 4]]] if data[i:i + 4] in table and i >= far_from else [])
        table[data[i:i + 4]] = i
        best = None
        for c in cand:
            if i - c > 65535 or data[c:c + 4] != data[i:i + 4] or i - anchor < min_ll:
                continue
            ml = 4
            while i + ml < n - last and data[c + ml] == data[i + ml]:
                ml += 1
            if max_ml:
                ml = min(ml, max_ml)
            if i + ml <= n - last:
                best = (c, ml)
                break
        if best is None:
            i += 1
            continue
        seqs.append((data[anchor:i], i - best[0], best[1]))
        i += best[1]
        anchor = i
    seqs.append((data[anchor:], 0, 0))
    assert decode_seqs(seqs) == data
    return seqs


def seqs_of(block):
    """[(literals, offset, match length)] of a bare block, as encode() takes them."""
    return [(block[lit:lit + ll], off, ml) for lit, ll, off, ml in walk(block)["seqs"]]


def hadoop(units):
    """A codec-5 body from [[bare block, ...], ...] or [(U, [bare block, ...]), ...]: U defaults to
    what the unit's blocks decode to."""
    out = bytearray()
    for u in units:
        U, blocks = u if isinstance(u, tuple) else (sum(walk(b)["size"] for b in u), u)
        out += struct.pack(">I", U)
        for b in blocks:
            out += struct.pack(">I", len(b)) + b
    return bytes(out)


def walk(block):
    """The format walk of a bare block, with no rule but the input's end: {seqs: [(literal position,
    literal length, offset, match length)], size, heads: positions of tokens, length bytes and
    offsets}, or None when a sequence runs off the input."""
    n, ip, seqs, heads, size = len(block), 0, [], [], 0
    while True:
        if ip >= n:
            return None
        t = block[ip]
        heads.append(ip)
        ip += 1
        ll = t >> 4
        if ll == 15:
            while True:
                if ip >= n:
                    return None
                heads.append(ip)
                ll += block[ip]
                ip += 1
                if block[ip - 1] != 255:
                    break
        if ip + ll > n:
            return None
        lit = ip
        ip += ll
        size += ll
        if ip == n:
            seqs.append((lit, ll, 0, 0))
            return {"seqs": seqs, "size": size, "heads": heads}
        if ip + 2 > n:
            return None
        heads += [ip, ip + 1]
        off = block[ip] | block[ip + 1] << 8
        ip += 2
        ml = t & 15
        if ml == 15:
            while True:
                if ip >= n:
                    return None
                heads.append(ip)
                ml += block[ip]
                ip += 1
                if block[ip - 1] != 255:
                    break
        ml += 4
        seqs.append((lit, ll, off, ml))
        size += ml


def units_of(body):
    """[(U, [(position, C)])] of a codec-5 body as far as its words parse, and the word positions."""
    pos, units, heads = 0, [], []
    while pos + 8 <= len(body):
        U = struct.unpack_from(">I", body, pos)[0]
        heads += range(pos, pos + 4)
        pos += 4
        blocks, left = [], U
        while left > 0 and pos + 4 <= len(body):
            c = struct.unpack_from(">I", body, pos)[0]
            heads += range(pos, pos + 4)
            pos += 4
            if c > len(body) - pos:
                return units + [(U, blocks)], heads
            w = walk(body[pos:pos + c])
            blocks.append((pos, c))
            pos += c
            if w is None or w["size"] == 0 or w["size"] > left:
                return units + [(U, blocks)], heads
            left -= w["size"]
        units.append((U, blocks))
    return units, heads


def zero_offset(body, framing):
    """The structural predicate of the one tolerated class: a sequence of the body has offset 0, which
    liblz4 does not look at (it copies what its destination held) and lz4_fmt.h refuses."""
    blocks = [body] if framing == BARE else [body[p:p + c] for _, bl in units_of(body)[0] for p, c in bl]
    for b in blocks:
        w = walk(b)
        if w and any(off == 0 and ml for _, _, off, ml in w["seqs"]):
            return True
    return False


_codec = None


def _block(block, cap):
    """liblz4's LZ4_decompress_safe of one bare block into `cap` bytes: the bytes it produced, or None.
    pyarrow hands back the whole destination, so the produced length comes from the format walk."""
    global _codec
    import pyarrow as pa
    if _codec is None:
        _codec = pa.Codec("lz4_raw")
    try:
        got = _codec.decompress(block, decompressed_size=cap, asbytes=True)
    except Exception:
        return None
    w = walk(block)
    assert w is not None and w["size"] <= cap, "liblz4 accepted a block the format walk cannot follow"
    return got[:w["size"]]


def reference(body, n_out, framing):
    """The bytes the reference gives for a page body that must fill exactly n_out bytes, or None. Framing
    BARE: one block, liblz4's capacity n_out. HADOOP: the unit grammar, every inner block through liblz4
    with the capacity that is left of its unit."""
    if framing == BARE:
        got = _block(body, n_out)
        return got if got is not None and len(got) == n_out else None
    out, pos, n = bytearray(), 0, len(body)
    while pos < n:
        if n - pos < 8:
            return None
        U = struct.unpack_from(">I", body, pos)[0]
        pos += 4
        if U == 0 or U > n_out - len(out):
            return None
        left = U
        while left:
            if n - pos < 4:
                return None
            c = struct.unpack_from(">I", body, pos)[0]
            pos += 4
            if c > n - pos:
                return None
            got = _block(body[pos:pos + c], left)
            if got is None:
                return None
            pos += c
            out += got
            left -= len(got)
    return bytes(out) if len(out) == n_out else None


# ---- the corpus ------------------------------------------------------------------------------------
def far_repeat(distance):
    """200 KiB in which every byte repeats the one `distance` before it."""
    period = text(distance, 13)
    return (period * (200 * 1024 // distance + 1))[:200 * 1024]


def payloads():
    rng = np.random.default_rng(7)
    out = {"empty": b"", "text": text(20000, 5), "paths": "\n".join(C.config3_paths(1500, 3)).encode(),
           "far65535": far_repeat(65535), "far65536": far_repeat(65536), "run": b"\x07" * 70000,
           "runs": b"ab" * 500 + b"xyz" * 400 + b"q" * 300 + text(100, 1),
           "random": rng.integers(0, 256, 5000, dtype=np.uint8).tobytes()}
    for k in range(1, 14):
        out["tiny%d" % k] = text(k, k)
    return out


def pyarrow_block(data, level=None):
    import pyarrow as pa
    c = pa.Codec("lz4_raw") if level is None else pa.Codec("lz4_raw", compression_level=level)
    return c.compress(data, asbytes=True)


def crafted():
    """{name: (block, expected output)}: what a compressor rarely writes."""
    out = {}
    pre = text(40, 2)

    def add(name, seqs):
        out[name] = (encode(seqs), decode_seqs(seqs))
    tail = b"12345"
    for off in (1, 2, 3):
        add("offset %d" % off, [(pre, off, 40), (tail + b"6789012", 0, 0)])
    big = text(65535, 3)
    add("offset 65535", [(big, 65535, 100), (b"x" * 12, 0, 0)])
    for ext, v in ((0, 14), (1, 15), (1, 15 + 254), (2, 15 + 255), (3, 15 + 255 * 2), (3, 15 + 255 * 2 + 7)):
        add("literal length %d (%d extension bytes)" % (v, ext), [(text(v, v), 3, 8), (b"y" * 12, 0, 0)])
        add("match length %d (%d extension bytes)" % (v + 4, ext), [(pre, 7, v + 4), (b"z" * 12, 0, 0)])
    # the last place a match may end: five literals behind it, and its start twelve bytes before the end
    add("match ends at the last permitted position", [(pre, 4, 7), (tail, 0, 0)])
    add("last literals of length 15", [(pre, 4, 30), (text(15, 4), 0, 0)])
    add("literals only", [(text(300, 6), 0, 0)])
    return out


def corpus():
    """[(name, body, framing, expected output)]"""
    out = []
    for name, data in payloads().items():
        for tag, level in (("default", None), ("l12", 12)):
            out.append(("%s/%s" % (name, tag), pyarrow_block(data, level), BARE, data))
    for name, (block, data) in crafted().items():
        out.append(("crafted/" + name, block, BARE, data))
    p = payloads()
    a, b, c = p["text"][:3000], p["paths"][:4000], p["runs"]
    blk = pyarrow_block
    out.append(("hadoop/one unit", hadoop([[blk(a)]]), HADOOP, a))
    out.append(("hadoop/three units", hadoop([[blk(a)], [blk(b, 12)], [blk(c)]]), HADOOP, a + b + c))
    out.append(("hadoop/one unit of three inner blocks", hadoop([[blk(a), blk(b), blk(c)]]), HADOOP, a + b + c))
    # boundaries directly after a match: a block that ends in a match and an empty literal run, which
    # liblz4 accepts while the capacity (what is left of the unit) lies further on and the literal run
    # before the match is one its first loop does not check (below 15, 17 bytes of input behind the token)
    m = encode([(a[:14], 3, 18), (b"", 0, 0)])
    md = decode_seqs([(a[:14], 3, 18)])
    out.append(("hadoop/inner boundary after a match", hadoop([[m, blk(b)]]), HADOOP, md + b))
    out.append(("hadoop/unit boundary after a match", hadoop([[m, blk(c)], [blk(a)]]), HADOOP, md + c + a))
    out.append(("hadoop/empty page", b"", HADOOP, b""))
    return out


def mutations(stream, count, seed, framing=BARE):
    """`count` copies of `stream` with one bit flipped or one byte replaced: half of them in the tokens,
    length bytes, offsets and framing words, the others anywhere; every eighth loses or gains a byte at
    its end instead."""
    rng = np.random.default_rng(seed)
    n = len(stream)
    if framing == BARE:
        w = walk(stream)
        heads = w["heads"] if w else []
    else:
        units, heads = units_of(stream)
        heads = list(heads)
        for _, blocks in units:
            for p, c in blocks:
                w = walk(stream[p:p + c])
                heads += [p + h for h in (w["heads"] if w else [])]
    for k in range(count):
        if n == 0 or k % 8 == 7:
            yield stream[:-1] if k % 16 == 7 and n else stream + bytes([int(rng.integers(0, 256))])
            continue
        at = heads[int(rng.integers(0, len(heads)))] if k % 2 == 0 and heads else int(rng.integers(0, n))
        b = bytearray(stream)
        b[at] = b[at] ^ (1 << int(rng.integers(0, 8))) if k % 3 else int(rng.integers(0, 256))
        yield bytes(b)


def records(items):
    """The stand-alone program's input: <u32 n_out> <u32 n_in> <u8 framing> <stream> per item
    (n_out, framing, stream)."""
    return b"".join(struct.pack("<IIB", n_out, len(s), framing) + s for n_out, framing, s in items)


# ---- Thrift compact, as far as Parquet's metadata goes -------------------------------------------------
def _zz(v):
    return C.uleb((v << 1) ^ (v >> 63))


def t_read(buf, pos):
    """A struct at pos: ([(field id, type, value)], end). Values: bool, int, bytes, (element type, [values])
    for lists, a field list for structs."""
    def value(t, pos):
        if t in (1, 2):
            return t == 1, pos
        if t == 3:
            return buf[pos], pos + 1
        if t in (4, 5, 6):
            z, pos = C.read_uleb(buf, pos)
            return (z >> 1) ^ -(z & 1), pos
        if t == 7:
            return bytes(buf[pos:pos + 8]), pos + 8
        if t == 8:
            n, pos = C.read_uleb(buf, pos)
            return bytes(buf[pos:pos + n]), pos + n
        if t in (9, 10):
            h = buf[pos]
            pos += 1
            n, et = h >> 4, h & 15
            if n == 15:
                n, pos = C.read_uleb(buf, pos)
            vals = []
            for _ in range(n):
                if et in (1, 2):
                    vals.append(buf[pos] == 1)
                    pos += 1
                else:
                    v, pos = value(et, pos)
                    vals.append(v)
            return (et, vals), pos
        if t == 12:
            return t_read(buf, pos)
        raise ValueError("thrift type %d" % t)
    fields, last = [], 0
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
        v, pos = value(t, pos)
        fields.append((fid, t, v))


def t_write(fields):
    def value(t, v):
        if t in (1, 2):
            return b""
        if t == 3:
            return bytes([v])
        if t in (4, 5, 6):
            return bytes(_zz(v))
        if t == 7:
            return v
        if t == 8:
            return bytes(C.uleb(len(v))) + v
        if t in (9, 10):
            et, vals = v
            head = bytes([len(vals) << 4 | et]) if len(vals) < 15 else bytes([0xf0 | et]) + bytes(C.uleb(len(vals)))
            return head + b"".join(bytes([1 if x else 2]) if et in (1, 2) else value(et, x) for x in vals)
        if t == 12:
            return t_write(v)
        raise ValueError("thrift type %d" % t)
    out, last = bytearray(), 0
    for fid, t, v in fields:
        if t in (1, 2):
            t = 1 if v else 2
        d = fid - last
        out += bytes([d << 4 | t]) if 0 < d <= 15 else bytes([t]) + bytes(_zz(fid))
        out += value(t, v)
        last = fid
    return bytes(out) + b"\0"


def _get(fields, fid, default=None):
    return next((v for f, _, v in fields if f == fid), default)


def _set(fields, fid, value):
    for k, (f, t, _) in enumerate(fields):
        if f == fid:
            fields[k] = (f, t, value)
            return
    raise KeyError(fid)


def _footer(buf):
    n = struct.unpack_from("<I", buf, len(buf) - 8)[0]
    assert buf[-4:] == b"PAR1"
    return t_read(buf, len(buf) - 8 - n)[0], len(buf) - 8 - n


def _chunks(buf):
    """[(row group fields, chunk fields, metadata fields, leaf, start, end)] in file order."""
    meta, _ = _footer(buf)
    out = []
    for rg in _get(meta, 4)[1]:
        for cc in _get(rg, 1)[1]:
            md = _get(cc, 3)
            start = _get(md, 9)
            d = _get(md, 11)
            if d is not None and 0 < d < start:
                start = d
            leaf = ".".join(p.decode() for p in _get(md, 3)[1])
            out.append((rg, cc, md, leaf, start, start + _get(md, 7)))
    return meta, out


def _pages(buf, start, end):
    """[(header fields, body position, levels prefix, values compressed)] of a chunk."""
    out, pos = [], start
    while pos < end:
        h, pos = t_read(buf, pos)
        v2 = _get(h, 8)
        lv = (_get(v2, 5, 0) + _get(v2, 6, 0)) if v2 is not None else 0
        out.append((h, pos, lv, v2 is None or _get(v2, 7, True)))
        pos += _get(h, 3)
    return out


def codecs_of(path):
    """{leaf: the codec number of its first chunk}"""
    return {leaf: _get(md, 4) for _, _, md, leaf, _, _ in reversed(_chunks(open(path, "rb").read())[1])}


def lz4_pages(path, leaf):
    """[(offset, compressed length, uncompressed length, codec)] of the LZ4-compressed part of every
    page of `leaf` (all row groups)."""
    buf = open(path, "rb").read()
    out = []
    for _, _, md, name, start, end in _chunks(buf)[1]:
        if name != leaf:
            continue
        assert _get(md, 4) in (5, 7), _get(md, 4)
        for h, pos, lv, compressed in _pages(buf, start, end):
            if compressed:
                out.append((pos + lv, _get(h, 3) - lv, _get(h, 2) - lv, _get(md, 4)))
    return out


def is_literals_only(body, n_out, codec):
    """The page is a copy for the planner: every block is one literal run that fills its capacity."""
    if codec == 7:
        w = walk(body)
        return w is not None and len(w["seqs"]) == 1 and w["size"] == n_out and n_out > 0
    units, _ = units_of(body)
    return bool(units) and all(len(bl) == 1 and len(walk(body[p:p + c])["seqs"]) == 1 and walk(body[p:p + c])["size"] == U
                               for U, bl in units for p, c in bl)


def rewrite(path, out, bodies=None, chunk_codecs=None, body_of=None, stored=()):
    """Writes `out`: `path` with page bodies replaced. bodies: {(leaf, page index over all row groups):
    (codec, body)} for the compressed part of a page; chunk_codecs: {leaf: codec} for the footer;
    body_of(leaf, index, codec, body, uncompressed length) -> body or None, asked for every compressed
    page that `bodies` does not name. Page headers get the new compressed_page_size; the footer gets each
    chunk's codec, total_compressed_size, page offsets and file_offset, and each row group's
    total_compressed_size and file_offset. stored: leaves whose DATA_PAGE_V2 pages the writer left
    uncompressed (is_compressed false) count as compressed pages too; one that gets a body is marked
    compressed. The header must hold is_compressed, as pyarrow's do: one that leaves the field to its default
    raises KeyError here."""
    bodies, chunk_codecs = bodies or {}, chunk_codecs or {}
    buf = open(path, "rb").read()
    meta, chunks = _chunks(buf)
    new = bytearray(b"PAR1")
    seen = {}
    for rg in _get(meta, 4)[1]:
        rg_first, rg_total = None, 0
        for rg2, cc, md, leaf, start, end in chunks:
            if rg2 is not rg:
                continue
            codec = chunk_codecs.get(leaf, _get(md, 4))
            at0 = len(new)
            data_off = dict_off = None
            for h, pos, lv, compressed in _pages(buf, start, end):
                k = seen.get(leaf, 0)
                body = buf[pos:pos + _get(h, 3)]
                if compressed or (leaf in stored and _get(h, 8) is not None):
                    seen[leaf] = k + 1
                    repl = bodies.get((leaf, k))
                    if repl is None and body_of is not None:
                        b = body_of(leaf, k, _get(md, 4), body[lv:], _get(h, 2) - lv)
                        repl = None if b is None else (codec, b)
                    if repl is not None:
                        assert repl[0] == codec, "page %d of %s is codec %d in a chunk of codec %d" % (k, leaf, repl[0], codec)
                        body = body[:lv] + repl[1]
                        _set(h, 3, len(body))
                        if not compressed:
                            _set(_get(h, 8), 7, True)
                if _get(h, 1) == 2:
                    dict_off = len(new)
                elif data_off is None:
                    data_off = len(new)
                new += t_write(h) + body
            _set(md, 4, codec)
            _set(md, 7, len(new) - at0)
            _set(md, 9, data_off)
            if _get(md, 11) is not None:
                _set(md, 11, dict_off if dict_off is not None else 0)
            if _get(cc, 2) is not None:
                _set(cc, 2, _get(cc, 2) + at0 - start)
            rg_first = at0 if rg_first is None else rg_first
            rg_total += len(new) - at0
        if _get(rg, 5) is not None:
            _set(rg, 5, rg_first)
        if _get(rg, 6) is not None:
            _set(rg, 6, rg_total)
    foot = t_write(meta)
    new += foot + struct.pack("<I", len(foot)) + b"PAR1"
    open(out, "wb").write(bytes(new))


def to_hadoop(path, out, leaves=None, split=None):
    """A codec-7 file as codec 5: every page body of `leaves` (default: all) becomes one unit of one inner
    block -- the form Arrow reads -- or, with split(leaf, index, data) -> [[piece, ...], ...], the units
    and inner blocks of the pieces, each compressed on its own."""
    cod = codecs_of(path)
    leaves = [l for l in cod if cod[l] == 7] if leaves is None else leaves

    def body_of(leaf, k, codec, body, usize):
        if leaf not in leaves:
            return None
        if codec == 5:
            return None
        if usize == 0:
            return b""
        if split is None:
            return struct.pack(">II", usize, len(body)) + body
        data = reference(body, usize, BARE)
        return hadoop([[pyarrow_block(p) for p in unit] for unit in split(leaf, k, data)])
    rewrite(path, out, chunk_codecs={l: 5 for l in leaves}, body_of=body_of)
