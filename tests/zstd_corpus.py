"""Shared by the ZSTD page tests (host and GPU): payloads, frames written by pyarrow's libzstd (one-shot
at several levels, streaming with a flush), frames assembled by hand (every Frame_Content_Size width,
single-segment or a Window_Descriptor, a content checksum from a pure-Python XXH64, Raw / RLE / empty
blocks, compressed blocks whose three sequence tables are in RLE mode), skippable frames, a walker
that reports which features of the format a stream uses, the reference decoder (pyarrow's libzstd),
deterministic mutations, and the in-place replacement of a page body in a Parquet file."""
import struct

import numpy as np

from tests import delta_pages_corpus as C
from tests import inflate_corpus as I
from tests.inflate_corpus import records, text  # noqa: F401  (records: the stand-alone program's input)

MAGIC = 0xFD2FB528
M64 = (1 << 64) - 1


# ---- payloads ------------------------------------------------------------------------------------
def far_repeat():
    """300 KiB: a 150 KiB text twice, so the second half matches at a distance beyond one block."""
    half = text(150 * 1024, 11)
    return half + half


def int64_column(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 40, n, dtype=np.int64).tobytes()


def payloads(small=False):
    rng = np.random.default_rng(7)
    if small:
        return {"empty": b"", "one": b"x", "run": b"a" * 3000, "paths": "\n".join(C.config3_paths(40, 3)).encode(),
                "random": rng.integers(0, 256, 600, dtype=np.uint8).tobytes(), "text": text(2500, 5)}
    return {"empty": b"", "one": b"x", "run": b"\x07" * 300000, "paths": plain_paths(9000),
            "paths4k": plain_paths(9000)[:4096], "random": rng.integers(0, 256, 100 * 1024, dtype=np.uint8).tobytes(),
            "text": text(40000, 5), "int64": int64_column(20000, 3), "far": far_repeat()}


def plain_paths(n):
    """PLAIN-encoded BYTE_ARRAY values: <u32 length> <bytes> per config-3 path."""
    return b"".join(struct.pack("<I", len(p)) + p.encode() for p in C.config3_paths(n, 3))


# ---- frames by libzstd -----------------------------------------------------------------------------
def one_shot(data, level=3):
    import pyarrow as pa
    return pa.Codec("zstd", compression_level=level).compress(data, asbytes=True)


def streaming(data):
    """A frame written through a stream with a flush in the middle: a Window_Descriptor, no content size."""
    import pyarrow as pa
    sink = pa.BufferOutputStream()
    with pa.CompressedOutputStream(sink, "zstd") as z:
        z.write(data[:len(data) // 2])
        z.flush()
        z.write(data[len(data) // 2:])
    return sink.getvalue().to_pybytes()


# ---- frames by hand ----------------------------------------------------------------------------------
def xxh64(data, seed=0):
    P1, P2, P3, P4, P5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5
    rotl = lambda x, r: ((x << r) | (x >> (64 - r))) & M64
    rnd = lambda acc, v: (rotl((acc + v * P2) & M64, 31) * P1) & M64
    n, p = len(data), 0
    if n >= 32:
        v = [(seed + P1 + P2) & M64, (seed + P2) & M64, seed, (seed - P1) & M64]
        while p + 32 <= n:
            for k, w in enumerate(struct.unpack_from("<4Q", data, p)):
                v[k] = rnd(v[k], w)
            p += 32
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & M64
        for k in range(4):
            h = ((h ^ rnd(0, v[k])) * P1 + P4) & M64
    else:
        h = (seed + P5) & M64
    h = (h + n) & M64
    while p + 8 <= n:
        h = (rotl(h ^ rnd(0, struct.unpack_from("<Q", data, p)[0]), 27) * P1 + P4) & M64
        p += 8
    if p + 4 <= n:
        h = (rotl(h ^ (struct.unpack_from("<I", data, p)[0] * P1 & M64), 23) * P2 + P3) & M64
        p += 4
    while p < n:
        h = (rotl(h ^ (data[p] * P5 & M64), 11) * P1) & M64
        p += 1
    h ^= h >> 33
    h = h * P2 & M64
    h ^= h >> 29
    h = h * P3 & M64
    return h ^ (h >> 32)


def block(kind, body, size=None, last=False):
    """kind 0 Raw (body: the bytes), 1 RLE (body: one byte; size: the run), 2 Compressed, 3 reserved."""
    size = len(body) if size is None else size
    return struct.pack("<I", int(last) | kind << 1 | size << 3)[:3] + body


def raw_blocks(data, step=100000):
    """`data` as Raw blocks of at most `step` bytes, the last one marked so."""
    cuts = list(range(0, len(data), step)) or [0]
    return b"".join(block(0, data[c:c + step], last=c == cuts[-1]) for c in cuts)


def frame(blocks, content, fcs=None, single=None, checksum=False, window=0x50, dict_id=None, descriptor_or=0):
    """A frame around `blocks` (already encoded, the last one marked so). fcs: bytes of the
    Frame_Content_Size field (0, 1, 2, 4, 8; default: the smallest that holds it with single-segment).
    content: the frame's output (for the size field and the checksum)."""
    n = len(content)
    if fcs is None:
        fcs = 1 if n < 256 else 2 if n < 65536 + 256 else 4
    single = fcs == 1 if single is None else single
    assert fcs != 1 or single
    d = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs] << 6 | int(single) << 5 | int(checksum) << 2 | descriptor_or
    out = struct.pack("<IB", MAGIC, d | (0 if dict_id is None else 1))
    if not single:
        out += bytes([window])
    if dict_id is not None:
        out += bytes([dict_id])
    if fcs:
        out += struct.pack("<Q", n - 256 if fcs == 2 else n)[:fcs]
    out += blocks
    if checksum:
        out += struct.pack("<I", xxh64(content) & 0xffffffff)
    return out


def skippable(payload=b"", nibble=0):
    return struct.pack("<II", 0x184D2A50 | nibble, len(payload)) + payload


def rle_sequences(literals, seqs, rle_literals=False):
    """The body of a Compressed block: Raw literals and `seqs` = [(ll_code, of_code, of_extra, ml_code)]
    whose three tables are in RLE mode -- so every sequence of the block has the same codes, and the
    bitstream holds only the offsets' extra bits. Codes with extra bits of their own are not offered."""
    ll, of, _, ml = seqs[0]
    assert all(s[0] == ll and s[1] == of and s[3] == ml for s in seqs) and ll < 16 and ml < 32 and len(seqs) < 128
    n, kind = len(literals), int(rle_literals)   # RLE literals: `literals` is one byte, repeated
    assert not rle_literals or literals == literals[:1] * n
    head = bytes([kind | n << 3]) if n < 32 else struct.pack("<H", kind | 1 << 2 | n << 4) if n < 4096 else \
        struct.pack("<I", kind | 3 << 2 | n << 4)[:3]
    literals = literals[:1] if rle_literals else literals
    bits = nbits = 0
    for _, _, extra, _ in reversed(seqs):   # the first sequence's bits are read first: they lie highest
        bits |= extra << nbits
        nbits += of
    bits |= 1 << nbits                      # the final-bit marker
    return head + literals + bytes([len(seqs), 1 << 6 | 1 << 4 | 1 << 2, ll, of, ml]) + \
        bits.to_bytes(nbits // 8 + 1, "little")


def huffman_literals(symbols):
    """A block body without sequences whose literals are one Huffman stream over the two symbols 'a' and
    'b' (one bit each), the tree described by direct 4-bit weights."""
    assert set(symbols) <= set(b"ab") and len(symbols) < 1024
    nibbles = [0] * 98
    nibbles[97] = 1                                   # 'a': weight 1; 'b' is the implied last weight
    tree = bytes([127 + 98]) + bytes(nibbles[i] << 4 | nibbles[i + 1] for i in range(0, 98, 2))
    v = 1
    for c in symbols:
        v = v << 1 | (c == 98)
    stream = v.to_bytes(v.bit_length() // 8 + 1, "little").rstrip(b"\0")
    body = tree + stream
    return struct.pack("<I", 2 | len(symbols) << 4 | len(body) << 14)[:3] + body + b"\0"


def hand_frames(data):
    """{name: stream} assembled here; each decodes to `data`."""
    out = {}
    blocks = raw_blocks(data)
    for fcs in (0, 1, 2, 4, 8):
        if (fcs == 1 and len(data) > 255) or (fcs == 2 and not 256 <= len(data) < 65536 + 256):
            continue
        out["fcs%d" % fcs] = frame(blocks, data, fcs=fcs)
        if fcs not in (0, 1):
            out["fcs%d+single" % fcs] = frame(blocks, data, fcs=fcs, single=True)
    out["checksum"] = frame(blocks, data, checksum=True)
    out["checksum+window"] = frame(blocks, data, fcs=0, checksum=True)
    out["empty blocks"] = frame(_with_empties(data), data)
    out["final empty raw"] = frame(_not_last(raw_blocks(data)) + block(0, b"", last=True), data)
    if data and data == data[:1] * len(data):
        out["rle blocks"] = frame(b"".join(block(1, data[:1], min(1 << 20, len(data) - c), last=c + (1 << 20) >= len(data))
                                           for c in range(0, len(data), 1 << 20)), data, fcs=0)
    return out


def _not_last(blocks):
    """`blocks` (from raw_blocks) with the last-block bit of its final block cleared."""
    b, pos = bytearray(blocks), 0
    while True:
        h = int.from_bytes(b[pos:pos + 3], "little")
        if h & 1:
            b[pos] &= 0xfe
            return bytes(b)
        pos += 3 + (h >> 3)


def _with_empties(data):
    half = len(data) // 2
    return block(0, b"") + block(1, b"z", 0) + _not_last(raw_blocks(data[:half], 70000)) + block(0, b"") + \
        raw_blocks(data[half:], 70000)


def raw_rle_then_compressed(data, level=19):
    """One frame that opens with a Raw and an RLE block and continues with libzstd's compressed blocks
    of the rest (taken out of a streaming frame, whose blocks do not refer to anything before them
    except through offsets -- so the rest is compressed on its own and its blocks are spliced in)."""
    rest = one_shot(data[6:], level)
    f = walk(rest)[0][0]
    body = rest[f["first_block"]:f["end"] - (4 if f["checksum"] else 0)]
    return frame(block(0, data[:5]) + block(1, data[5:6], 1) + body, data, fcs=0, window=0xa0)


def variants(data):
    """{name: stream} of one payload; each decodes to `data`."""
    third = len(data) // 3
    out = {"l%d" % lv: one_shot(data, lv) for lv in (1, 3, 19)}
    out["stream"] = streaming(data)
    out["two"] = one_shot(data[:third], 19) + one_shot(data[third:], 1)
    out["three"] = one_shot(data[:third], 3) + streaming(data[third:2 * third]) + one_shot(data[2 * third:], 3)
    out["skips"] = skippable(b"abc") + one_shot(data[:third], 3) + skippable(b"", 5) + skippable(b"\0" * 20, 15) + \
        one_shot(data[third:], 3) + skippable(b"tail")
    for k, v in hand_frames(data).items():
        out["hand/" + k] = v
    return out


def crafted():
    """[(name, stream, data)]: features the writers above do not reach on these payloads."""
    out = []
    lit = b"abcdefgh"
    # one sequence: 4 literals, a match of 5 at offset 2 (offset code 2: value 4 + extra 1 = 5, minus 3)
    body = rle_sequences(lit, [(4, 2, 1, 2)])
    out.append(("crafted/rle tables", frame(block(2, body, last=True), b"abcdcdcdcefgh", fcs=0), b"abcdcdcdcefgh"))
    # repeat offsets: offset code 0 (the last offset) right after it, in a second block of the frame
    b2 = rle_sequences(b"XY", [(1, 0, 0, 1)])
    data = b"abcdcdcdcefgh" + b"X" + b"hXhX" + b"Y"
    out.append(("crafted/repeat offset across blocks", frame(block(2, body) + block(2, b2, last=True), data, fcs=0), data))
    body = rle_sequences(b"q" * 40, [(3, 2, 0, 4)] * 2, rle_literals=True)   # twice: 3 literals, 7 at offset 1
    out.append(("crafted/rle literals", frame(block(2, body, last=True), b"q" * 54, fcs=0, checksum=True), b"q" * 54))
    data = b"abbabaaabbbbab" * 9
    out.append(("crafted/direct weights", frame(block(2, huffman_literals(data), last=True), data, fcs=4), data))
    return out


def streams(small=False):
    """[(name, stream, expected output)]"""
    out = [("%s/%s" % (p, v), s, data) for p, data in payloads(small).items() for v, s in variants(data).items()]
    if not small:
        data = payloads()["paths"]
        out += [("paths/l9", one_shot(data, 9), data), ("paths/raw+rle+compressed", raw_rle_then_compressed(data), data)]
    return out + crafted()


# ---- the walker ------------------------------------------------------------------------------------
def walk(s):
    """([frame], features, header offsets) of a well-formed stream. A frame: {first_block, end, checksum,
    skippable}. features: a set of names such as "block:raw", "literals:treeless", "streams:4",
    "weights:fse", "mode:repeat". header offsets: the stream positions of frame headers, block headers,
    literals and sequences section headers and table descriptions (where a mutation changes a decision
    of the format, not a payload byte)."""
    frames, feats, heads, pos = [], set(), [], 0
    while pos < len(s):
        magic = struct.unpack_from("<I", s, pos)[0]
        if magic & 0xfffffff0 == 0x184D2A50:
            size = struct.unpack_from("<I", s, pos + 4)[0]
            heads += range(pos, pos + 8)
            frames.append({"skippable": True, "first_block": pos + 8, "end": pos + 8 + size, "checksum": False})
            feats.add("frame:skippable")
            pos += 8 + size
            continue
        assert magic == MAGIC
        d, at = s[pos + 4], pos + 5
        single, checksum = d >> 5 & 1, d >> 2 & 1
        at += (0 if single else 1) + (0, 1, 2, 4)[d & 3]
        fcs = (single, 2, 4, 8)[d >> 6]
        feats.add("fcs:%d" % fcs)
        feats.add("frame:single" if single else "frame:window")
        if checksum:
            feats.add("frame:checksum")
        at += fcs
        heads += range(pos, at)
        f = {"skippable": False, "first_block": at, "checksum": bool(checksum)}
        while True:
            h = int.from_bytes(s[at:at + 3], "little")
            heads += range(at, at + 3)
            last, kind, size = h & 1, h >> 1 & 3, h >> 3
            feats.add("block:" + ("raw", "rle", "compressed")[kind])
            if size == 0:
                feats.add("block:empty")
            at += 3
            if kind == 2:
                _walk_block(s, at, at + size, feats, heads)
            at += 1 if kind == 1 else size
            if last:
                break
        at += 4 if checksum else 0
        f["end"] = at
        frames.append(f)
        pos = at
    return frames, feats, heads


def _walk_block(s, pos, end, feats, heads):
    b0 = s[pos]
    kind, fmt = b0 & 3, b0 >> 2 & 3
    feats.add("literals:" + ("raw", "rle", "compressed", "treeless")[kind])
    if kind < 2:
        lh = (1, 2, 1, 3)[fmt]
        regen = int.from_bytes(s[pos:pos + lh], "little") >> (3 if lh == 1 else 4)
        csize = 1 if kind == 1 else regen
    else:
        lh = (3, 3, 4, 5)[fmt]
        v = int.from_bytes(s[pos:pos + lh], "little")
        bits = (10, 10, 14, 18)[fmt]
        csize = v >> (4 + bits) & ((1 << bits) - 1)
        feats.add("streams:%d" % (1 if fmt == 0 else 4))
        if kind == 2:
            feats.add("weights:direct" if s[pos + lh] >= 128 else "weights:fse")
            tree = (s[pos + lh] - 127 + 1) // 2 if s[pos + lh] >= 128 else s[pos + lh]
            heads += range(pos + lh, pos + lh + 1 + tree)
    heads += range(pos, pos + lh)
    at = pos + lh + csize
    n = s[at]
    heads.append(at)
    at += 1
    if n > 0x7f:
        heads.append(at)
        if n == 0xff:
            heads.append(at + 1)
            n = int.from_bytes(s[at:at + 2], "little") + 0x7f00
            at += 2
        else:
            n = (n - 0x80 << 8) + s[at]
            at += 1
    if n == 0:
        feats.add("sequences:none")
        return
    m = s[at]
    heads += range(at, min(at + 12, end))   # the modes byte and the start of the table descriptions
    for shift in (6, 4, 2):
        feats.add("mode:" + ("predefined", "rle", "fse", "repeat")[m >> shift & 3])


FEATURES = {"block:raw", "block:rle", "block:compressed", "block:empty", "literals:raw", "literals:rle",
            "literals:compressed", "literals:treeless", "streams:1", "streams:4", "weights:direct", "weights:fse",
            "mode:predefined", "mode:rle", "mode:fse", "mode:repeat", "frame:skippable", "frame:single", "frame:window",
            "frame:checksum", "fcs:0", "fcs:1", "fcs:2", "fcs:4", "fcs:8", "sequences:none"}


# ---- the reference ---------------------------------------------------------------------------------
def reference(stream, n_out):
    """What pyarrow's libzstd gives for `stream` when it must fill exactly n_out bytes, or None."""
    import pyarrow as pa
    try:
        return pa.Codec("zstd").decompress(stream, n_out, asbytes=True)
    except Exception:
        return None


def huffman_sections(s):
    """[{regen, streams, bounds}] of the Huffman-coded literals sections of a stream that need not be well
    formed (what can be read before the walk fails): bounds are the stream positions [s0, s1, s2, s3,
    end] of four streams, None for one stream or where they do not fit."""
    out, pos = [], 0
    try:
        while pos + 5 <= len(s):
            magic = struct.unpack_from("<I", s, pos)[0]
            if magic & 0xfffffff0 == 0x184D2A50:
                pos += 8 + struct.unpack_from("<I", s, pos + 4)[0]
                continue
            if magic != MAGIC:
                break
            d, at = s[pos + 4], pos + 5
            single = d >> 5 & 1
            at += (0 if single else 1) + (0, 1, 2, 4)[d & 3] + (single, 2, 4, 8)[d >> 6]
            while True:
                h = int.from_bytes(s[at:at + 3], "little")
                last, kind, size = h & 1, h >> 1 & 3, h >> 3
                at += 3
                if kind == 2 and s[at] & 3 >= 2:
                    fmt = s[at] >> 2 & 3
                    lh, bits = (3, 3, 4, 5)[fmt], (10, 10, 14, 18)[fmt]
                    v = int.from_bytes(s[at:at + lh], "little")
                    regen, csize = v >> 4 & ((1 << bits) - 1), v >> (4 + bits) & ((1 << bits) - 1)
                    body, bounds = at + lh, None
                    if s[at] & 3 == 2:
                        body += 1 + ((s[body] - 127 + 1) // 2 if s[body] >= 128 else s[body])
                    if fmt:
                        j = [body + 6]
                        for k in range(3):
                            j.append(j[-1] + int.from_bytes(s[body + 2 * k:body + 2 * k + 2], "little"))
                        j.append(at + lh + csize)
                        bounds = j if j[3] <= j[4] <= len(s) else None
                    out.append({"regen": regen, "streams": 4 if fmt else 1, "bounds": bounds})
                at += 1 if kind == 1 else size
                if kind == 3 or last:
                    break
            pos = at + (4 if d >> 2 & 1 else 0)
    except IndexError:
        pass
    return out


def loose_eligible(s):
    """Does `s` hold a literals section that libzstd's four-stream loop decodes (four streams of eight
    bytes or more each)? Structural: read off the section headers and the jump table."""
    return any(h["bounds"] and all(h["bounds"][k + 1] - h["bounds"][k] >= 8 for k in range(4)) for h in huffman_sections(s))


def two_symbol_eligible(s):
    """Does `s` hold a four-stream literals section of 768 regenerated bytes or more? Only for those may
    libzstd pick its two-symbol Huffman decoder (HUF_selectDecoder weighs a table-build time against a
    time per 256 output bytes; by its table the two-symbol decoder cannot win below three such units at
    any compression ratio), whose loop has refusal conditions of its own that zstd_fmt.h does not
    reproduce: the one tolerated class, capped at 2 % by the test that uses this."""
    return any(h["streams"] == 4 and h["regen"] >= 768 for h in huffman_sections(s))


def reference_is_loose():
    """Does the reference decode four Huffman streams with its loop that has no end check (libzstd
    1.5.5 or later on a CPU with BMI2)? Probed: the lowest bit of the first byte of a stream -- the
    last bit read -- is flipped, so the stream no longer ends exactly where its last symbol does."""
    data = text(2500, 5)
    s = one_shot(data, 3)
    h = next(h for h in huffman_sections(s) if h["bounds"])
    b = bytearray(s)
    b[h["bounds"][1]] ^= 1
    return reference(bytes(b), len(data)) is not None


def mutations(stream, count, seed):
    """`count` copies of `stream` with one bit flipped or one byte replaced: half of them in the frame,
    block and section headers (walk()'s header offsets), the others anywhere."""
    rng = np.random.default_rng(seed)
    n, heads = len(stream), walk(stream)[2]
    for k in range(count):
        at = heads[int(rng.integers(0, len(heads)))] if k % 2 == 0 else int(rng.integers(0, n))
        b = bytearray(stream)
        b[at] = b[at] ^ (1 << int(rng.integers(0, 8))) if k % 3 else int(rng.integers(0, 256))
        yield bytes(b)


# ---- page bodies of a Parquet file -----------------------------------------------------------------
def zstd_pages(path, leaf):
    """[(offset, compressed length, uncompressed length)] of the ZSTD-compressed part of every page of
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
            assert col.compression == "ZSTD"
            pos = col.dictionary_page_offset if col.has_dictionary_page else col.data_page_offset
            end = pos + col.total_compressed_size
            while pos < end:
                h, pos = I._page_header(buf, pos)
                lv = 0
                if h["type"] == 3:   # v2: the levels stay uncompressed, and so may the values (is_compressed)
                    lv = h["v2"].get(5, 0) + h["v2"].get(6, 0)
                if h["type"] != 3 or h["v2"].get(7, 1):
                    out.append((pos + lv, h["csize"] - lv, h["usize"] - lv))
                pos += h["csize"]
    return out


def pad_to(stream, size, front=True):
    """`stream` with one skippable frame in front of it (or behind) that brings it to `size` bytes."""
    gap = size - len(stream)
    assert gap == 0 or gap >= 8, "a gap of %d bytes cannot be filled (%d for %d)" % (gap, len(stream), size)
    pad = skippable(b"\0" * (gap - 8)) if gap else b""
    return pad + stream if front else stream + pad


def grow(stream, g):
    """`stream` made 1 to 7 bytes longer inside its first zstd frame, for gaps no whole frame fills: a
    Dictionary_ID field of 1, 2 or 4 bytes that holds 0 (no dictionary) and 3-byte empty Raw blocks in
    front of the frame's blocks."""
    did, blocks = {1: (1, 0), 2: (2, 0), 3: (0, 1), 4: (3, 0), 5: (2, 1), 6: (0, 2), 7: (3, 1)}[g]
    f = next(f for f in walk(stream)[0] if not f["skippable"])
    start = max(e["end"] for e in walk(stream)[0] if e["end"] <= f["first_block"]) if \
        any(e["end"] <= f["first_block"] for e in walk(stream)[0]) else 0
    d = stream[start + 4]
    assert d & 3 == 0, "the frame already has a Dictionary_ID field"
    at = start + 5 + (0 if d >> 5 & 1 else 1)           # behind the Window_Descriptor
    out = stream[:start + 4] + bytes([d | did]) + stream[start + 5:at] + b"\0" * (0, 1, 2, 4)[did] + \
        stream[at:f["first_block"]] + block(0, b"") * blocks + stream[f["first_block"]:]
    assert len(out) == len(stream) + g
    return out


def refit(stream, data, size):
    """A stream of exactly `size` bytes that decodes to `data`: `stream` behind a skippable frame that
    absorbs the difference; a gap of 1 to 7 bytes, which no frame fills, goes into the stream's first
    frame (grow). Asserts that it fits."""
    gap = size - len(stream)
    assert gap >= 0, "the replacement (%d bytes) does not fit the page's %d" % (len(stream), size)
    s = grow(stream, gap) if 0 < gap < 8 else pad_to(stream, size)
    assert len(s) == size and reference(s, len(data)) == data
    return s


def reheader(stream, data, fcs, single=False, checksum=False, window=0xa0):
    """libzstd's frame `stream` (one frame, which decodes to `data`) under a frame header built here."""
    f = walk(stream)[0]
    assert len(f) == 1 and not f[0]["checksum"]
    return frame(stream[f[0]["first_block"]:f[0]["end"]], data, fcs=fcs, single=single, checksum=checksum, window=window)


def replace_page(path, out, leaf, index, make):
    """Writes `out`: `path` with the ZSTD body of page `index` of `leaf` replaced by make(data, size) --
    a stream of exactly the body's length, so that every header and the footer stay valid."""
    buf = bytearray(open(path, "rb").read())
    at, csize, usize = zstd_pages(path, leaf)[index]
    data = reference(bytes(buf[at:at + csize]), usize)
    assert data is not None and len(data) == usize
    new = make(data, csize)
    assert len(new) == csize
    buf[at:at + csize] = new
    open(out, "wb").write(bytes(buf))
    return data
