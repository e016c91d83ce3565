"""Shared by the SNAPPY page tests (host and GPU): raw SNAPPY bodies built from explicit element lists
(every legal encoding of a length or an offset, not only the shortest), the inverse walk, a strict reference
decoder, a small greedy compressor whose choices the tests steer (copy tags, literal length bytes, preferred
offsets, copy lengths below 4, elements that ignore the writers' 64 KiB fragments), deterministic mutations
and the crafted streams. pyarrow's SNAPPY is the second oracle: every body built here decompresses to its
data there, and the reference judges every mutation as pyarrow does (tests/test_snappy_host.py).

The Parquet rewriter is tests/lz4_corpus's (codec-agnostic)."""
import numpy as np

from tests import delta_pages_corpus as C
from tests.inflate_corpus import text
from tests.lz4_corpus import _chunks, _get, _pages, codecs_of, records, rewrite  # noqa: F401 (re-exported)

FRAGMENT = 65536


# ---- elements --------------------------------------------------------------------------------------
def varint(n, size=None):
    """The preamble of n; `size` pads it to that many bytes (continuation bits on zero groups)."""
    out = bytearray()
    while True:
        out.append(n & 0x7f)
        n >>= 7
        if not n:
            break
    if size is not None:
        assert size >= len(out)
        out += b"\0" * (size - len(out))
    return bytes(b | 0x80 for b in out[:-1]) + out[-1:]


def min_nb(length):
    """The fewest length bytes a literal of `length` needs (0: the length sits in the tag)."""
    return 0 if length <= 60 else (length - 1).bit_length() + 7 >> 3


def encode_element(e):
    if e[0] == "lit":
        _, data, nb = e
        v = len(data) - 1
        assert 0 <= v < (60 if nb == 0 else 1 << 8 * nb) and 0 <= nb <= 4, (len(data), nb)
        return (bytes([v << 2]) if nb == 0 else bytes([(59 + nb) << 2]) + v.to_bytes(nb, "little")) + data
    _, off, n, kind = e
    if kind == 1:
        assert 4 <= n <= 11 and 0 <= off < 2048, e
        return bytes([1 | (n - 4) << 2 | (off >> 8) << 5, off & 0xff])
    assert 1 <= n <= 64 and kind in (2, 4) and 0 <= off < 1 << 8 * kind, e
    return bytes([(2 if kind == 2 else 3) | (n - 1) << 2]) + off.to_bytes(kind, "little")


def encode(elements, n_out=None, preamble=None):
    """A body from [("lit", bytes, nb) | ("copy", offset, length, kind)]: the varint preamble of what the
    elements decode to (or of n_out), in `preamble` bytes when given, and the elements."""
    if n_out is None:
        n_out = sum(len(e[1]) if e[0] == "lit" else e[2] for e in elements)
    return varint(n_out, preamble) + b"".join(encode_element(e) for e in elements)


def decode_elements(elements):
    """What the elements stand for."""
    out = bytearray()
    for e in elements:
        if e[0] == "lit":
            out += e[1]
        else:
            _, off, n, _ = e
            assert 0 < off <= len(out), e
            if off >= n:
                out += out[len(out) - off:len(out) - off + n]
            else:
                for _ in range(n):
                    out.append(out[-off])
    return bytes(out)


def preamble_of(body):
    """(value, bytes) of the varint, or None: truncated, longer than 5 bytes, or more than 32 bits."""
    v = 0
    for k in range(5):
        if k >= len(body):
            return None
        v |= (body[k] & 0x7f) << 7 * k
        if not body[k] & 0x80:
            return (v, k + 1) if v < 1 << 32 else None
    return None


def layout(body):
    """[(position behind the preamble, header bytes, element)] as far as the elements parse, and whether the
    walk reached the body's end exactly. A literal cut off by the end of the input is not part of the list."""
    pre = preamble_of(body)
    assert pre is not None
    s = body[pre[1]:]
    n, ip, out = len(s), 0, []
    while ip < n:
        tag = s[ip]
        t, l6 = tag & 3, tag >> 2
        if t == 0:
            nb = l6 - 59 if l6 >= 60 else 0
            if ip + 1 + nb > n:
                return out, False
            ln = (int.from_bytes(s[ip + 1:ip + 1 + nb], "little") if nb else l6) + 1
            if ip + 1 + nb + ln > n:
                return out, False
            out.append((ip, 1 + nb, ("lit", s[ip + 1 + nb:ip + 1 + nb + ln], nb)))
            ip += 1 + nb + ln
            continue
        hdr = (0, 2, 3, 5)[t]
        if ip + hdr > n:
            return out, False
        if t == 1:
            e = ("copy", (tag >> 5) << 8 | s[ip + 1], (l6 & 7) + 4, 1)
        else:
            e = ("copy", int.from_bytes(s[ip + 1:ip + hdr], "little"), l6 + 1, 2 if t == 2 else 4)
        out.append((ip, hdr, e))
        ip += hdr
    return out, True


def elements_of(body):
    """The inverse of encode(): the body's elements, or None when they do not parse to its end."""
    lay, whole = layout(body)
    return [e for _, _, e in lay] if whole else None


def wrapping_literal(body):
    """The structural predicate of the one form libsnappy takes and the format does not: the element at which
    the walk stops is a literal whose 4-byte length field holds 0xffffffff -- 2^32 bytes, 0 in 32 bits."""
    lay, whole = layout(body)
    stop = 0                                   # where the walk stops, behind the preamble
    if lay:
        ip, hdr, e = lay[-1]
        stop = ip + hdr + (len(e[1]) if e[0] == "lit" else 0)
    at = preamble_of(body)[1] + stop
    return not whole and body[at:at + 5] == b"\xfc\xff\xff\xff\xff"


def reference(body, n_out):
    """The strict decoder: the n_out bytes of the body, or None for anything the format forbids -- a preamble
    that is not n_out, is truncated, longer than 5 bytes or wider than 32 bits; a truncated element header; a
    literal running past the input (a literal length of 2^32 among them); offset 0; an offset reaching
    before the start of the output; more or fewer than n_out bytes."""
    pre = preamble_of(body)
    if pre is None or pre[0] != n_out:
        return None
    lay, whole = layout(body)
    if not whole:
        return None
    out = bytearray()
    for _, _, e in lay:
        if e[0] == "lit":
            out += e[1]
        else:
            _, off, n, _ = e
            if off == 0 or off > len(out):
                return None
            if off >= n:
                out += out[len(out) - off:len(out) - off + n]
            else:
                for _ in range(n):
                    out.append(out[-off])
        if len(out) > n_out:
            return None
    return bytes(out) if len(out) == n_out else None


def pyarrow_decode(body, n_out):
    """The second oracle: pyarrow's (libsnappy's) verdict and bytes for a body that must give n_out bytes."""
    import pyarrow as pa
    pre = preamble_of(body)
    try:
        got = pa.decompress(body, decompressed_size=n_out, codec="snappy", asbytes=True)
    except Exception:
        return None
    # libsnappy accepted the stream and produced what its preamble says; the caller's n_out is the contract
    return got if pre is not None and pre[0] == n_out and len(got) == n_out else None


# ---- the steered compressor --------------------------------------------------------------------------
def _copy_kind(off, n, kinds):
    for k in kinds:
        if k == 1 and 4 <= n <= 11 and off < 2048:
            return 1
        if k == 2 and off < 65536:
            return 2
        if k == 4:
            return 4
    raise AssertionError("no tag of %r holds offset %d, length %d" % (kinds, off, n))


def literal(data, nb=None):
    """The literal elements of `data`: one element, in `nb` length bytes (the fewest that do when None or too
    few); nb = 0 cuts the data into literals of at most 60 bytes."""
    if not data:
        return []
    if nb == 0:
        return [("lit", data[k:k + 60], 0) for k in range(0, len(data), 60)]
    return [("lit", data, max(min_nb(len(data)), nb or 0))]


def compress(data, fragment=FRAGMENT, kinds=(1, 2), lit_nb=None, offsets=(), max_copy=64, min_copy=4, min_lit=0,
             key=None):
    """A greedy compressor: the elements of `data`. At every position it tries the distances of `offsets`
    first, then the most recent earlier occurrence of the next `key` bytes (default: min(4, min_copy)). A
    match of at least min_copy bytes becomes copies of at most max_copy, each in the first tag of `kinds`
    that holds it; the bytes between matches become one literal in lit_nb length bytes (see literal()), and a
    match is only taken when the literal before it is empty or at least min_lit long. With `fragment` the
    data is compressed in pieces of that size, as the writers do: no element straddles a piece's end and no
    copy reaches before its piece. fragment=None drops both rules."""
    key = key or max(1, min(4, min_copy))
    n, out = len(data), []
    step = fragment or max(n, 1)
    for f0 in range(0, max(n, 1), step):
        f1 = min(n, f0 + step)
        table, i, anchor = {}, f0, f0
        while i < f1:
            k4 = data[i:i + key]
            cand = [i - d for d in offsets if 0 < d <= i - f0]
            c = table.get(k4)
            if c is not None:
                cand.append(c)
            table[k4] = i
            best = 0
            if i == anchor or i - anchor >= min_lit:
                for c in cand:
                    ml = 0
                    while i + ml < f1 and data[c + ml] == data[i + ml]:
                        ml += 1
                    if ml >= min_copy and (i - c < 65536 or 4 in kinds):
                        best, at = ml, c
                        break
            if not best:
                i += 1
                continue
            out += literal(data[anchor:i], lit_nb)
            left, off = best, i - at
            while left >= min_copy:
                m = min(left, max_copy)
                if 0 < left - m < min_copy and m - (min_copy - (left - m)) >= min_copy:
                    m -= min_copy - (left - m)
                out.append(("copy", off, m, _copy_kind(off, m, kinds)))
                i += m
                left -= m
            anchor = i
        out += literal(data[anchor:f1], lit_nb)
    assert decode_elements(out) == data
    return out


def spans(elements):
    """[(output position, output length, element)]"""
    out, op = [], 0
    for e in elements:
        n = len(e[1]) if e[0] == "lit" else e[2]
        out.append((op, n, e))
        op += n
    return out


def keeps_fragments(elements):
    """The writers' rules: no element straddles a 64 KiB boundary of the output, no copy reaches before the
    fragment it lies in."""
    return all(op // FRAGMENT == (op + n - 1) // FRAGMENT and (e[0] == "lit" or e[1] <= op % FRAGMENT)
               for op, n, e in spans(elements))


# ---- Parquet -----------------------------------------------------------------------------------------
def snappy_pages(path, leaf):
    """[(offset, compressed length, uncompressed length)] of the SNAPPY-compressed part of every page of
    `leaf` (all row groups)."""
    buf = open(path, "rb").read()
    out = []
    for _, _, md, name, start, end in _chunks(buf)[1]:
        if name != leaf:
            continue
        assert _get(md, 4) == 1, _get(md, 4)
        for h, pos, lv, compressed in _pages(buf, start, end):
            if compressed:
                out.append((pos + lv, _get(h, 3) - lv, _get(h, 2) - lv))
    return out


# ---- the corpus ----------------------------------------------------------------------------------------
def payloads():
    rng = np.random.default_rng(11)
    out = {"text": text(20000, 5), "paths": "\n".join(C.config3_paths(1500, 3)).encode(),
           "runs": b"ab" * 500 + b"xyz" * 400 + b"q" * 300 + text(100, 1), "run": b"\x07" * 70000,
           "random": rng.integers(0, 256, 5000, dtype=np.uint8).tobytes(),
           "three fragments": "\n".join(C.config3_paths(1800, 4)).encode()[:150000]}
    for k in range(1, 6):
        out["tiny%d" % k] = text(k, k)
    return out


def pyarrow_body(data):
    import pyarrow as pa
    return pa.compress(data, codec="snappy", asbytes=True)


def _far():
    """140,000 bytes whose second and third 64 KiB repeat the first with a few bytes changed, so that copies
    at offset 65536 and beyond exist."""
    a = bytearray(text(FRAGMENT, 21))
    b = bytearray(a)
    b[1000:1004] = b"####"
    c = bytearray(a)
    c[3000:3003] = b"@@@"
    return bytes(a + b + c)[:140000]


def crafted():
    """{name: (body, expected output)}: what one compressor never writes. test_snappy_host asserts on
    elements_of() that each holds what it is named for."""
    p = payloads()
    paths, runs, txt = p["paths"][:30000], p["runs"], p["text"]
    out = {}

    def add(name, elements, **kw):
        out[name] = (encode(elements, **kw), decode_elements(elements))
    add("every copy tag 3", compress(paths, kinds=(4,)))
    add("every copy tag 2", compress(paths, kinds=(2,)))
    for nb in (1, 2, 3, 4):
        add("literals in %d length bytes" % nb, compress(paths, lit_nb=nb))
    add("literals of one byte in 4 length bytes", compress(runs, lit_nb=4, min_copy=1, kinds=(2,), max_copy=3, key=2))
    for n in (60, 61, 64, 65, 256, 257, 65536):
        d = text(n, n)
        add("literal of %d" % n, literal(d[:30], 0) + [("copy", 7, 9, 1)] + literal(d) + [("copy", n, 12, 2 if n < 65536 else 4)])
    for n in (1, 2, 3, 64):
        add("copies of %d" % n, compress(runs, kinds=(2,), min_copy=n, max_copy=n, offsets=(1, 2, 3)))
    for off in (1, 2, 3):
        add("offset %d length 64" % off, compress(runs, kinds=(2, 4), offsets=(off,), key=4))
    big = text(FRAGMENT, 3)
    add("offset 65535", literal(big[:65535]) + [("copy", 65535, 1, 2)])
    add("offset equal to the position in the fragment", literal(big[:40000]) + [("copy", 40000, 64, 2), ("copy", 40064, 64, 4)])
    add("copy reaching before its fragment", compress(_far(), fragment=None, kinds=(1, 2, 4)))
    add("copy straddling a fragment end", literal(big[:65530]) + [("copy", 65530, 20, 2)] + literal(b"tail"))
    add("literal straddling a fragment end", literal(big[:100], 0) + [("copy", 50, 30, 2)] + literal(big[130:] + b"over the end"))
    add("tag 3 offset of 65536 and more", literal(big) + literal(b"abcd") + [("copy", 65536, 40, 4), ("copy", 65540, 4, 4)])
    add("two blocks of 65537 bytes", literal(big[:65533]) + [("copy", 3, 4, 2)])
    for n in (1, 2, 3, 4, 5):
        add("page of %d" % n, literal(text(n, 40 + n)))
        add("page of %d in a 3-byte preamble" % n, literal(text(n, 40 + n)), preamble=3)
    add("5-byte preamble", compress(txt[:500]), preamble=5)
    add("copies only after one byte", literal(b"z") + [("copy", 1, 64, 2)] * 50 + [("copy", 1, 1, 4)] * 50)
    return out


def corpus():
    """[(name, body, expected output)]"""
    out = [("pyarrow/" + name, pyarrow_body(data), data) for name, data in payloads().items()]
    out += [("crafted/" + name, body, data) for name, (body, data) in crafted().items()]
    return out


def header_positions(body):
    pre = preamble_of(body)[1]
    return list(range(pre)) + [pre + ip + k for ip, hdr, _ in layout(body)[0] for k in range(hdr)]


def mutations(stream, count, seed):
    """`count` copies of `stream`, each changed in one place: a bit flipped or a byte set (half of them in
    the preamble and the element headers, the others anywhere), and every fourth one cut short, or with a
    byte inserted or deleted."""
    rng = np.random.default_rng(seed)
    n = len(stream)
    heads = header_positions(stream)
    for k in range(count):
        at = heads[int(rng.integers(0, len(heads)))] if k % 2 == 0 else int(rng.integers(0, n))
        b = bytearray(stream)
        if k % 4 == 3:
            how = (k // 4) % 3
            if how == 0:
                b = b[:int(rng.integers(0, n))] if (k // 12) % 2 else b[:n - 1 - int(rng.integers(0, min(n, 6)))]
            elif how == 1:
                b.insert(at, int(rng.integers(0, 256)))
            else:
                del b[at]
        elif k % 3:
            b[at] ^= 1 << int(rng.integers(0, 8))
        else:
            b[at] = int(rng.integers(0, 256))
        yield bytes(b)
