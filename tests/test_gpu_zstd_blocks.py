"""Steered ZSTD blocks through k_zstd: every literals form, table mode and repeat offset of RFC 8878, and
the kernel's own machinery (the batch of ZS_BATCH sequences, the literal slab, the `drained` position, the
lock step of four Huffman streams next to the per-lane path), each on a body whose form is asserted with
zstd_steer.sequences() on the bytes that are sent -- not assumed.

The table is one (config 3 at scale 0.001, seed 3) whose add.stats is steered: the first add.stats page --
the only one, 572,250 bytes of PLAIN values in a DATA_PAGE_V2, so that the levels stay outside the body -- holds
a marker row that the last row repeats (a match over nearly the whole page: the largest offset code the page
allows, reaching the frame's first byte), a run of 65,6xx 'Z', runs of period 1, 2, 3, 63, 64 and 65, a row
written by a list of sequences with known repeat offsets, rows that differ only in a number, and a stretch of
68,921 bytes without a repeated three-byte string (a de Bruijn sequence: one literal run) right in front
of a second 'Z' run more than 256 KiB behind the first. A body is put in with lz4_corpus.rewrite, so its
length is free; the bytes around the steered frames go into frames libzstd writes. The SNAPPY twin of the
same table is the expectation: export(0), export(1) and the state against the oracle.

A form maps to a body and a predicate over what sequences() reads from it; bodies are shared, and each is
replayed once. Measured on an MI355X: the file's 49 cases take 11.6 s, 3.4 s of it
the module's tables; the slowest case (count 0x7F00) 0.75 s."""
import os
import re
import shutil

import numpy as np
import pytest

from oracle import delta_oracle as O
from tests import lz4_corpus as L
from tests import zstd_corpus as Z
from tests import zstd_steer as T
from tests.test_gpu_parity import _assert_same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kernel_constant(name):
    src = open(os.path.join(ROOT, "delta_amd", "csrc", "k_zstd.hip")).read()
    return re.search(r"constexpr uint32_t %s = ([^;]+);" % name, src).group(1)


ZS_BATCH = int(_kernel_constant("ZS_BATCH"))
SLAB = 128 * 1024
PERIODS = (1, 2, 3, 63, 64, 65)
LOWER = "abcdefghijklmnopqrstuvwxyz0123456789"
UPPER = "ABCDEFGHIJKLMNOPQRSTUVWXY!#$%&'()*+-./;<=>?@[]^_|~"[:41]   # no 'Z', nothing JSON escapes
FILL = '{"numRecords":%07d,"tags":"f"}'
W = len(FILL % 0) + 4             # a filler value with its length prefix
DIGITS = 4 + 14 + 4               # where the last three digits of a filler value start
FAR_ROW = 4004                    # the valid row that holds the stretch and the second 'Z' run


# ---- the steered table -------------------------------------------------------------------------------
def _random(n, seed, alphabet=LOWER):
    rng = np.random.default_rng(seed)
    return "".join(alphabet[k] for k in rng.integers(0, len(alphabet), n))


def _de_bruijn(k, n):
    """The de Bruijn sequence B(k, n) as symbol indices: every n-gram at most once in its linear form."""
    a, out = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                out.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return out


STRETCH = "".join(UPPER[i] for i in _de_bruijn(len(UPPER), 3))
MARKER = '{"numRecords":0,"tags":"%s"}' % _random(300, 1)


def _low_bytes_ascii(head, run, tail):
    """head + run + tail with `run` (one byte repeated) grown until the two low bytes of the value's length
    are below 128: a value's length prefix then stays inside what direct Huffman weights can name."""
    while (len(head + run + tail) & 0xff) >= 128 or (len(head + run + tail) >> 8 & 0xff) >= 128:
        run += run[:1]
    return head + run + tail


def _period_runs():
    """[(period, the run)]: each longer than 130 bytes, and for the periods above 1 not a whole number of
    periods long."""
    out = []
    for p in PERIODS:
        pat = {1: "q", 2: "ab", 3: "xyz"}.get(p) or _random(p, 100 + p)
        n = 140 if p == 1 else 141 if p == 2 else 151 if p == 3 else 3 * p + 7
        out.append((p, (pat * (n // p + 1))[:n]))
    return out


def _written(plan, seed):
    """The blocks of zstd_steer.run for a plan whose sequences are (ll, ml, distance, Offset_Value to send):
    literals are random, so a wrong offset gives other bytes. A plan entry: ("raw", n) or ("seq", [sequences],
    literals behind the last one)."""
    rng, blocks, out = np.random.default_rng(seed), [], bytearray()
    fresh = lambda n: bytes(ord(LOWER[k]) for k in rng.integers(0, len(LOWER), n))
    for entry in plan:
        if entry[0] == "raw":
            blocks.append(("raw", fresh(entry[1])))
            out += blocks[-1][1]
            continue
        lits, seqs = bytearray(), []
        for ll, ml, d, value in entry[1]:
            piece = fresh(ll)
            lits += piece
            out += piece
            for _ in range(ml):
                out.append(out[-d])
            seqs.append((ll, ml, d if value > 3 else -value))
        tail = fresh(entry[2])
        out += tail
        blocks.append(("seq", bytes(lits + tail), seqs, {}))
    assert T.run(blocks) == bytes(out)
    return blocks


FAR = 99   # "send the distance itself"
# one frame: three real offsets, then every repeat code with ll > 0 and ll == 0, each followed by Offset_Value 1
# with ll > 0 (the most recent offset), which shows how the three were rotated; a Raw block; the offsets again
REP_PLAN = [("seq", [(120, 10, 100, FAR), (5, 9, 77, FAR), (4, 8, 50, FAR),       # rep = 50, 77, 100
                     (3, 6, 50, 1), (2, 5, 50, 1),                                 # code 0, ll > 0: rep[0]
                     (0, 7, 77, 1), (2, 5, 77, 1),                                 # code 0, ll == 0: rep[1]; 77, 50, 100
                     (2, 6, 50, 2), (1, 5, 50, 1),                                 # code 1 bit 0, ll > 0: rep[1]; 50, 77, 100
                     (2, 6, 100, 3), (1, 5, 100, 1),                               # code 1 bit 1, ll > 0: rep[2]; 100, 50, 77
                     (0, 6, 77, 2), (1, 5, 77, 1),                                 # code 1 bit 0, ll == 0: rep[2]; 77, 100, 50
                     (0, 6, 76, 3), (1, 5, 76, 1)], 7),                            # code 1 bit 1, ll == 0: rep[0] - 1; 76, 77, 100
            ("raw", 40),
            ("seq", [(3, 6, 76, 1), (2, 5, 77, 2), (2, 5, 100, 3), (1, 4, 100, 1)], 5)]
# three more frames: behind a Raw block the first sequence takes Offset_Value 1, 2 or 3 of a fresh frame
START_PLANS = [[("raw", 20), ("seq", [(2, 6, d, v), (1, 4, d, 1)], 3)] for v, d in ((1, 1), (2, 4), (3, 8))]


def _written_rows():
    frames = [_written(REP_PLAN, 7)] + [_written(p, 8 + k) for k, p in enumerate(START_PLANS)]
    return frames, "".join(T.run(f).decode() for f in frames)


def _rows(n, shown):
    """{valid add row: its add.stats} of this file's table."""
    assert n > FAR_ROW + 1000
    return {0: MARKER, n - 1: MARKER,
            1: _low_bytes_ascii('{"tags":"', "Z" * 65616, '"}'),
            2: '{"tags":"%s"}' % "".join(_random(6, 50 + p) + run for p, run in _period_runs()),
            3: '{"tags":"%s"}' % _written_rows()[1],
            FAR_ROW: _low_bytes_ascii('{"tags":"' + STRETCH, "Z" * 65616, '"}')}


def _steered_table(table, rows_of, shown):
    """The table with add.stats steered: rows_of(number of valid add rows, shown) -> {row: value}; the other rows are
    fillers. shown[i]: the live state takes valid row i's stats from the checkpoint."""
    import pyarrow as pa
    col = table.schema.get_field_index("add")
    add = table.column(col).combine_chunks()
    valid = add.is_valid().to_pylist()
    n = sum(valid)
    rows = rows_of(n, shown)
    it = iter(range(n))
    stats = pa.array([(lambda i: rows.get(i, FILL % i))(next(it)) if v else None for v in valid], pa.string())
    k = add.type.get_field_index("stats")
    children = [stats if j == k else add.field(j) for j in range(add.type.num_fields)]
    new = pa.StructArray.from_arrays(children, fields=list(add.type), mask=pa.array([not v for v in valid]))
    return table.set_column(col, table.schema.field(col), new)


class Page:
    """The first add.stats page's bytes and where the steered rows lie in them."""

    def __init__(self, data):
        self.D = D = data
        self.z1 = D.index(b"Z" * 65616)
        self.periods = {p: D.index(run.encode()) for p, run in _period_runs()}
        self.frames, text = _written_rows()
        self.written = D.index(text.encode())
        self.fill = D.index((FILL % 4).encode()) - 4            # the first filler value (row 4)
        self.stretch = D.index(STRETCH.encode())
        self.z2 = self.stretch + len(STRETCH)
        self.z2_end = self.z2 + len(D[self.z2:]) - len(D[self.z2:].lstrip(b"Z"))
        self.far_row = self.stretch - 9 - 4
        self.last = len(D) - len(MARKER) - 4
        self.after = D.index((FILL % (FAR_ROW + 1)).encode()) - 4
        assert D[:len(MARKER) + 4] == D[self.last:] and D[self.far_row + 4:self.stretch] == b'{"tags":"'
        assert all(b < 128 for b in D[self.fill:])

    def row(self, r):
        """Where filler value r starts."""
        at = self.fill + (r - 4) * W if r < FAR_ROW else self.after + (r - FAR_ROW - 1) * W
        assert self.D[at + 4:at + W] == (FILL % r).encode()
        return at

    def around(self, a, steered):
        """The page with the bytes from D[a] on that the `steered` frames stand for sent as those frames, and the
        rest as libzstd's frames."""
        content = b"".join(c for _, c in steered)
        b = a + len(content)
        assert self.D[a:b] == content, "the steered frames do not stand for the page's bytes"
        body = (Z.one_shot(self.D[:a], 1) if a else b"") + b"".join(f for f, _ in steered) + \
            (Z.one_shot(self.D[b:], 1) if b < len(self.D) else b"")
        assert Z.reference(body, len(self.D)) == self.D, "libzstd refuses the steered body"
        return body


# ---- the bodies ----------------------------------------------------------------------------------------
def _rows_block(P, r0, n, first=None):
    """n sequences over filler values from r0 on, starting at r0's last three digits: three literal digits,
    then a match of W - 3 at distance W -- the previous sequence's match, byte for byte. first: another
    distance for the first one."""
    at = P.row(r0) + DIGITS
    lits = b"".join(P.D[at + k * W:at + k * W + 3] for k in range(n))
    return ("seq", lits, [(3, W - 3, first if first and k == 0 else W) for k in range(n)], {})


def body_literals(P):
    """Raw and RLE literals with and without sequences; their size formats; leftover literals; a match that reads an
    RLE block's output."""
    D, r = P.D, P.row(1100)
    e = P.row(1121) + DIGITS
    raw = T.encode_frame([("raw", D[r:P.row(1101) + DIGITS]), ("raw", b""), _rows_block(P, 1101, 20),
                          ("seq", D[e:e + 300], [], {}), ("seq", D[e + 300:e + 321], [], {}),   # an odd size: reads as format 2
                          ("seq", D[e + 321:e + 331], [], {}), ("seq", D[e + 331:e + 360], [], {"size_format": 3})],
                         fcs=2, single=True)
    rle = T.encode_frame([("rle", b"Z", 1000),
                          ("seq", b"Z" * 40, [(3, 200, 500), (3, 7, 1)], {"lit": "rle"}),
                          ("seq", b"Z" * 50, [], {"lit": "rle", "size_format": 1}), ("seq", b"Z" * 20, [], {"lit": "rle"}),
                          ("seq", b"Z" * 5000, [(4999, 300, 1)], {"lit": "rle"})], checksum=True)
    return _two(P, P.z1 + 10, rle, r, raw)


def _two(P, a, fa, b, fb):
    """The page with two steered regions (a < b), libzstd's frames around and between them, and a skippable frame."""
    D = P.D
    ea, eb = a + len(fa[1]), b + len(fb[1])
    assert a < ea <= b < eb and D[a:ea] == fa[1] and D[b:eb] == fb[1]
    body = Z.one_shot(D[:a], 1) + fa[0] + Z.skippable(b"between") + Z.one_shot(D[ea:b], 19) + fb[0] + Z.one_shot(D[eb:], 1)
    assert Z.reference(body, len(D)) == D, "libzstd refuses the steered body"
    return body


def body_huffman(P):
    """Compressed literals on 1 stream, on 4 streams in lock step and not (a stream under 8 bytes; regen 6);
    Treeless right after a Compressed block, and after a Raw-literals block and a Raw block; direct weights;
    every size format; regen below 32, below 4096 and at least 4096."""
    a = at = P.row(1200)
    w = T.huffman_weights(P.D[a:P.row(1800)])

    def take(n, **o):
        nonlocal at
        piece = P.D[at:at + n]
        at += n
        return piece, o
    tree = dict(lit="compressed", weights=w)
    plan = [take(25 * W, streams=1, **tree), take(25 * W, lit="treeless", streams=4), take(25 * W, streams=4, **tree),
            take(W + 9, streams=4, **tree), take(6, streams=4, **tree), take(400 * W, streams=4, size_format=2, **tree),
            take(20 * W, lit="treeless", streams=1), take(3 * W, lit="raw"), take(2 * W), take(25 * W, lit="treeless", streams=4,
                                                                                                size_format=3)]
    spec = []
    for piece, o in plan:
        if not o:
            spec.append(("raw", piece))
        elif len(piece) == 6:
            spec.append(("seq", piece, [], o))
        else:
            (lits, seqs), = T.parse(piece, max_ml=4 if len(piece) > 100 * W else 6, min_ll=8 if len(piece) > 100 * W else 3)
            spec.append(("seq", lits, seqs, o))
    return P.around(a, [T.encode_frame(spec, fcs=4)])


def body_slab(P):
    """131,072 literals under the 5-byte header: the slab filled to its last byte, in a block without sequences."""
    a = P.stretch + 100
    lits = P.D[a:a + SLAB]
    return P.around(a, [T.encode_frame([("seq", lits, [], dict(lit="compressed", streams=4))], fcs=8, single=True)])


def body_spliced(P):
    """FSE-described weights: libzstd's own tree description for the literals of its first block, under streams
    written here."""
    a = P.stretch - 80 * W
    for n in (8000, 20000, 5000):
        for level in (3, 19, 1):
            p = T.sequences(Z.one_shot(P.D[a:a + n], level))
            blocks = p.frames[0]["blocks"]
            b = blocks[0]
            if len(blocks) == 1 and b["type"] == "compressed" and b["literals"]["weights"] == "fse" and b["seqs"]:
                lits, at = bytearray(), 0   # the literals: the output with every match taken out
                for ll, ml, _, _, _, _ in b["seqs"]:
                    lits += p.data[at:at + ll]
                    at += ll + ml
                seqs = [(ll, ml, d) for ll, ml, d, _, _, _ in b["seqs"]]
                spec = [("seq", bytes(lits + p.data[at:]), seqs, dict(
                    lit="compressed", streams=4, tree=b["literals"]["tree"], ll=T.fitted(seqs, 0, 9), of=T.fitted(seqs, 1, 8),
                    ml=T.fitted(seqs, 2, 9)))]
                return P.around(a, [T.encode_frame(spec, fcs=2, single=True)])
    raise AssertionError("libzstd describes no tree with FSE for these literals")


def body_tables(P):
    """Each of the four modes on each of the three tables; Repeat after Predefined, after RLE and after
    FSE_Compressed, across a Raw block and across a block without sequences; accuracy logs 5 and 9/8/9; a "less
    than 1" symbol and a zero run in a table description."""
    a = P.row(2100)
    rows = lambda r, n, **o: _rows_block(P, r, n)[:3] + (o,)
    mixed = T.parse(P.D[P.row(2161) + DIGITS:P.row(2190) + DIGITS], max_ml=9, cut_every=30, use_repeats=False)[0]
    assert len(mixed[1]) == 30
    rest = P.D[P.row(2161) + DIGITS + len(T.run([("seq",) + mixed])):P.row(2190) + DIGITS]
    allrep = dict(ll=T.REPEAT, of=T.REPEAT, ml=T.REPEAT)
    low = {t: T.fitted(mixed[1], t, 5, pad=(3,) if t == 0 else ()) for t in range(3)}
    spec = [("raw", P.D[a:P.row(2101) + DIGITS]),
            rows(2101, 10), rows(2111, 10, **allrep),                                      # Predefined, Repeat
            rows(2121, 10, ll=T.RLE, of=T.RLE, ml=T.RLE), rows(2131, 10, **allrep),          # RLE, Repeat
            ("raw", P.D[P.row(2141) + DIGITS:P.row(2151) + DIGITS]), rows(2151, 5, **allrep),     # across a Raw block
            ("seq", P.D[P.row(2156) + DIGITS:P.row(2158) + DIGITS], [], {}), rows(2158, 3, **allrep),   # across no sequences
            ("seq",) + mixed + (dict(ll=low[0], of=low[1], ml=low[2]),),
            ("seq", rest, [], {}),
            rows(2190, 10, ll=T.REPEAT, of=T.PREDEFINED, ml=T.RLE),
            rows(2200, 10, ll=T.PREDEFINED, of=T.RLE, ml=T.REPEAT),
            rows(2210, 10, ll=T.RLE, of=T.REPEAT, ml=T.PREDEFINED)]
    # a "less than 1" symbol that no sequence uses, and zero runs of three or more between the codes in use
    again = T.parse(P.D[P.row(2220) + DIGITS:P.row(2250) + DIGITS], max_ml=9, cut_every=30, use_repeats=False)
    every = [q for _, s in again for q in s]
    spec += [("seq", again[0][0], again[0][1], dict(ll=T.fitted(every, 0, 9, (35,), (35,)), of=T.fitted(every, 1, 8, (20,), (20,)),
                                                    ml=T.fitted(every, 2, 9, (52,), (52,))))]
    spec += [("seq", l, s, allrep if s else {}) for l, s in again[1:]]
    return P.around(a, [T.encode_frame(spec)])


def body_counts(P, big):
    """Sequence counts of 1, 127 and 128 and of `big` (0x7EFF: two bytes; 0x7F00: three) in successive blocks."""
    a = P.row(4100)
    region = P.D[a:a + 125000]
    blocks = T.parse(region, max_ml=3, cut_every=[1, 127, 128, big, 1 << 20], use_repeats=False)
    return P.around(a, [T.encode_frame(T.steer(blocks))])


def body_batches(P):
    """Blocks of ZS_BATCH - 1, ZS_BATCH, ZS_BATCH + 1 and 2 * ZS_BATCH + 1 sequences in which every match reads the
    match before it; the first sequence of the second block reads below the first block's end and the next
    one reads what it wrote; a Raw block read by the first match; a second frame whose first match reads only
    its own literal run and reaches the frame's first byte."""
    a, r, spec = P.row(2400), 2401, [("raw", P.D[P.row(2400):P.row(2401) + DIGITS])]
    for k, n in enumerate((ZS_BATCH - 1, ZS_BATCH, ZS_BATCH + 1, 2 * ZS_BATCH + 1)):
        spec.append(_rows_block(P, r, n, first=2 * W if k == 1 else None))
        r += n
    s = P.row(r) + DIGITS + 3
    spec[-1] = ("seq", spec[-1][1] + P.D[s - 3:s], spec[-1][2], {})   # the digits: literals behind the last sequence
    one = T.encode_frame(spec)
    assert a + len(one[1]) == s
    lits = P.D[s:s + W] + P.D[s + 2 * W - 3:s + 2 * W]
    two = T.encode_frame([("seq", lits, [(W, W - 3, W), (3, W - 3, W)], {})], fcs=1, single=True)
    return P.around(a, [one, two])


def body_far(P):
    """One frame over the whole page. ML code 52 on the first 'Z' run. LL code 35, ML code 51 and the offset code of
    a distance above 256 KiB in one sequence, each with extra bits that are not 0: the stretch as one literal run,
    then the second 'Z' run copied from the first, in a block that stands for exactly 128 KiB. (LL 35 and ML 52
    cannot share a legal block: 65,537 + 65,540 bytes are more than Block_Maximum_Size, and libzstd decodes such a
    block only where it is a frame's last.) The last row is copied from the first, at the frame's first byte: the
    largest offset code the page allows."""
    D = P.D
    run1 = len(D[P.z1:]) - len(D[P.z1:].lstrip(b"Z"))
    ll = P.z2 - P.far_row
    ml = T.BLOCK_MAX - ll
    assert ml <= min(run1, P.z2_end - P.z2)
    top = dict(ll=T.fitted([(ll, 3, 1)], 0, 9, pad=(0,)), of=T.fitted([(0, 3, P.z2 - P.z1)], 1, 8, pad=(0,)),
               ml=T.fitted([(0, ml, 1)], 2, 9, pad=(0,)))
    spec = [("seq", D[:P.z1 + 1], [(P.z1 + 1, run1 - 1, 1)], {})]
    spec += [("raw", D[c:min(c + 100000, P.far_row)]) for c in range(P.z1 + run1, P.far_row, 100000)]
    spec.append(("seq", D[P.far_row:P.z2], [(ll, ml, P.z2 - P.z1)], dict(lit="compressed", streams=4, **top)))
    spec += [("raw", D[c:min(c + 100000, P.last)]) for c in range(P.z2 + ml, P.last, 100000)]
    spec.append(("seq", b"", [(0, len(D) - P.last, P.last)], {}))
    return P.around(0, [T.encode_frame(spec, fcs=4)])


def body_overlap(P):
    """Offsets 1, 2, 3, 63, 64 and 65 under matches longer than a wave."""
    a = P.periods[1] - 6
    region = P.D[a:P.periods[65] + 3 * 65 + 7]
    return P.around(a, [T.encode_frame(T.steer(T.parse(region, offsets=PERIODS, min_ml=4)))])


def body_repeats(P):
    """The written row: every repeat code, the rotation behind each, the offsets over a Raw block, and the three
    offsets of a fresh frame."""
    return P.around(P.written, [T.encode_frame(f, fcs=1 if len(T.run(f)) < 256 else 0, single=len(T.run(f)) < 256) for f in P.frames])


BODIES = {"literals": body_literals, "huffman": body_huffman, "slab": body_slab, "spliced": body_spliced, "tables": body_tables,
          "counts 0x7EFF": lambda P: body_counts(P, 0x7EFF), "counts 0x7F00": lambda P: body_counts(P, 0x7F00),
          "batches": body_batches, "far": body_far, "overlap": body_overlap, "repeats": body_repeats}


# ---- what each form must show ----------------------------------------------------------------------------
def _blocks(p, kind="compressed"):
    return [b for f in p.frames for b in f["blocks"] if b["type"] == kind]


def _lit(p, **want):
    """The compressed blocks whose literals section has these properties."""
    return [b for b in _blocks(p) if all(b["literals"][k] == v for k, v in want.items())]


def _placed(p):
    """[(frame index, block index, sequence index, frame start, where the match starts, ll, ml, distance)]"""
    out = []
    for fi, f in enumerate(p.frames):
        for bi, b in enumerate(f["blocks"]):
            at = b["start"]
            for si, q in enumerate(b.get("seqs", [])):
                out.append((fi, bi, si, f["start"], at + q[0], q[0], q[1], q[2]))
                at += q[0] + q[1]
    return out


def _modes_seen(p):
    """{(table, mode)} and {(table, "repeat after <the mode that built the table>")}"""
    out = set()
    for f in p.frames:
        built = [None] * 3
        for b in f["blocks"]:
            for t, m in enumerate(b.get("modes") or ()):
                out.add((t, m))
                if m == T.REPEAT:
                    out.add((t, "repeat after " + built[t]))
                else:
                    built[t] = m
    return out


def _zero_run(norm):
    """The longest run of zeros: four or more put a repeat flag of 3 (three more zeros, and another flag) behind the
    first one."""
    return max((len(r) for r in "".join("0" if x == 0 else " " for x in norm).split()), default=0)


def _repeat_over(p, kind):
    """Is there a block all in Repeat mode right behind a block of `kind` ("raw", or "none": no sequences)?"""
    for f in p.frames:
        bl = f["blocks"]
        for k in range(1, len(bl)):
            between = bl[k - 1]["type"] == "raw" if kind == "raw" else bl[k - 1]["type"] == "compressed" and bl[k - 1]["nseq"] == 0
            if between and bl[k].get("modes") == (T.REPEAT,) * 3:
                return True
    return False


def _reads_previous_batch(p):
    """A match at batch index 0 whose source is the last match of the batch before it."""
    for b in _blocks(p):
        at, spans = b["start"], []
        for ll, ml, d, _, _, _ in b["seqs"]:
            spans.append((at + ll, ml, d))
            at += ll + ml
        for k in range(ZS_BATCH, len(spans), ZS_BATCH):
            (m, ml, d), (pm, pml, _) = spans[k], spans[k - 1]
            if pm <= m - d and m - d + min(d, ml) <= pm + pml:
                return True
    return False


def _below_drained_then_read(p):
    """A block's first match whose source ends at or below the previous block's end, followed at once by a match
    that reads what it wrote."""
    for f in p.frames:
        for k, b in enumerate(f["blocks"]):
            if k and b.get("seqs") and len(b["seqs"]) > 1:
                (l0, m0, d0), (l1, m1, d1) = b["seqs"][0][:3], b["seqs"][1][:3]
                at0 = b["start"] + l0
                at1 = at0 + m0 + l1
                if at0 - d0 + min(d0, m0) <= b["start"] and at0 <= at1 - d1 < at0 + m0:
                    return True
    return False


def _reads_block(p, kind):
    """A match whose source lies wholly in the block before its own, of type `kind`."""
    for f in p.frames:
        for k, b in enumerate(f["blocks"]):
            if k and f["blocks"][k - 1]["type"] == kind and b.get("seqs"):
                prev, (ll, ml, d) = f["blocks"][k - 1], b["seqs"][0][:3]
                m = b["start"] + ll
                if prev["start"] <= m - d and m - d + min(d, ml) <= prev["end"]:
                    return True
    return False


def _frame_start_matches(p):
    """The indices, among the frames with blocks, of the frames that hold a match with off == op + ll - frame0."""
    real = [id(f) for f in p.frames if not f["skippable"]]
    return {real.index(id(p.frames[fi])) for fi, _, _, f0, m, _, _, d in _placed(p) if m - d == f0}


def _rep_events(p):
    """{(offset code, its extra bit, ll == 0)} of the repeat codes a body uses, and whether each is followed by
    Offset_Value 1 with ll > 0 in the same block."""
    seen = {}
    for f in p.frames:
        rep = [1, 4, 8]
        for b in f["blocks"]:
            seqs = b.get("seqs", [])
            values = []
            for ll, ml, d, oc, _, _ in seqs:
                cands = [v for v in (1, 2, 3) if T.offset_code(v)[0] == oc and T.resolve(rep, v, ll)[0] == d] if oc < 2 else []
                values.append(cands[0] if cands else None)
                rep = T.resolve(rep, cands[0] if cands else d + 3, ll)[1]
            for k, v in enumerate(values):
                if v:
                    proved = k + 1 < len(values) and values[k + 1] == 1 and seqs[k + 1][0] > 0
                    key = (T.offset_code(v)[0], T.offset_code(v)[1], seqs[k][0] == 0)
                    seen[key] = seen.get(key, False) or proved
    return seen


def _first_of_later_frames(p):
    """{distance} of the first sequence of every frame but the page's first, where it uses a repeat code behind a
    Raw block."""
    real = [f for f in p.frames if not f["skippable"]]
    out = set()
    for f in real[1:]:
        bl = f["blocks"]
        if len(bl) > 1 and bl[0]["type"] == "raw" and bl[1].get("seqs") and bl[1]["seqs"][0][3] < 2:
            out.add(bl[1]["seqs"][0][2])
    return out


def _rep_over_raw(p):
    for f in p.frames:
        bl = f["blocks"]
        for k in range(2, len(bl)):
            if bl[k - 1]["type"] == "raw" and bl[k - 2].get("seqs") and bl[k].get("seqs") and bl[k]["seqs"][0][3] < 2 and \
                    bl[k]["seqs"][0][2] not in (1, 4, 8):
                return True
    return False


def _overlaps(p):
    return {d for _, _, _, _, _, _, ml, d in _placed(p) if ml > 64 and d in PERIODS and (d == 1 or ml % d)}


def _treeless_after(p, what):
    for f in p.frames:
        bl = f["blocks"]
        for k, b in enumerate(bl):
            if b["type"] != "compressed" or b["literals"]["type"] != "treeless" or k == 0:
                continue
            if what == "compressed" and bl[k - 1]["type"] == "compressed" and bl[k - 1]["literals"]["type"] == "compressed":
                return True
            if what == "raw" and k > 1 and bl[k - 1]["type"] == "raw" and bl[k - 2]["type"] == "compressed" and \
                    bl[k - 2]["literals"]["type"] == "raw":
                return True
    return False


def _one_sequence_of_75_bits(p):
    """A sequence with LL code 35, ML code 51 and an offset code of 18 or more, every one with extra bits that are
    not 0, in a block whose tables are at the largest accuracy logs: 16 + 15 + 18 extra bits and 9 + 9 + 8 bits of
    state updates behind them, more than 64 bits between two state updates."""
    for b in _blocks(p):
        for ll, ml, d, oc, lc, mc in b["seqs"]:
            if lc == 35 and mc == 51 and oc >= 18 and ll > 65536 and ml > 32771 and d + 3 > 1 << oc:
                return b["logs"] == (9, 8, 9) and 16 + 15 + oc + sum(b["logs"]) > 64
    return False


def _largest_offset_code(p):
    n = len(p.data)
    top = (n - 1 + 3).bit_length() - 1
    return any(oc == top and d + 3 > 1 << oc for b in _blocks(p) for _, _, d, oc, _, _ in b["seqs"]) and top >= 18


FORMS = {
    # literals
    "raw literals with sequences": ("literals", lambda p: any(b["nseq"] for b in _lit(p, type="raw"))),
    "raw literals without sequences": ("literals", lambda p: any(not b["nseq"] for b in _lit(p, type="raw"))),
    "rle literals with sequences": ("literals", lambda p: any(b["nseq"] for b in _lit(p, type="rle"))),
    "rle literals without sequences": ("literals", lambda p: any(not b["nseq"] for b in _lit(p, type="rle"))),
    "raw and rle size formats": ("literals", lambda p: {(t, f) for t in ("raw", "rle") for f in (0, 1, 3)} | {("raw", 2)} <= {
        (b["literals"]["type"], b["literals"]["size_format"]) for b in _blocks(p)}),
    "one stream": ("huffman", lambda p: any(b["nseq"] for b in _lit(p, type="compressed", streams=1))),
    "four streams in lock step": ("huffman", lambda p: any(T.loose(b["literals"]) for b in _lit(p, type="compressed", streams=4))),
    "four streams, one under 8 bytes": ("huffman", lambda p: any(
        not T.loose(b["literals"]) and min(b["literals"]["stream_sizes"]) < 8 and b["literals"]["regen"] > 6
        for b in _lit(p, type="compressed", streams=4))),
    "four streams, regen 6": ("huffman", lambda p: any(not T.loose(b["literals"]) for b in _lit(p, streams=4, regen=6))),
    "treeless after compressed": ("huffman", lambda p: _treeless_after(p, "compressed")),
    "treeless after raw literals and a raw block": ("huffman", lambda p: _treeless_after(p, "raw")),
    "treeless on one stream": ("huffman", lambda p: bool(_lit(p, type="treeless", streams=1))),
    "regen below 32, below 4096, at least 4096": ("huffman", lambda p: (
        lambda r: any(x < 32 for x in r) and any(32 <= x < 4096 for x in r) and any(4096 <= x < SLAB for x in r))(
        [b["literals"]["regen"] for b in _blocks(p) if b["literals"]["type"] in ("compressed", "treeless")])),
    "compressed size formats 0 to 3": ("huffman", lambda p: {0, 1, 2, 3} <= {
        b["literals"]["size_format"] for b in _blocks(p) if b["literals"]["type"] in ("compressed", "treeless")}),
    "regen 131072 under the 5-byte header": ("slab", lambda p: bool(_lit(p, type="compressed", size_format=3, regen=SLAB))),
    "leftover literals: none": ("batches", lambda p: any(b["nseq"] and b["leftover"] == 0 for b in _blocks(p))),
    "leftover literals: some": ("repeats", lambda p: any(b["nseq"] and b["leftover"] > 0 for b in _blocks(p))),
    "direct weights": ("huffman", lambda p: bool(_lit(p, weights="direct"))),
    "FSE weights, spliced": ("spliced", lambda p: any(b["literals"]["weights"] == "fse" and b["logs"] == (9, 8, 9) for b in _blocks(p))),
    # tables
    "four modes on three tables": ("tables", lambda p: {(t, m) for t in range(3) for m in T.MODES} <= _modes_seen(p)),
    "repeat after each other mode": ("tables", lambda p: {(t, "repeat after " + m) for t in range(3) for m in (
        T.PREDEFINED, T.RLE, T.FSE)} <= _modes_seen(p)),
    "repeat across a raw block": ("tables", lambda p: _repeat_over(p, "raw")),
    "repeat across a block without sequences": ("tables", lambda p: _repeat_over(p, "none")),
    "accuracy logs 5 and 9/8/9": ("tables", lambda p: {(5, 5, 5), (9, 8, 9)} <= {b["logs"] for b in _blocks(p) if b["nseq"] and b[
        "modes"] == (T.FSE,) * 3}),
    "a less-than-1 symbol and a zero run under flag 3": ("tables", lambda p: all(
        any(b["norms"][t] and -1 in b["norms"][t] and _zero_run(b["norms"][t]) >= 4 for b in _blocks(p) if b["nseq"])
        for t in range(3))),
    # sequence codes
    "counts 1, 127, 128, 0x7EFF": ("counts 0x7EFF", lambda p: {(1, 1), (127, 1), (128, 2), (0x7EFF, 2)} <= {
        (b["nseq"], b["count_width"]) for b in _blocks(p)}),
    "count 0x7F00": ("counts 0x7F00", lambda p: any(b["nseq"] == 0x7F00 and b["count_width"] == 3 for b in _blocks(p))),
    "LL 35, ML 51 and offset code 18 in one sequence": ("far", _one_sequence_of_75_bits),
    "ML 52 with extra bits": ("far", lambda p: any(mc == 52 and ml > 65539 for b in _blocks(p) for _, ml, _, _, _, mc in b["seqs"])),
    "the largest offset code": ("far", _largest_offset_code),
    # batches and drained
    "blocks around ZS_BATCH": ("batches", lambda p: {ZS_BATCH - 1, ZS_BATCH, ZS_BATCH + 1, 2 * ZS_BATCH + 1} <= {
        b["nseq"] for b in _blocks(p)}),
    "batch index 0 reads the batch before": ("batches", _reads_previous_batch),
    "a source below drained, then read": ("batches", _below_drained_then_read),
    "a match inside its own literal run": ("batches", lambda p: any(d <= ll and d >= ml for _, _, _, _, _, ll, ml, d in _placed(p))),
    "a raw block read": ("batches", lambda p: _reads_block(p, "raw")),
    "an rle block read": ("literals", lambda p: _reads_block(p, "rle")),
    "the frame's first byte, first frame": ("far", lambda p: 0 in _frame_start_matches(p)),
    "the frame's first byte, second frame": ("batches", lambda p: any(k > 0 for k in _frame_start_matches(p))),
    # overlap
    "overlap at 1, 2, 3, 63, 64, 65": ("overlap", lambda p: _overlaps(p) == set(PERIODS)),
    # repeat offsets
    "every repeat code, rotation proved": ("repeats", lambda p: _rep_events(p) == {
        (c, x, z): True for c, x in ((0, 0), (1, 0), (1, 1)) for z in (False, True)}),
    "repeat offsets over a raw block": ("repeats", _rep_over_raw),
    "distances 1, 4, 8 at later frames' starts": ("repeats", lambda p: _first_of_later_frames(p) >= {1, 4, 8}),
}


# ---- the fixtures ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    from delta_amd.delta_log import Engine
    return Engine.get(0)


def build_base(d, rows_of=_rows):
    """(the SNAPPY twin's log, the checkpoint's name, the steered table, cutoff, the oracle's snapshot, the original
    table): everything the bodies need, without a device."""
    import pyarrow.parquet as pq
    from delta_amd.testing import synth as S
    exp = S.build_table(d, S.config_spec(3, 0.001), seed=3)
    lp = os.path.join(d, "_delta_log")
    ck = [f for f in os.listdir(lp) if f.endswith(".checkpoint.parquet")]
    assert len(ck) == 1
    original = pq.read_table(os.path.join(lp, ck[0]))
    cutoff = exp.min_file_retention_timestamp
    live = {a["path"]: a.get("stats") for a in O.state_reconstruction(O.get_log_segment(lp), cutoff).all_files}
    add = original.column("add").combine_chunks()
    shown = [p in live and live[p] == s for p, s, v in zip(add.field("path").to_pylist(), add.field("stats").to_pylist(),
                                                            add.is_valid().to_pylist()) if v]
    table = _steered_table(original, rows_of, shown)
    pq.write_table(table, os.path.join(lp, ck[0]), compression="snappy", use_dictionary=False, version="1.0",
                   write_statistics=False)
    return lp, ck[0], table, cutoff, O.state_reconstruction(O.get_log_segment(lp), cutoff), original


def zstd_variant(base, d, table=None, level=1, page_size=1 << 20):
    """A copy of the twin's log with the checkpoint as ZSTD, DATA_PAGE_V2; (log path, checkpoint path)."""
    import pyarrow.parquet as pq
    lp = os.path.join(str(d), "_delta_log")
    shutil.copytree(base[0], lp)
    kw = {"write_batch_size": 32} if page_size < 65536 else {}
    pq.write_table(base[2] if table is None else table, os.path.join(lp, base[1]), compression="zstd", compression_level=level,
                   use_dictionary=False, version="1.0", data_page_version="2.0", data_page_size=page_size, write_statistics=False, **kw)
    return lp, os.path.join(lp, base[1])


def page_of(ck):
    pages = Z.zstd_pages(ck, "add.stats")
    assert len(pages) == 1
    at, c, u = pages[0]
    data = Z.reference(open(ck, "rb").read()[at:at + c], u)
    assert data is not None and len(data) == u
    return Page(data)


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    return build_base(str(tmp_path_factory.mktemp("zb_base")))


@pytest.fixture(scope="module")
def good(base, tmp_path_factory):
    """(log path, checkpoint path, Page) of the ZSTD variant every case starts from."""
    lp, ck = zstd_variant(base, tmp_path_factory.mktemp("zb_good"))
    P = page_of(ck)
    assert len(P.D) == 572250   # the page's length
    return lp, ck, P


@pytest.fixture(scope="module")
def twin(engine, base):
    """export(0) and export(1) of the SNAPPY twin."""
    staged = engine.stage_log(base[0])
    try:
        st = staged.replay(base[3])
    finally:
        staged.release()
    try:
        live = st.export(0)
        assert sum(STRETCH in (a.get("stats") or "") for a in live) == 1 and sum((a.get("stats") or "") == MARKER for a in live) == 2
        return live, st.export(1)
    finally:
        st.release()


_parsed = {}


def parsed_body(P, name):
    if name not in _parsed:
        body = BODIES[name](P)
        p = T.sequences(body)
        assert p.data == P.D
        _parsed[name] = (body, p)
    return _parsed[name]


def _replay_body(engine, base, good, twin, tmp, body):
    lp = os.path.join(str(tmp), "_delta_log")
    shutil.copytree(good[0], lp)
    L.rewrite(good[1], os.path.join(lp, base[1]), {("add.stats", 0): (6, body)})
    staged = engine.stage_log(lp)
    try:
        st = staged.replay(base[3])
    finally:
        staged.release()
    try:
        assert st.export(0) == twin[0] and st.export(1) == twin[1]
        _assert_same(st, base[4])
    finally:
        st.release()


@pytest.fixture(scope="module")
def replayed(engine, base, good, twin, tmp_path_factory):
    """replayed(name): the table with that body is replayed once, and whatever that raised is raised again for every
    form that shares the body, so each of them shows the difference itself."""
    results = {}

    def get(name):
        if name not in results:
            try:
                _replay_body(engine, base, good, twin, tmp_path_factory.mktemp("zb_body"), parsed_body(good[2], name)[0])
                results[name] = None
            except Exception as e:   # kept for the forms that follow
                results[name] = e
        if results[name] is not None:
            raise results[name]
    return get


@pytest.mark.parametrize("form", sorted(FORMS))
def test_form(good, replayed, form):
    """The body shows the form (asserted on its bytes), and the table with that body replays as the twin."""
    name, shows = FORMS[form]
    assert shows(parsed_body(good[2], name)[1]), form
    replayed(name)


def test_every_body_has_a_form():
    assert {name for name, _ in FORMS.values()} == set(BODIES)


# ---- refusals -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", T.REFUSALS)
def test_refusals(engine, base, good, twin, tmp_path, kind):
    """Bounds checks of the kernel: each body is refused by libzstd here and by the host program in
    tests/test_zstd_steer.py first; on the device it ends in DR_E_PARQUET naming the column, and a good table
    replays afterwards."""
    from delta_amd.delta_log import DeltaError
    body = T.refused_bodies()[kind]
    assert Z.reference(body, len(good[2].D)) is None
    lp = os.path.join(str(tmp_path), "_delta_log")
    shutil.copytree(good[0], lp)
    L.rewrite(good[1], os.path.join(lp, base[1]), {("add.stats", 0): (6, body)})
    with pytest.raises(DeltaError) as e:   # add.stats is decoded when the state is exported
        staged = engine.stage_log(lp)
        try:
            st = staged.replay(base[3])
        finally:
            staged.release()
        try:
            st.export(0)
        finally:
            st.release()
    assert e.value.code == "DR_E_PARQUET" and "zstd page in add.stats" in str(e.value), str(e.value)
    _replay_body(engine, base, good, twin, tmp_path / "good", Z.one_shot(good[2].D, 1))


# ---- the census ---------------------------------------------------------------------------------------------
def census(base, good, tmp):
    """(forms of the pages pyarrow writes for the table of test_gpu_zstd_pages.test_parity at levels 1 and 19 and
    both page sizes, forms of the steered bodies)."""
    import pyarrow.parquet as pq
    written = set()
    for level in (1, 19):
        for page_size in (4096, 1 << 20):
            _, ck = zstd_variant(base, os.path.join(str(tmp), "l%d_%d" % (level, page_size)), table=base[5], level=level,
                                 page_size=page_size)
            buf = open(ck, "rb").read()
            md = pq.ParquetFile(ck).metadata
            for leaf in sorted({md.row_group(0).column(c).path_in_schema for c in range(md.num_columns)}):
                for at, c, u in Z.zstd_pages(ck, leaf):
                    if c:
                        written |= T.forms(T.sequences(buf[at:at + c], decode=False))
    steered = set()
    for name in BODIES:
        steered |= T.forms(parsed_body(good[2], name)[1])
    return written, steered


def test_census(base, good, tmp_path):
    """Every feature of the format reaches the device in some page: in one pyarrow writes, or in a steered body."""
    written, steered = census(base, good, tmp_path)
    print("only the steered bodies supply:", sorted(steered - written))
    assert not Z.FEATURES - (written | steered), sorted(Z.FEATURES - (written | steered))
