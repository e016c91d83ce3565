"""A steered ZSTD encoder and a strict block reader, written from RFC 8878 for the tests of k_zstd and
the host decoder. Neither shares code with zstd_fmt.h: the reader is the independent side.

  sequences(body)   per frame and per block: the block type, the literals form, the width of the sequence
                    count, the mode and accuracy log of each table, every sequence with its codes and its
                    repeat offset resolved, and the decoded bytes;
  encode_block      one Compressed block from an explicit literal string and explicit (ll, ml, offset)
                    triples, with the literals form and each table's mode chosen by the caller;
  encode_frame      blocks (Raw, RLE, steered) under a frame header, with the content they stand for;
  parse             a greedy parser that turns real bytes into such blocks, steered by its options.

An offset is a distance (> 0) or one of REP1, REP2, REP3: the Offset_Values 1, 2 and 3, which the
offset codes 0 (value 1) and 1 (values 2 and 3, by its one extra bit) carry."""
import heapq
import struct
from collections import namedtuple

from tests import zstd_corpus as Z

REP1, REP2, REP3 = -1, -2, -3
PREDEFINED, RLE, FSE, REPEAT = "predefined", "rle", "fse", "repeat"
MODES = (PREDEFINED, RLE, FSE, REPEAT)
LIT_TYPES = ("raw", "rle", "compressed", "treeless")
BLOCK_MAX = 128 * 1024

LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387,
                                32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
DEFAULT = (([4, 3] + [2] * 11 + [1] * 3 + [2] * 9 + [3, 2] + [1] * 5 + [-1] * 4, 6),      # literal lengths
           ([1] * 6 + [2] * 3 + [1] * 15 + [-1] * 5, 5),                                     # offsets
           ([1, 4, 3] + [2] * 6 + [1] * 37 + [-1] * 7, 6))                                   # match lengths
MAX_SYM, MAX_LOG = (35, 31, 52), (9, 8, 9)
assert len(LL_BASE) == len(LL_BITS) == 36 and len(ML_BASE) == len(ML_BITS) == 53
assert [len(d) for d, _ in DEFAULT] == [36, 29, 53] and all(sum(abs(p) for p in d) == 1 << lg for d, lg in DEFAULT)


class Malformed(Exception):
    """What the strict reader raises for a stream that RFC 8878 does not allow."""


def _need(ok, what):
    if not ok:
        raise Malformed(what)


def code_of(value, base):
    """The code whose range holds `value`, and the extra bits' value."""
    c = max(k for k in range(len(base)) if base[k] <= value)
    return c, value - base[c]


def offset_code(value):
    """(offset code, extra bits' value) of an Offset_Value >= 1."""
    c = value.bit_length() - 1
    return c, value - (1 << c)


def resolve(rep, value, ll):
    """(distance, the repeat offsets afterwards) of Offset_Value `value` in a sequence whose literal
    length is ll (RFC 8878 3.1.1.5); a distance of 0 (Repeated_Offset1 - 1 of 1) is the caller's to refuse."""
    if value > 3:
        return value - 3, [value - 3, rep[0], rep[1]]
    k = value - 1 + (ll == 0)
    if k == 0:
        return rep[0], list(rep)
    if k == 1:
        return rep[1], [rep[1], rep[0], rep[2]]
    d = rep[2] if k == 2 else rep[0] - 1
    return d, [d, rep[0], rep[1]]


# ---- FSE -------------------------------------------------------------------------------------------
def fse_table(norm, log):
    """[(symbol, bits to read, baseline)] per state, by the RFC's spread (4.1.1)."""
    size = 1 << log
    _need(sum(abs(p) for p in norm) == size, "the distribution does not fill the table")
    sym, high = [0] * size, size - 1
    for s, p in enumerate(norm):
        if p == -1:
            sym[high] = s
            high -= 1
    step, pos = (size >> 1) + (size >> 3) + 3, 0
    for s, p in enumerate(norm):
        for _ in range(max(p, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    nxt = [1 if p == -1 else p for p in norm]
    table = []
    for u in range(size):
        s = sym[u]
        ns = nxt[s]
        nxt[s] += 1
        nb = log - (ns.bit_length() - 1)
        table.append((s, nb, (ns << nb) - size))
    return table


def write_distribution(norm, log):
    """The FSE table description of norm (the last entry is not 0) at accuracy log `log`: "less than 1"
    probabilities are -1, and a run of zeros behind a zero goes into two-bit repeat flags."""
    assert 5 <= log <= 15 and norm[-1] != 0 and sum(abs(p) for p in norm) == 1 << log
    acc, bp = log - 5, 4
    remaining, threshold, nb, s = (1 << log) + 1, 1 << log, log + 1, 0

    def emit(v, k):
        nonlocal acc, bp
        acc |= v << bp
        bp += k
    while s < len(norm):
        p = norm[s]
        val, mx = p + 1, 2 * threshold - 1 - remaining
        if val < mx:
            emit(val, nb - 1)
        elif val < threshold:
            emit(val, nb)
        else:
            emit(val + mx, nb)
        remaining -= abs(p)
        s += 1
        if p == 0:
            z = 0
            while norm[s] == 0:
                z, s = z + 1, s + 1
            while z >= 3:
                emit(3, 2)
                z -= 3
            emit(z, 2)
        if remaining < threshold:
            if remaining <= 1:
                break
            nb = remaining.bit_length()
            threshold = 1 << (nb - 1)
    assert remaining == 1 and s == len(norm)
    return acc.to_bytes((bp + 7) // 8, "little")


def read_distribution(s, pos, end, max_sym):
    """(norm, log, bytes taken) of the table description at s[pos:end]."""
    _need(pos < end, "no table description")
    v = int.from_bytes(s[pos:end], "little")
    avail = 8 * (end - pos)
    log, bp = (v & 15) + 5, 4
    remaining, norm = 1 << log, []
    while remaining > 0:
        _need(len(norm) <= max_sym, "more symbols than the alphabet")
        k = (remaining + 1).bit_length()
        low = (1 << k) - 1 - (remaining + 1)
        x = v >> bp & ((1 << k) - 1)
        if x & ((1 << (k - 1)) - 1) < low:
            x &= (1 << (k - 1)) - 1
            bp += k - 1
        else:
            bp += k
            if x >= 1 << (k - 1):
                x -= low
        p = x - 1
        norm.append(p)
        remaining -= abs(p)
        if p == 0:
            while True:
                r = v >> bp & 3
                bp += 2
                norm += [0] * r
                if r != 3:
                    break
        _need(bp <= avail, "the table description runs past its section")
    _need(remaining == 0 and len(norm) <= max_sym + 1, "the distribution overshoots")
    return norm, log, (bp + 7) // 8


def distribution(used, log, less_than_one=(), heavy=None):
    """A normalised distribution at `log` over the symbols `used`: the ones of less_than_one get -1, the
    others 1, and `heavy` (default: the smallest other symbol) takes what is left."""
    n = max(used) + 1
    norm = [0] * n
    for s in used:
        norm[s] = -1 if s in less_than_one else 1
    heavy = min(s for s in used if s not in less_than_one) if heavy is None else heavy
    norm[heavy] += (1 << log) - sum(abs(p) for p in norm)
    assert norm[heavy] >= 1
    return norm


# ---- bits read backwards ---------------------------------------------------------------------------
def _backward(fields):
    """The bytes of a stream from which (value, bits) fields are read in this order, the first one right
    below the final-bit marker."""
    parts = ["1"] + [format(v, "0%db" % k) for v, k in fields if k]
    bits = "".join(parts)
    return int(bits, 2).to_bytes((len(bits) + 7) // 8, "little")


class _Bits:
    """The bits of s[start:end] as the decoder meets them, behind the marker."""

    def __init__(self, s, start, end):
        _need(end > start and s[end - 1] != 0, "a bitstream without its final-bit marker")
        self.bits = bin(int.from_bytes(s[start:end], "little"))[3:]
        self.at = 0

    def take(self, k):
        if k == 0:
            return 0
        _need(self.at + k <= len(self.bits), "a bitstream read past its start")
        v = int(self.bits[self.at:self.at + k], 2)
        self.at += k
        return v

    def left(self):
        return len(self.bits) - self.at


# ---- Huffman -----------------------------------------------------------------------------------------
def huffman_weights(data, max_bits=11):
    """Weights (index: symbol, up to the largest one present) of a Huffman code for `data` whose codes are at
    most max_bits long; at least two symbols must occur."""
    freq = {}
    for b in data:
        freq[b] = freq.get(b, 0) + 1
    assert len(freq) >= 2
    while True:
        heap = [(f, s, (s,)) for s, f in sorted(freq.items())]
        heapq.heapify(heap)
        length = dict.fromkeys(freq, 0)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                length[s] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        top = max(length.values())
        if top <= max_bits:
            break
        freq = {s: (f >> 1) | 1 for s, f in freq.items()}
    w = [0] * (max(freq) + 1)
    for s, n in length.items():
        w[s] = top + 1 - n
    return w


def huffman_codes(weights):
    """({symbol: (code, length)}, table log) of a complete weight list (RFC 8878 4.2.1.3)."""
    total = sum(1 << (w - 1) for w in weights if w)
    log = total.bit_length() - 1
    _need(total == 1 << log and log >= 1, "Huffman weights do not fill a tree")
    at, codes = 0, {}
    for w in range(1, log + 1):
        for s, ws in enumerate(weights):
            if ws == w:
                codes[s] = (at >> (w - 1), log + 1 - w)
                at += 1 << (w - 1)
    return codes, log


def direct_weights(weights):
    """The tree description with 4-bit weights; the last symbol's weight is implied."""
    given = list(weights[:-1])
    assert weights[-1] and 1 <= len(given) <= 128
    given += [0] * (len(given) & 1)
    return bytes([127 + len(weights) - 1]) + bytes(given[i] << 4 | given[i + 1] for i in range(0, len(given), 2))


def huffman_stream(data, codes):
    return _backward([codes[b] for b in data])


def _read_weights(s, pos, end):
    """(weights with the implied one, "direct" or "fse", bytes taken) of the tree description at s[pos:end]."""
    _need(pos < end, "no tree description")
    hb = s[pos]
    if hb >= 128:
        n, kind = hb - 127, "direct"
        used = 1 + (n + 1) // 2
        _need(pos + used <= end, "the weights run past the section")
        w = [s[pos + 1 + i // 2] >> (0 if i & 1 else 4) & 15 for i in range(n)]
    else:
        kind, used = "fse", 1 + hb
        _need(hb and pos + used <= end, "the weights run past the section")
        norm, log, taken = read_distribution(s, pos + 1, pos + used, 255)
        _need(log <= 6, "the weights' accuracy log is over 6")
        tab = fse_table(norm, log)
        br = _Bits(s, pos + 1 + taken, pos + used)
        s1, s2, w = br.take(log), br.take(log), []
        while True:   # two states take turns; the stream ends when one of them cannot be refilled
            w.append(tab[s1][0])
            if br.left() < tab[s1][1]:
                w.append(tab[s2][0])
                break
            s1 = tab[s1][2] + br.take(tab[s1][1])
            w.append(tab[s2][0])
            if br.left() < tab[s2][1]:
                w.append(tab[s1][0])
                break
            s2 = tab[s2][2] + br.take(tab[s2][1])
        _need(len(w) <= 255, "more than 255 weights")
    total = sum(1 << (x - 1) for x in w if x)
    _need(total > 0 and all(x <= 12 for x in w), "weights out of range")
    rest = (1 << total.bit_length()) - total
    _need(rest & (rest - 1) == 0, "the implied weight is no power of two")
    return w + [rest.bit_length()], kind, used


def _decode_stream(s, start, end, codes_by_bits, log, count):
    br = _Bits(s, start, end)
    bits, at, out = br.bits + "0" * log, 0, bytearray()
    for _ in range(count):
        sym, n = codes_by_bits[bits[at:at + log]]
        out.append(sym)
        at += n
    _need(at == len(br.bits), "a Huffman stream is not consumed exactly")
    return bytes(out)


# ---- the literals section ----------------------------------------------------------------------------
def literals_section(kind, literals, streams=1, weights=None, tree=None, size_format=None):
    """kind "raw", "rle" (literals: one byte repeated), "compressed" (direct weights from `weights`, or
    tree = (description bytes, its weights) to splice a description written elsewhere), "treeless"
    (weights: the tree the decoder still holds). size_format: the header's two bits; default the smallest."""
    t, n = LIT_TYPES.index(kind), len(literals)
    if t < 2:
        fmt = (0 if n < 32 else 1 if n < 4096 else 3) if size_format is None else size_format
        # the one-byte header has a one-bit format: what reads as size format 2 is format 0 with an odd size
        assert fmt in (0, 1, 3) and n < (32, 4096, 0, 1 << 20)[fmt] and (t == 0 or literals == literals[:1] * n)
        head = bytes([t | n << 3]) if fmt == 0 else struct.pack("<I", t | fmt << 2 | n << 4)[:2 if fmt == 1 else 3]
        return head + (literals if t == 0 else literals[:1])
    desc, weights = tree if tree is not None else (direct_weights(weights) if t == 2 else b"", weights)
    codes, _ = huffman_codes(weights)
    if streams == 1:
        body = huffman_stream(literals, codes)
    else:
        seg = (n + 3) // 4
        parts = [huffman_stream(literals[k * seg:(k + 1) * seg] if k < 3 else literals[3 * seg:], codes) for k in range(4)]
        body = struct.pack("<3H", *[len(p) for p in parts[:3]]) + b"".join(parts)
    body = (desc if t == 2 else b"") + body
    if size_format is None:
        size_format = 0 if streams == 1 else 1 if max(n, len(body)) < 1024 else 2 if max(n, len(body)) < 16384 else 3
    assert (size_format == 0) == (streams == 1)
    bits = (10, 10, 14, 18)[size_format]
    assert n < 1 << bits and len(body) < 1 << bits
    return (t | size_format << 2 | n << 4 | len(body) << (4 + bits)).to_bytes((3, 3, 4, 5)[size_format], "little") + body


# ---- the encoder -------------------------------------------------------------------------------------
class Context:
    """What an encoder carries from block to block of a frame: the three tables and the Huffman weights."""

    def __init__(self):
        self.tables = [None, None, None]   # (table, log)
        self.weights = None


def _states(table, syms):
    """The state per sequence of one table, chosen backwards: the last sequence takes any state of its
    symbol, each earlier one the state of its symbol whose baseline range holds the state that follows."""
    by = {}
    for u, (s, nb, base) in enumerate(table):
        by.setdefault(s, []).append((base, nb, u))
    out, nxt = [None] * len(syms), None
    for i in range(len(syms) - 1, -1, -1):
        cands = by.get(syms[i])
        assert cands, "symbol %d is not in the table" % syms[i]
        st = cands[0] if nxt is None else next(c for c in cands if c[0] <= nxt < c[0] + (1 << c[1]))
        out[i], nxt = st, st[2]
    return out


def encode_block(literals, seqs, ctx=None, lit="raw", streams=1, weights=None, tree=None, size_format=None,
                 ll=PREDEFINED, of=PREDEFINED, ml=PREDEFINED, count_width=None):
    """The body of a Compressed block. seqs: [(ll, ml, offset)], an offset being a distance or REP1..REP3.
    lit: the literals form (literals_section). ll / of / ml: PREDEFINED, RLE, REPEAT, or (FSE, norm, log).
    ctx: the frame's Context, needed for REPEAT and for Treeless literals. Nothing here checks that the
    sequences fit the literals or the output: refused blocks are built with it too."""
    ctx = Context() if ctx is None else ctx
    if lit == "compressed":
        weights = tree[1] if tree is not None else huffman_weights(literals) if weights is None else weights
        ctx.weights = weights
    out = literals_section(lit, literals, streams, ctx.weights if lit == "treeless" else weights, tree, size_format)
    n = len(seqs)
    w = (1 if n < 128 else 2 if n < 0x7f00 else 3) if count_width is None else count_width
    assert (w == 1 and n < 128) or (w == 2 and n < 0x7f00) or (w == 3 and 0x7f00 <= n < 0x7f00 + 65536)
    out += bytes([n]) if w == 1 else bytes([0x80 + (n >> 8), n & 255]) if w == 2 else b"\xff" + struct.pack("<H", n - 0x7f00)
    if n == 0:
        return out
    codes = []
    for l, m, o in seqs:
        codes.append((code_of(l, LL_BASE), offset_code(o + 3 if o > 0 else -o), code_of(m, ML_BASE)))
    modes, desc = (ll, of, ml), b""
    for t, mode in enumerate(modes):
        syms = {c[t][0] for c in codes}
        if mode == PREDEFINED:
            ctx.tables[t] = (fse_table(*DEFAULT[t]), DEFAULT[t][1])
        elif mode == RLE:
            assert len(syms) == 1
            desc += bytes(syms)
            ctx.tables[t] = ([(min(syms), 0, 0)], 0)
        elif mode == REPEAT:
            assert ctx.tables[t] is not None
        else:
            _, norm, log = mode
            desc += write_distribution(norm, log)
            ctx.tables[t] = (fse_table(norm, log), log)
    name = lambda m: m if isinstance(m, str) else m[0]
    out += bytes([MODES.index(name(ll)) << 6 | MODES.index(name(of)) << 4 | MODES.index(name(ml)) << 2]) + desc
    st = [_states(ctx.tables[t][0], [c[t][0] for c in codes]) for t in range(3)]
    fields = [(st[t][0][2], ctx.tables[t][1]) for t in range(3)]
    for i, ((lc, lx), (oc, ox), (mc, mx)) in enumerate(codes):
        fields += [(ox, oc), (mx, ML_BITS[mc]), (lx, LL_BITS[lc])]
        if i + 1 < n:
            fields += [(st[t][i + 1][2] - st[t][i][0], st[t][i][1]) for t in (0, 2, 1)]
    return out + _backward(fields)


def run(blocks):
    """The bytes that the blocks of one frame stand for. A block: ("raw", bytes), ("rle", byte, count) or
    ("seq", literals, seqs, options of encode_block)."""
    out, rep = bytearray(), [1, 4, 8]
    for b in blocks:
        if b[0] == "raw":
            out += b[1]
        elif b[0] == "rle":
            out += b[1] * b[2]
        else:
            at, lits = 0, b[1]
            for l, m, o in b[2]:
                out += lits[at:at + l]
                at += l
                d, rep = resolve(rep, o + 3 if o > 0 else -o, l)
                assert 0 < d <= len(out), "offset %d with %d bytes of output" % (d, len(out))
                for _ in range(m):
                    out.append(out[-d])
            assert at <= len(lits)
            out += lits[at:]
    return bytes(out)


def encode_frame(blocks, ctx=None, **frame_options):
    """(the frame, its content) of blocks as run() takes them; frame_options go to zstd_corpus.frame
    (default: a Window_Descriptor of 1 MiB and no content size)."""
    ctx = Context() if ctx is None else ctx
    content, out = run(blocks), b""
    for k, b in enumerate(blocks):
        last = k + 1 == len(blocks)
        if b[0] == "raw":
            out += Z.block(0, b[1], last=last)
        elif b[0] == "rle":
            out += Z.block(1, b[1], b[2], last=last)
        else:
            body = encode_block(b[1], b[2], ctx, **(b[3] if len(b) > 3 else {}))
            assert len(body) <= BLOCK_MAX
            out += Z.block(2, body, last=last)
    frame_options.setdefault("fcs", 0)
    return Z.frame(out, content, **frame_options), content


# ---- the steered parser ------------------------------------------------------------------------------
def parse(data, offsets=(), max_ml=None, min_ll=0, use_repeats=True, cut_every=None, min_ml=3, literal=()):
    """[(literals, [(ll, ml, offset)])]: blocks of one frame that decode to `data`, found greedily. At every
    position the distances of `offsets` are tried first, then the most recent earlier occurrence of the next
    min_ml bytes. max_ml caps a match, min_ll forbids a match before that many literals; with use_repeats a
    distance that a repeat offset holds is sent as REP1..REP3. cut_every: a block ends after that many
    sequences (an int, or a list of counts for the successive blocks, the last one repeated), and always
    before it would stand for more than 128 KiB. literal: (start, end) ranges in which no match starts."""
    n, table, i, anchor = len(data), {}, 0, 0
    blocks, seqs, lits, start, rep = [], [], bytearray(), 0, [1, 4, 8]
    cuts = [cut_every] if isinstance(cut_every, int) else list(cut_every or [])

    def close():
        nonlocal seqs, lits, start, anchor
        blocks.append((bytes(lits), seqs))
        seqs, lits, start = [], bytearray(), anchor
    while i < n:
        limit = cuts[min(len(blocks), len(cuts) - 1)] if cuts else None
        room = start + BLOCK_MAX - i
        if room <= 0:   # the block is full of literals
            lits += data[anchor:i]
            anchor = i
            close()
            continue
        key = data[i:i + min_ml]
        cand = [i - d for d in offsets if 0 < d <= i]
        if key in table:
            cand.append(table[key])
        table[key] = i
        best = None
        if i - anchor >= min_ll and not any(a <= i < b for a, b in literal) and room >= min_ml and i + min_ml <= n:
            for c in cand:
                if data[c:c + min_ml] != key:
                    continue
                ml, top = min_ml, min(n - i, room, max_ml or n)
                while ml < top and data[c + ml] == data[i + ml]:
                    ml += 1
                best = (i - c, ml)
                break
        if best is None:
            i += 1
            continue
        d, ml = best
        ll, value = i - anchor, d + 3
        if use_repeats:
            for v in (1, 2, 3):
                if resolve(rep, v, ll)[0] == d:
                    value = v
                    break
        rep = resolve(rep, value, ll)[1]
        lits += data[anchor:i]
        seqs.append((ll, ml, -value if value <= 3 else d))
        for j in range(i + 1, min(i + ml, n - min_ml + 1), 7):   # sparse: keeps later matches recent
            table[data[j:j + min_ml]] = j
        i += ml
        anchor = i
        if limit and len(seqs) == limit:
            close()
    lits += data[anchor:]
    anchor = n
    if lits or seqs or not blocks:
        close()
    assert run([("seq", l, s) for l, s in blocks]) == data
    return blocks


def steer(blocks, **options):
    """parse()'s blocks as encode_frame takes them, every one with the same options."""
    return [("seq", l, s, dict(options)) for l, s in blocks]


def fitted(seqs, t, log, less_than_one=(), pad=()):
    """(FSE, norm, log) for table t (0 LL, 1 OF, 2 ML) that holds every code of `seqs` (and of `pad`)."""
    used = set(pad)
    for l, m, o in seqs:
        used.add((code_of(l, LL_BASE)[0], offset_code(o + 3 if o > 0 else -o)[0], code_of(m, ML_BASE)[0])[t])
    return (FSE, distribution(used, log, less_than_one), log)


# ---- the strict reader -------------------------------------------------------------------------------
Parsed = namedtuple("Parsed", "frames data")


def sequences(body, decode=True):
    """Parsed(frames, data) of a well-formed stream; Malformed otherwise. A frame: {skippable, single,
    checksum, fcs (bytes of the size field), start (of its output in data), blocks}. A block: {type ("raw",
    "rle", "compressed"), size, last, start, end (of its output)} and, for a compressed one, literals = {type,
    size_format, streams, weights ("direct", "fse" or None), regen, stream_sizes, log, tree (the description's
    bytes and the weights)}, count_width (0 for no sequences), modes, logs and norms (LL, OF, ML; a norm is the
    distribution an FSE_Compressed table was described with, else None), seqs = [(ll, ml,
    distance, of_code, ll_code, ml_code)], leftover (literals behind the last sequence). decode=False: the
    forms only -- literals are not decoded and no sequence is read; data is then None."""
    frames, out, pos = [], bytearray(), 0
    while pos < len(body):
        _need(pos + 4 <= len(body), "a truncated magic number")
        magic = struct.unpack_from("<I", body, pos)[0]
        if magic & 0xfffffff0 == 0x184D2A50:
            _need(pos + 8 <= len(body), "a truncated skippable frame")
            size = struct.unpack_from("<I", body, pos + 4)[0]
            _need(pos + 8 + size <= len(body), "a skippable frame past the end")
            frames.append({"skippable": True, "blocks": [], "start": len(out), "checksum": False})
            pos += 8 + size
            continue
        _need(magic == Z.MAGIC, "no frame")
        d, at = body[pos + 4], pos + 5
        single, fcs = d >> 5 & 1, (d >> 5 & 1, 2, 4, 8)[d >> 6]
        _need(not d & 0x08, "a reserved descriptor bit")
        at += 0 if single else 1
        did = (0, 1, 2, 4)[d & 3]
        _need(int.from_bytes(body[at:at + did], "little") == 0, "a dictionary")
        at += did
        size = int.from_bytes(body[at:at + fcs], "little") + (256 if fcs == 2 else 0) if fcs else None
        at += fcs
        f = {"skippable": False, "single": bool(single), "checksum": bool(d >> 2 & 1), "fcs": fcs, "blocks": [],
             "start": len(out)}
        st = {"rep": [1, 4, 8], "tables": [None] * 3, "huf": None}
        while True:
            _need(at + 3 <= len(body), "a truncated block header")
            h = int.from_bytes(body[at:at + 3], "little")
            at += 3
            b = {"type": ("raw", "rle", "compressed", None)[h >> 1 & 3], "size": h >> 3, "last": bool(h & 1), "start": len(out)}
            _need(b["type"] is not None, "block type 3")
            take = 1 if b["type"] == "rle" else b["size"]
            _need(at + take <= len(body), "a block past the end")
            if b["type"] == "raw":
                out += body[at:at + take]
            elif b["type"] == "rle":
                out += body[at:at + 1] * b["size"]
            else:
                _need(b["size"] <= BLOCK_MAX, "a block over 128 KiB")
                _block(body, at, at + take, b, st, out, f["start"], decode)
            b["end"] = len(out)
            at += take
            f["blocks"].append(b)
            if b["last"]:
                break
        if decode:
            _need(size is None or size == len(out) - f["start"], "Frame_Content_Size differs")
        if f["checksum"]:
            _need(at + 4 <= len(body), "a truncated checksum")
            if decode:
                _need(struct.unpack_from("<I", body, at)[0] == Z.xxh64(bytes(out[f["start"]:])) & 0xffffffff, "checksum")
            at += 4
        frames.append(f)
        pos = at
    return Parsed(frames, bytes(out) if decode else None)


def _block(s, pos, end, b, st, out, frame0, decode):
    _need(end - pos >= 2, "a compressed block under two bytes")
    t, fmt = s[pos] & 3, s[pos] >> 2 & 3
    L = b["literals"] = {"type": LIT_TYPES[t], "size_format": fmt, "streams": 1, "weights": None, "stream_sizes": None,
                         "log": None, "tree": None}
    if t < 2:
        lh = (1, 2, 1, 3)[fmt]
        regen = int.from_bytes(s[pos:pos + lh], "little") >> (3 if lh == 1 else 4)
        csize = 1 if t == 1 else regen
        _need(pos + lh + csize <= end, "literals past the block")
        lits = (s[pos + lh:pos + lh + regen] if t == 0 else s[pos + lh:pos + lh + 1] * regen) if decode else None
    else:
        lh, bits = (3, 3, 4, 5)[fmt], (10, 10, 14, 18)[fmt]
        v = int.from_bytes(s[pos:pos + lh], "little")
        regen, csize = v >> 4 & ((1 << bits) - 1), v >> (4 + bits) & ((1 << bits) - 1)
        L["streams"] = 1 if fmt == 0 else 4
        _need(pos + lh + csize <= end and csize > 0, "literals past the block")
        at, lend = pos + lh, pos + lh + csize
        if t == 2:
            L["weights"] = "direct" if s[at] >= 128 else "fse"
            if decode:
                w, _, used = _read_weights(s, at, lend)
                st["huf"] = w
                L["tree"] = (bytes(s[at:at + used]), w)
                at += used
        elif decode:
            _need(st["huf"] is not None, "Treeless literals without a tree")
        lits = None
        if decode:
            codes, log = huffman_codes(st["huf"])
            L["log"] = log
            by_bits = {}
            for sym, (c, n) in codes.items():
                for fill in range(1 << (log - n)):
                    by_bits[format(c << (log - n) | fill, "0%db" % log)] = (sym, n)
            if L["streams"] == 1:
                bounds, counts = [at, lend], [regen]
            else:
                _need(lend - at >= 10 and regen >= 6, "four streams need a jump table")
                sizes = struct.unpack_from("<3H", s, at)
                bounds = [at + 6, at + 6 + sizes[0], at + 6 + sizes[0] + sizes[1], at + 6 + sum(sizes), lend]
                _need(bounds[3] < lend, "the jump table runs past the section")
                seg = (regen + 3) // 4
                counts = [seg, seg, seg, regen - 3 * seg]
            L["stream_sizes"] = [bounds[k + 1] - bounds[k] for k in range(len(counts))]
            lits = b"".join(_decode_stream(s, bounds[k], bounds[k + 1], by_bits, log, counts[k]) for k in range(len(counts)))
    _need(regen <= BLOCK_MAX, "more than 128 KiB of literals")
    L["regen"] = regen
    at = pos + lh + csize
    _need(at < end, "no sequences section")
    n, w = s[at], 1
    at += 1
    if n > 0x7f:
        w = 3 if n == 0xff else 2
        _need(at + w - 1 <= end, "a truncated sequence count")
        n = int.from_bytes(s[at:at + 2], "little") + 0x7f00 if w == 3 else (n - 0x80 << 8) + s[at]
        at += w - 1
    b.update(count_width=w, nseq=n, modes=None, logs=None, seqs=[], leftover=regen)
    if n == 0:
        _need(at == end, "bytes behind an empty sequences section")
        if decode:
            out += lits
        return
    _need(at < end and not s[at] & 3, "the modes byte")
    modes = [MODES[s[at] >> sh & 3] for sh in (6, 4, 2)]
    at += 1
    logs, norms = [], [None] * 3
    for t3, mode in enumerate(modes):
        if mode == PREDEFINED:
            st["tables"][t3] = (fse_table(*DEFAULT[t3]), DEFAULT[t3][1])
        elif mode == RLE:
            _need(at < end and s[at] <= MAX_SYM[t3], "an RLE symbol")
            st["tables"][t3] = ([(s[at], 0, 0)], 0)
            at += 1
        elif mode == FSE:
            norm, log, used = read_distribution(s, at, end, MAX_SYM[t3])
            _need(log <= MAX_LOG[t3], "an accuracy log over the limit")
            st["tables"][t3] = (fse_table(norm, log), log)
            norms[t3] = norm
            at += used
        else:
            _need(st["tables"][t3] is not None, "Repeat mode without a table")
        logs.append(st["tables"][t3][1])
    b["modes"], b["logs"], b["norms"] = tuple(modes), tuple(logs), tuple(norms)
    if not decode:
        return
    br = _Bits(s, at, end)
    tabs = [x[0] for x in st["tables"]]
    state = [br.take(logs[0]), br.take(logs[1]), br.take(logs[2])]
    lit_at, rep = 0, st["rep"]
    for i in range(n):
        lc, oc, mc = tabs[0][state[0]][0], tabs[1][state[1]][0], tabs[2][state[2]][0]
        value = (1 << oc) + br.take(oc)
        ml = ML_BASE[mc] + br.take(ML_BITS[mc])
        ll = LL_BASE[lc] + br.take(LL_BITS[lc])
        dist, rep = resolve(rep, value, ll)
        _need(ll <= regen - lit_at, "a literal length beyond the literals")
        out += lits[lit_at:lit_at + ll]
        lit_at += ll
        _need(dist != 0, "a repeat offset of 0")
        _need(dist <= len(out) - frame0, "an offset beyond the frame's output")
        if dist >= ml:
            out += out[len(out) - dist:len(out) - dist + ml]
        else:
            piece = bytes(out[len(out) - dist:])
            out += (piece * (ml // dist + 1))[:ml]
        b["seqs"].append((ll, ml, dist, oc, lc, mc))
        if i + 1 < n:
            for t3 in (0, 2, 1):
                _, nb, base = tabs[t3][state[t3]]
                state[t3] = base + br.take(nb)
    _need(br.left() == 0, "the sequence bitstream is not consumed exactly")
    st["rep"] = rep
    b["leftover"] = regen - lit_at
    out += lits[lit_at:]


def forms(parsed):
    """What a parsed stream shows, in the vocabulary of zstd_corpus.FEATURES, plus finer names: "format:<literals
    type>:<size format>", "count:<width>", "ll:<mode>", "of:<mode>", "ml:<mode>"."""
    out = set()
    for f in parsed.frames:
        if f["skippable"]:
            out.add("frame:skippable")
            continue
        out |= {"fcs:%d" % f["fcs"], "frame:single" if f["single"] else "frame:window"}
        if f["checksum"]:
            out.add("frame:checksum")
        for b in f["blocks"]:
            out.add("block:" + b["type"])
            if b["size"] == 0:
                out.add("block:empty")
            if b["type"] != "compressed":
                continue
            L = b["literals"]
            out |= {"literals:" + L["type"], "format:%s:%d" % (L["type"], L["size_format"]), "count:%d" % (b["count_width"] if b["nseq"] else 0)}
            if L["type"] in ("compressed", "treeless"):
                out.add("streams:%d" % L["streams"])
            if L["weights"]:
                out.add("weights:" + L["weights"])
            if b["nseq"] == 0:
                out.add("sequences:none")
            else:
                out |= {"mode:" + m for m in b["modes"]} | {"%s:%s" % (t, m) for t, m in zip(("ll", "of", "ml"), b["modes"])}
    return out


def loose(literals):
    """Does k_zstd decode these four streams in lock step (HufStreams::loose)? The rule, restated: codes of at
    most 11 bits, a last segment that is not empty (3 * seg < regen), every stream at least 8 bytes."""
    if literals["streams"] != 4:
        return False
    seg = (literals["regen"] + 3) // 4
    return literals["log"] <= 11 and 3 * seg < literals["regen"] and all(n >= 8 for n in literals["stream_sizes"])


# ---- a small steered corpus, and bodies that must be refused -----------------------------------------
def corpus():
    """[(name, stream, data)]: small streams that use every choice of the encoder, on text the parser cuts."""
    data, out = Z.text(5000, 9), []

    def add(name, blocks, **frame):
        fr, content = encode_frame(blocks, **frame)
        out.append(("steered/" + name, fr, content))
    base = parse(data[:2500], max_ml=12, cut_every=[1, 127, 128, 40])
    w = huffman_weights(data)
    add("predefined, raw literals", steer(base))
    one = [parse(data[k * 700:(k + 1) * 700], max_ml=12)[0] for k in range(4)]   # each refers to itself only
    seqs = [q for _, s in one for q in s]
    for streams in (1, 4):
        add("compressed literals, %d" % streams, steer(one, lit="compressed", streams=streams, weights=w))
    add("treeless", [("seq",) + one[1] + (dict(lit="compressed", streams=4, weights=w),), ("raw", b"in between"),
                     ("seq",) + one[2] + (dict(lit="treeless", streams=1),),
                     ("seq",) + one[3] + (dict(lit="treeless", streams=4, size_format=3),)], checksum=True)
    for logs in ((5, 5, 5), (9, 8, 9)):
        o = dict(ll=fitted(seqs, 0, logs[0], (35,), (35,)), of=fitted(seqs, 1, logs[1], (25,), (25,)), ml=fitted(seqs, 2, logs[2], (52,), (52,)))
        add("fse %d/%d/%d, then repeat" % logs, [("seq",) + one[1] + (o,), ("seq", b"no sequences", []),
                                                 ("seq",) + one[2] + (dict(ll=REPEAT, of=REPEAT, ml=REPEAT),)], fcs=4)
    same = [("seq", data[:3] + data[100:140], [(3, 7, 1), (3, 7, 2), (3, 7, 2)], dict(ll=RLE, of=RLE, ml=RLE)),
            ("seq", data[200:212], [(3, 7, 1), (3, 7, 2)], dict(ll=REPEAT, of=PREDEFINED, ml=REPEAT)),
            ("seq", b"z" * 40, [(3, 7, 1), (3, 7, REP1)], dict(lit="rle", of=(FSE, [1, 15, 16], 5))), ("rle", b"r", 300),
            ("seq", b"q" * 5000, [(0, 100, 250), (0, 3, REP2), (1, 3, REP3), (2, 3, REP1), (2, 9, REP2)], dict(lit="rle"))]
    add("rle tables, mixed modes, repeat codes", same, fcs=8, single=True)
    long = parse(data, max_ml=3, min_ll=0)
    add("short matches", steer(long, lit="compressed", streams=4, weights=w, ll=fitted([q for _, s in long for q in s], 0, 6),
                               ml=RLE), fcs=2, single=True)
    add("all sizes of raw and rle literals", [("seq", data[:n], [], dict(size_format=f)) for n, f in ((4, 0), (5, 0), (31, 1), (400, 3))] +
        [("seq", b"r" * n, [], dict(lit="rle", size_format=f)) for n, f in ((4, 0), (5, 0), (31, 1), (4000, 3))])
    return out


REFUSALS = ("rep[0] - 1 of 1", "treeless in a second frame's first block", "repeat mode in a second frame's first block",
            "offset one beyond the second frame's output", "literal length one beyond the literals")
# what the strict reader says of each: every body carries one fault
REASONS = dict(zip(REFUSALS, ("a repeat offset of 0", "Treeless literals without a tree", "Repeat mode without a table",
                              "an offset beyond the frame's output", "a literal length beyond the literals")))


def refused_bodies():
    """{kind: body}: two frames each; the first is good, the second holds one thing a bounds check must refuse. The
    Treeless and the Repeat block are their frame's first block, and would be good blocks under the first frame's
    tree and tables; the three others lie behind a Raw block, so that only the named bound refuses them."""
    text = Z.text(600, 4)
    w = huffman_weights(text)
    ctx = Context()
    first, _ = encode_frame([("seq", text[:200], [(150, 20, 100)], dict(lit="compressed", streams=1, weights=w,
                                                                        ll=fitted([(150, 3, 1)], 0, 6, pad=(0, 18)))),
                             ("raw", text[200:300])], ctx)
    alone = lambda body: Z.frame(Z.block(2, body, last=True), b"", fcs=0)
    second = lambda body: Z.frame(Z.block(0, text[300:340]) + Z.block(2, body, last=True), b"", fcs=0)
    return {
        REFUSALS[0]: first + second(encode_block(text[340:348], [(0, 4, REP3)])),
        REFUSALS[1]: first + alone(encode_block(text[340:400], [], ctx, lit="treeless")),
        REFUSALS[2]: first + alone(encode_block(text[340:400], [(20, 4, 10)], ctx, ll=REPEAT, of=REPEAT, ml=REPEAT)),
        REFUSALS[3]: first + second(encode_block(text[340:348], [(8, 4, 49)])),
        REFUSALS[4]: first + second(encode_block(text[340:348], [(9, 4, 10)])),
    }
