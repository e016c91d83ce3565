"""A steered DEFLATE writer and an independent reader, for the GZIP page tests (host and GPU).

The writer takes a list of blocks -- ("stored", bytes, final), ("fixed", tokens, final), ("dynamic", tokens,
lit_lengths, dist_lengths, options, final) -- and returns the raw stream of RFC 1951: fields LSB first, Huffman
codes most significant bit first. A token is a literal (an int), a match (length, distance) or (length,
distance, 284) for length 258 sent as symbol 284 with extra 31, ("sym", s) for a bare literal/length symbol, or
("bits", value, width) for bits put in as they are. Options of a dynamic block: hlit, hdist, hclen (larger than
needed), rle (the code-length symbols to send: 0..15, or (16 | 17 | 18, repeat count)), bad (send what was
asked for although no inflater may accept it).

limited_lengths() builds a length-limited code from frequencies; steered_lengths() puts chosen symbols at
chosen lengths and fills the code up with symbols nobody uses, so that it stays complete. tokenise() is a greedy
parser whose choices the caller steers. walk() reads a stream back following RFC 1951 alone (codes are read one
bit at a time against the canonical assignment of section 3.2.2; it shares nothing with deflate_fmt.h): every
form a test claims is asserted on what walk() reads from the bytes that are sent."""
import heapq
import struct

from tests import inflate_corpus as I

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
FULL = 1 << 15


class Malformed(Exception):
    pass


# ---- codes -----------------------------------------------------------------------------------------------
def kraft(lengths):
    """The code space the lengths take, in units of 2^-15: FULL for a complete code."""
    return sum(FULL >> l for l in lengths if l)


def canonical(lengths):
    """{symbol: (code, length)} by RFC 1951 3.2.2."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def limited_lengths(freqs, maxbits, n=None):
    """Code lengths (a list of n) of a Huffman code over the symbols with freqs[s] > 0, no longer than maxbits and
    complete. An alphabet of fewer than two symbols gets a second one, so that an inflater accepts the code."""
    n = len(freqs) if n is None else n
    used = [s for s in range(len(freqs)) if freqs[s] > 0]
    for s in range(n):
        if len(used) >= 2:
            break
        if s not in used:
            used.append(s)
    heap = [(max(freqs[s], 0) if s < len(freqs) else 0, s, (s,)) for s in used]
    heapq.heapify(heap)
    depth = dict.fromkeys(used, 0)
    while len(heap) > 1:
        fa, ka, a = heapq.heappop(heap)
        fb, kb, b = heapq.heappop(heap)
        for s in a + b:
            depth[s] += 1
        heapq.heappush(heap, (fa + fb, min(ka, kb), a + b))
    num = [0] * (maxbits + 1)
    for d in depth.values():
        num[min(d, maxbits)] += 1
    total = sum(num[i] << (maxbits - i) for i in range(1, maxbits + 1))
    while total > 1 << maxbits:      # move code space from the longest codes to a shorter one
        num[maxbits] -= 1
        for i in range(maxbits - 1, 0, -1):
            if num[i]:
                num[i] -= 1
                num[i + 1] += 2
                break
        total -= 1
    order = sorted(used, key=lambda s: (depth[s], -(freqs[s] if s < len(freqs) else 0), s))
    out, k = [0] * n, 0
    for length in range(1, maxbits + 1):
        for _ in range(num[length]):
            out[order[k]] = length
            k += 1
    assert kraft(out) == FULL
    return out


def steered_lengths(freqs, n, forced, maxbits=15, spare=None):
    """A complete code of n lengths in which forced = {symbol: length} holds: the other symbols in use share half of
    the code space by their frequencies (all of it when nothing is forced), the forced ones take theirs from the
    other half, and what is left goes to `spare` symbols (default: the unused ones, ascending) that no token names."""
    others = [s for s in range(len(freqs)) if freqs[s] > 0 and s not in forced]
    out = [0] * n
    if not forced:
        return limited_lengths(freqs, maxbits, n)
    if len(others) == 1:
        out[others[0]] = 1
    elif others:
        base = limited_lengths([freqs[s] if s in others else 0 for s in range(len(freqs))], maxbits - 1, n)
        for s in others:
            out[s] = base[s] + 1
    for s, l in forced.items():
        out[s] = l
    left = FULL - kraft(out)
    assert left >= 0, "the forced lengths do not fit"
    spare = [s for s in (range(n) if spare is None else spare) if out[s] == 0 and not (s < len(freqs) and freqs[s] > 0)]
    for l in range(1, 16):
        if left & (FULL >> l):
            assert spare, "no unused symbol is left to complete the code"
            out[spare.pop(0)] = l
            left -= FULL >> l
    assert kraft(out) == FULL
    return out


def length_symbol(length, via284=False):
    """(symbol, extra value, extra bits) of a match length."""
    assert 3 <= length <= 258
    if length == 258:
        return (284, 31, 5) if via284 else (285, 0, 0)
    k = max(i for i in range(28) if LEN_BASE[i] <= length)
    return 257 + k, length - LEN_BASE[k], LEN_EXTRA[k]


def distance_symbol(d):
    assert 1 <= d <= 32768
    k = max(i for i in range(30) if DIST_BASE[i] <= d)
    return k, d - DIST_BASE[k], DIST_EXTRA[k]


_LSYM = {l: length_symbol(l) for l in range(3, 259)}
_DSYM = {}


def _dsym(d):
    if d not in _DSYM:
        _DSYM[d] = distance_symbol(d)
    return _DSYM[d]


def frequencies(tokens):
    """(literal/length frequencies with symbol 256 counted once, distance frequencies) of a token list."""
    lit, dist = [0] * 286, [0] * 30
    lit[256] = 1
    for t in tokens:
        if isinstance(t, int):
            lit[t] += 1
        elif t[0] == "sym":
            lit[t[1]] += 1
        elif t[0] != "bits":
            lit[(284 if len(t) > 2 and t[2] == 284 else _LSYM[t[0]][0])] += 1
            dist[_dsym(t[1])[0]] += 1
    return lit, dist


def expand(tokens, history=b""):
    """What the tokens stand for, behind `history`."""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif t[0] not in ("sym", "bits"):
            length, d = t[0], t[1]
            assert 1 <= d <= len(out)
            if d >= length:
                out += out[len(out) - d:len(out) - d + length]
            else:
                for _ in range(length):
                    out.append(out[-d])
    return bytes(out[len(history):])


# ---- the writer ----------------------------------------------------------------------------------------------
class Out:
    def __init__(self):
        self.buf, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, w):
        assert 0 <= v < 1 << w
        self.acc |= v << self.n
        self.n += w
        while self.n >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c):
        v, w = c
        self.put(int(format(v, "0%db" % w)[::-1], 2), w)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bitpos(self):
        return 8 * len(self.buf) + self.n

    def done(self):
        self.align()
        return bytes(self.buf)


def _reversed(codes):
    return {s: (int(format(v, "0%db" % w)[::-1], 2), w) for s, (v, w) in codes.items()}


def _tokens_out(out, tokens, lit, dist):
    lit, dist = _reversed(lit), _reversed(dist)
    for t in tokens:
        if isinstance(t, int):
            out.put(*lit[t])
        elif t[0] == "sym":
            out.put(*lit[t[1]])
        elif t[0] == "bits":
            out.put(t[1], t[2])
        else:
            s, x, xb = length_symbol(258, True) if len(t) > 2 and t[2] == 284 else _LSYM[t[0]]
            out.put(*lit[s])
            if xb:
                out.put(x, xb)
            s, x, xb = _dsym(t[1])
            out.put(*dist[s])
            if xb:
                out.put(x, xb)
    if 256 in lit:
        out.put(*lit[256])


def plain_rle(seq):
    """The plain encoder of a run of code lengths: 18 and 17 for zeros, 16 for repeats of the length before."""
    out, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k))
                run -= k
            if run >= 3:
                out.append((17, run))
                run = 0
            out += [0] * run
        else:
            out.append(v)
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k))
                run -= k
            out += [v] * run
        i = j
    return out


def rle_expand(rle):
    seq = []
    for r in rle:
        if isinstance(r, int):
            seq.append(r)
        elif r[0] == 16:
            seq += [seq[-1] if seq else 0] * r[1]
        else:
            seq += [0] * r[1]
    return seq


def _dynamic_header(out, lit_lengths, dist_lengths, o):
    bad = o.get("bad", False)
    need_l = max([257] + [s + 1 for s, l in enumerate(lit_lengths) if l])
    need_d = max([1] + [s + 1 for s, l in enumerate(dist_lengths) if l])
    nlen = o["hlit"] + 257 if "hlit" in o else need_l
    ndist = o["hdist"] + 1 if "hdist" in o else need_d
    assert nlen >= need_l and ndist >= need_d
    lit = (list(lit_lengths) + [0] * nlen)[:nlen]
    dist = (list(dist_lengths) + [0] * ndist)[:ndist]
    if not bad:
        for name, lens in (("literal/length", lit), ("distance", dist)):
            k, used = kraft(lens), [l for l in lens if l]
            assert k <= FULL, "the %s code is over-subscribed" % name
            assert k == FULL or not used or used == [1], "the %s code is incomplete" % name
        assert lit[256] and nlen <= 286 and ndist <= 30
    rle = o.get("rle") or plain_rle(lit) + plain_rle(dist)
    assert bad or rle_expand(rle) == lit + dist, "the code-length symbols do not stand for the lengths"
    freq = [0] * 19
    for r in rle:
        freq[r if isinstance(r, int) else r[0]] += 1
    cl = o.get("cl_lengths") or limited_lengths(freq, 7)
    assert bad or kraft(cl) == FULL
    ncode = max([4] + [i + 1 for i, s in enumerate(CLEN_ORDER) if cl[s]])
    if "hclen" in o:
        assert o["hclen"] + 4 >= ncode
        ncode = o["hclen"] + 4
    out.put(nlen - 257, 5)
    out.put(ndist - 1, 5)
    out.put(ncode - 4, 4)
    for s in CLEN_ORDER[:ncode]:
        out.put(cl[s], 3)
    codes = canonical(cl)
    for r in rle:
        if isinstance(r, int):
            out.code(codes[r])
        else:
            out.code(codes[r[0]])
            base, width = {16: (3, 2), 17: (3, 3), 18: (11, 7)}[r[0]]
            out.put(r[1] - base, width)
    return lit, dist


def write(blocks, out=None):
    """The raw DEFLATE stream of the blocks (with `out`, an Out to go on with: the blocks are added to it)."""
    given, out = out is not None, Out() if out is None else out
    for b in blocks:
        final = b[-1]
        out.put(int(bool(final)), 1)
        if b[0] == "stored":
            assert len(b[1]) <= 65535
            out.put(0, 2)
            out.align()
            out.buf += struct.pack("<HH", len(b[1]), len(b[1]) ^ 0xffff) + b[1]
        elif b[0] == "fixed":
            out.put(1, 2)
            _tokens_out(out, b[1], canonical(FIXED_LIT), canonical(FIXED_DIST))
        else:
            _, tokens, lit_lengths, dist_lengths, o, _ = b
            out.put(2, 2)
            lit, dist = _dynamic_header(out, lit_lengths, dist_lengths, o)
            _tokens_out(out, tokens, canonical(lit), canonical(dist))
    return out if given else out.done()


def dynamic(tokens, final=False, lit_forced=None, dist_forced=None, maxbits=15, lit_spare=None, dist_spare=None, **options):
    """A dynamic block whose codes come from the tokens' frequencies, with forced = {symbol: length}."""
    lf, df = frequencies(tokens)
    lit = steered_lengths(lf, 286, lit_forced or {}, maxbits, lit_spare)
    dist = steered_lengths(df, 30, dist_forced or {}, maxbits, dist_spare) if any(df) or dist_forced else [0]
    return ("dynamic", tokens, lit, dist, options, final)


def member(blocks, data, **kw):
    """The gzip member of the blocks, which must stand for `data` (checked with zlib's raw inflate)."""
    raw = write(blocks)
    m = I.member(data, raw=raw, **kw)
    assert I.reference(m, len(data)) == data, "zlib does not read the steered member as its data"
    return m


# ---- the tokeniser ---------------------------------------------------------------------------------------------
def tokenise(data, distances=(), min_len=3, max_len=258, no_match_before=0, literals_only=False, far=True, forced=None,
             start=0, end=None):
    """Greedy tokens for data[start:end], which may reach back to data[0]. At every position the distances of
    `distances` are tried first, in order, then (far) the most recent earlier occurrence of the next three bytes; a
    match must be min_len..max_len long; none starts before `no_match_before`; forced = {position: (length,
    distance)} puts that match there. The tokens are checked to stand for the data."""
    end = len(data) if end is None else end
    forced = forced or {}
    tokens, last, i = [], {}, start
    if far and not literals_only:
        for p in range(max(0, start - 32768), start):
            last[data[p:p + 3]] = p
    while i < end:
        if i in forced:
            length, d = forced[i][:2]
            assert d <= i and i + length <= end and all(data[i + k] == data[i + k - d] for k in range(length)), (i, forced[i])
            tokens.append(tuple(forced[i]))
            i += length
            continue
        best = None
        if not literals_only and i >= no_match_before and i + min_len <= end:
            cand = [i - d for d in distances if 0 < d <= i]
            key = data[i:i + 3]
            if far and key in last and i - last[key] <= 32768:
                cand.append(last[key])
            cap = min(max_len, end - i)
            nxt = min((p for p in forced if p > i), default=end)
            cap = min(cap, nxt - i)
            for c in cand:
                n = 0
                while n < cap and data[c + n] == data[i + n]:
                    n += 1
                if n >= max(min_len, 3):
                    best = (n, i - c)
                    break
        if far:
            last[data[i:i + 3]] = i
        if best is None:
            tokens.append(data[i])
            i += 1
            continue
        tokens.append(best)
        if far:
            for p in range(i + 1, i + min(best[0], 16)):
                last[data[p:p + 3]] = p
        i += best[0]
    assert expand(tokens, data[:start]) == data[start:end], "the tokens do not stand for the data"
    return tokens


# ---- the walker ------------------------------------------------------------------------------------------------
class _In:
    def __init__(self, raw, bit):
        self.raw, self.bit, self.end = raw, bit, 8 * len(raw)

    def take(self, w):
        if self.bit + w > self.end:
            raise Malformed("the input ends inside a block")
        p = self.bit >> 3
        v = int.from_bytes(self.raw[p:p + 4], "little") >> (self.bit & 7) & ((1 << w) - 1)
        self.bit += w
        return v

    def symbol(self, table):
        """One symbol of a code: bits are taken one at a time, the code's most significant bit first."""
        code, p, raw = 0, self.bit, self.raw
        for length in range(1, 16):
            if p >= self.end:
                raise Malformed("the input ends inside a block")
            code = code << 1 | (raw[p >> 3] >> (p & 7) & 1)
            p += 1
            s = table.get((length, code))
            if s is not None:
                self.bit = p
                return s, length
        raise Malformed("a bit pattern without a symbol")


def _table(lengths, what, single_ok=True):
    k, used = kraft(lengths), [l for l in lengths if l]
    if k > FULL:
        raise Malformed("the %s code is over-subscribed" % what)
    if k < FULL and used and not (single_ok and used == [1]):
        raise Malformed("the %s code is incomplete" % what)
    return {(l, c): s for s, (c, l) in canonical(lengths).items()}


def walk(raw, bit=0, out=None):
    """(blocks, the bit position behind the final block's last bit, the output) of the raw stream that starts at bit
    position `bit` of `raw`. A block: kind ("stored" | "fixed" | "dynamic"), final, bit (of its header), data_bit (of
    its first symbol, or of a stored block's first byte), end_bit, out (output position of its first byte), n_out;
    a stored block's length; a dynamic block's hlit, hdist, hclen, cl_lengths, cl_syms ([(symbol, repeat or None)] as
    sent), lit_lengths, dist_lengths; a coded block's tokens: (literal or length, distance or 0, literal/length
    symbol, bits of its code, distance symbol, bits of its code, input bit position, output position), and eob_bits.
    `out` holds the output of what came before (an earlier member); a distance may not reach below the start."""
    rd = _In(raw, bit)
    out = bytearray() if out is None else out
    origin, blocks = len(out), []
    while True:
        b = {"bit": rd.bit, "final": rd.take(1), "out": len(out)}
        typ = rd.take(2)
        if typ == 3:
            raise Malformed("block type 3")
        if typ == 0:
            rd.bit = (rd.bit + 7) & ~7
            n, c = rd.take(16), rd.take(16)
            if n ^ 0xffff != c:
                raise Malformed("a stored block's lengths disagree")
            if rd.bit + 8 * n > rd.end:
                raise Malformed("the input ends inside a block")
            at = rd.bit >> 3
            out += raw[at:at + n]
            rd.bit += 8 * n
            b.update(kind="stored", length=n, data_bit=8 * at, tokens=[])
        else:
            if typ == 1:
                lit, dist = FIXED_LIT, FIXED_DIST
                b.update(kind="fixed")
            else:
                hlit, hdist, hclen = rd.take(5), rd.take(5), rd.take(4)
                if hlit > 29 or hdist > 29:
                    raise Malformed("too many length or distance symbols")
                cl = [0] * 19
                for s in CLEN_ORDER[:hclen + 4]:
                    cl[s] = rd.take(3)
                table = _table(cl, "code-length", single_ok=False)
                lens, sent = [], []
                while len(lens) < hlit + hdist + 258:
                    s, _ = rd.symbol(table)
                    if s < 16:
                        lens.append(s)
                        sent.append((s, None))
                        continue
                    if s == 16 and not lens:
                        raise Malformed("a repeat with no length before it")
                    rep = rd.take(2) + 3 if s == 16 else rd.take(3) + 3 if s == 17 else rd.take(7) + 11
                    sent.append((s, rep))
                    lens += [lens[-1] if s == 16 else 0] * rep
                if len(lens) > hlit + hdist + 258:
                    raise Malformed("a repeat runs past the lengths")
                lit, dist = lens[:hlit + 257], lens[hlit + 257:]
                if not lit[256]:
                    raise Malformed("no end-of-block code")
                b.update(kind="dynamic", hlit=hlit, hdist=hdist, hclen=hclen, cl_lengths=cl, cl_syms=sent,
                         lit_lengths=lit, dist_lengths=dist)
            lt, dt = _table(lit, "literal/length"), _table(dist, "distance")
            b["data_bit"] = rd.bit
            tokens = b["tokens"] = []
            while True:
                at = rd.bit
                s, w = rd.symbol(lt)
                if s < 256:
                    tokens.append((s, 0, s, w, None, 0, at, len(out)))
                    out.append(s)
                    continue
                if s == 256:
                    b["eob_bits"] = w
                    b["eob_bit"] = at
                    break
                if s > 285:
                    raise Malformed("length symbol %d" % s)
                length = LEN_BASE[s - 257] + rd.take(LEN_EXTRA[s - 257])
                ds, dw = rd.symbol(dt)
                if ds > 29:
                    raise Malformed("distance symbol %d" % ds)
                d = DIST_BASE[ds] + rd.take(DIST_EXTRA[ds])
                if d > len(out) - origin:
                    raise Malformed("a distance beyond the start")
                tokens.append((length, d, s, w, ds, dw, at, len(out)))
                p = len(out) - d
                if d >= length:
                    out += out[p:p + length]
                else:
                    for k in range(length):
                        out.append(out[p + k])
        b["end_bit"] = rd.bit
        b["n_out"] = len(out) - b["out"]
        blocks.append(b)
        if b["final"]:
            return blocks, rd.bit, out


def walk_body(body):
    """[(byte position of the member's raw stream, blocks, output position of its first byte, output length)] of a
    page body of gzip members, every bit position counted from the body's first byte, and the body's output."""
    members, pos, out = [], 0, bytearray()
    while pos < len(body):
        at = I._header_end(body, pos)
        if at is None:
            raise Malformed("not a gzip member")
        start = len(out)
        blocks, bit, out = walk(body, 8 * at, out)
        pos = (bit + 7) // 8 + 8
        if pos > len(body) or struct.unpack_from("<I", body, pos - 4)[0] != (len(out) - start) & 0xffffffff:
            raise Malformed("the trailer")
        members.append((at, blocks, start, len(out) - start))
    return members, bytes(out)


def matches(blocks):
    return [t for b in blocks for t in b["tokens"] if t[1]]


def literals(blocks):
    return [t for b in blocks for t in b["tokens"] if not t[1]]


# ---- the small corpus: one stream per form ---------------------------------------------------------------------
def demote(tokens, keep, history=b""):
    """The tokens (which follow `history`) with every match that keep(length, distance) turns down sent as literals."""
    out, res = bytearray(history[-32768:]), []
    for t in tokens:
        piece = expand([t], bytes(out[-32768:]))
        res += [t] if isinstance(t, int) or keep(t[0], t[1]) else list(piece)
        out += piece
    return res


def crossings(block):
    """{16 | 17 | 18} of the code-length symbols whose run starts in the literal/length lengths and ends in the
    distance lengths."""
    at, nlen, out = 0, block["hlit"] + 257, set()
    for s, rep in block["cl_syms"]:
        n = 1 if rep is None else rep
        if rep is not None and at < nlen < at + n:
            out.add(s)
        at += n
    return out


def _all_lengths():
    """Behind 300 'a': every length symbol at its smallest and its largest extra bits, and 258 both ways."""
    tokens = [97] * 300
    for k in range(29):
        tokens += [(LEN_BASE[k], 1), 97, (min(LEN_BASE[k] + (1 << LEN_EXTRA[k]) - 1, 258), 7), 97]
    return tokens + [(258, 1, 284), (258, 300)]


def _all_distances():
    """Behind 32,768 'b': every distance symbol at its smallest and its largest extra bits."""
    tokens = [98] * 32768
    for k in range(30):
        tokens += [(3, DIST_BASE[k]), (4, DIST_BASE[k] + (1 << DIST_EXTRA[k]) - 1)]
    return tokens


def _crossing(tokens, kind, final=True):
    """A dynamic block whose code-length symbols cross from the literal/length lengths into the distance lengths.
    Kind 16: the last three literal/length lengths and the first three distance lengths are 6, sent as one 6 and a 16
    of 5. Kind 18: HLIT 29 with nothing in use above symbol 264 and no distance below 5, the zeros of both sides sent
    as one 18."""
    lf, df = frequencies(tokens)
    if kind == 16:
        lit = steered_lengths(lf, 286, {283: 6, 284: 6, 285: 6})
        dist = steered_lengths(df, 30, {0: 6, 1: 6, 2: 6}, spare=range(29, 2, -1))
        dist = dist[:max(s for s in range(30) if dist[s]) + 1]
        seq = lit + dist
        rle = plain_rle(seq[:283]) + [6, (16, 5)] + plain_rle(seq[289:])
    else:
        assert not any(lf[265:]) and not any(df[:4]) and any(df)
        lit = steered_lengths(lf, 286, {})
        dist = steered_lengths(df, 30, {}) if sum(f > 0 for f in df) > 1 else [int(f > 0) for f in df]   # or a lone code
        dist = dist[:max(s for s in range(30) if dist[s]) + 1]
        z0 = max(s for s in range(286) if lit[s]) + 1
        z1 = min(s for s in range(len(dist)) if dist[s])
        assert 286 - z0 + z1 >= 11 and z1 > 0
        rle = plain_rle(lit[:z0]) + [(18, 286 - z0 + z1)] + plain_rle(dist[z1:])
    return ("dynamic", tokens, lit, dist, {"hlit": 29, "rle": rle}, final)


EMPTY_DYNAMIC = ("dynamic", [], [0] * 256 + [1], [0], {}, False)


def shift_to(bit, at=0):
    """Empty blocks (fixed ones of 10 bits, a dynamic one whose only code is symbol 256 at one bit) behind which a
    stream that stood at bit `at` of a byte stands at bit `bit` of one."""
    for fixed in range(4):
        for hclen in (None, 14, 15):
            cand = [("fixed", [], False)] * fixed
            if hclen:
                cand = cand + [EMPTY_DYNAMIC[:4] + ({"hclen": hclen},) + (False,)]
            o = Out()
            o.put(0, at)
            if write(cand, o).bitpos() % 8 == bit:
                return cand
    raise AssertionError("no empty blocks lead to bit %d" % bit)


def corpus():
    """[(name, raw stream, expected output)]: the form catalogue's streams, a few hundred bytes to a few KiB each
    (the stored block of 65,535 bytes aside)."""
    out = []

    def add(name, blocks, data=None):
        out.append((name, write(blocks), expand([t for b in blocks if b[0] != "stored" for t in b[1]]) if data is None else data))

    text = I.text(1500, 5)
    toks = tokenise(text)
    add("lengths", [dynamic(_all_lengths(), True)])
    add("lengths fixed", [("fixed", _all_lengths(), True)])
    add("distances", [dynamic(_all_distances(), True)])
    lf, df = frequencies(toks)
    rare = sorted((s for s in range(256) if lf[s]), key=lambda s: (lf[s], s))[:3]
    rared = sorted((s for s in range(30) if df[s]), key=lambda s: (df[s], s))[:3]
    assert len(rare) == 3 and len(rared) == 3
    add("slow codes", [dynamic(toks, True, lit_forced=dict(zip(rare, (10, 11, 15))), dist_forced=dict(zip(rared, (8, 9, 15))))])
    run = [120, (258, 1), (258, 1, 284), (100, 1), (3, 1)]
    add("lone distance code", [("dynamic", run, steered_lengths(frequencies(run)[0], 286, {}), [1], {}, True)])
    only = list(text[:400])
    add("literals only", [("dynamic", only, limited_lengths(frequencies(only)[0], 15), [0], {}, True)])
    add("empty dynamic", [EMPTY_DYNAMIC[:5] + (True,)])
    add("hlit 29 hdist 29", [dynamic([98] * 24600 + list(text[:200]) + [(258, 24577 + 150)], True)])
    add("hclen 15", [dynamic(toks, True, lit_forced={rare[0]: 15})])
    # 16 with 3 and 6, 17 with 3 and 10, 18 with 11 and 138, 16 repeating a zero: sixteen symbols of four bits
    rle = [4, (16, 3), (17, 3), 4, (16, 6), (17, 10), 0, (16, 3), (18, 11), 4, 4, 4, 4, (18, 138), (18, 75), 4]
    lit = rle_expand(rle)
    assert len(lit) == 257 and kraft(lit) == FULL
    add("code-length runs", [("dynamic", [s for s in range(256) if lit[s]], lit, [0], {"rle": rle + [0]}, True)])
    add("16 crosses", [_crossing(toks, 16)])
    add("18 crosses", [_crossing(demote(tokenise(text[:600], max_len=10), lambda n, d: d >= 5), 18)])
    high = "\u00e9\u20ac\u00ff".encode() * 3
    add("fixed 7 8 9 bits", [("fixed", list(b"ab" + high) + [(3, 2), (115, 4), (131, 1), (163, 1), (195, 1), (258, 1), (227, 1), (258, 3, 284)], True)])
    add("stored empty", [("stored", b"", False), ("fixed", list(b"xy"), False), ("stored", b"", True)], b"xy")
    big = I.text(65535, 9)
    add("stored 65535", [("stored", big, True)], big)
    for k in range(8):
        add("stored at bit %d" % k, shift_to(k) + [("stored", b"stored %d" % k, True)], b"stored %d" % k)
    return out


def two_members(extra=0):
    """(body, output): two members; the second one's only match reaches exactly its member's first byte (extra: that
    much further back, which no inflater may follow)."""
    a, b = b"first member", b"abcdefgh"
    second = write([("fixed", list(b) + [(8, 8 + extra)], True)])
    return I.member(a) + I.member(b + b, raw=second), a + b + b


REFUSALS = ["incomplete literal/length code", "over-subscribed distance code", "16 first", "repeat past the lengths",
            "no end-of-block code", "HLIT 30: a code for symbol 286", "unused pattern of a lone distance code",
            "distance past the member's start"]
_refused = {}


def refused_bodies(data, repaired=False):
    """{class: body}: a good member for the first part of `data`, then a member that stands for all of the rest and is
    refused for the one reason it is named for: a reader without that one check would find the right bytes, the right
    ISIZE and the page's length. repaired: the twin of each body with the fault taken out (the same blocks and tokens),
    which zlib accepts -- so the fault is the only reason. Where the fault sits in a header, it sits in an empty final
    block behind good blocks. Two classes cannot be read to the right bytes by any reader: no code ends a block whose
    symbol 256 has none, and the unused pattern names no distance; their twins differ in that one length and that one bit.
    The twin of the last class is the same block in one member with the first part, where its distance is in range."""
    key = (data, repaired)
    if key in _refused:
        return _refused[key]
    cut = max(len(data) // 2, len(data) - 4000)
    good, rest = I.member(data[:cut], level=9), data[cut:]
    lits = list(rest)
    lf = frequencies(lits)[0]
    ok = limited_lengths(lf, 15)
    body = ("dynamic", lits, ok, [0], {}, False)
    x = rest[0]
    zeros = plain_rle([0] * 253)
    blocks = {}
    two = [0] * 257
    two[x], two[256] = (1, 1) if repaired else (2, 2)
    blocks["incomplete literal/length code"] = [body, ("dynamic", [], two, [0], {"bad": True}, True)]
    blocks["over-subscribed distance code"] = [("dynamic", lits, ok, [1, 2, 2] if repaired else [1, 1, 1], {"bad": True}, True)]
    # read as a run of zeros, the 16 gives the lengths of the twin: symbol 256 alone, at one bit
    blocks["16 first"] = [body, ("dynamic", [], [0] * 256 + [1], [0], {"bad": True, "rle": [(17 if repaired else 16, 3)] + zeros + [1, 0]}, True)]
    # cut off at HLIT + HDIST lengths, the last run gives the twin's one distance length of 0
    blocks["repeat past the lengths"] = [body, ("dynamic", [], [0] * 256 + [1], [0],
                                                {"bad": True, "rle": plain_rle([0] * 256) + [1] + ([0] if repaired else [(17, 3)])}, True)]
    none = [0] * 257
    none[x], none[(x + 1) % 256], none[256] = (1, 0, 1) if repaired else (1, 1, 0)
    blocks["no end-of-block code"] = [body, ("dynamic", [], none, [0], {"bad": True}, True)]
    if repaired:
        blocks["HLIT 30: a code for symbol 286"] = [("dynamic", lits, steered_lengths(lf, 286, {285: 15}), [0], {}, True)]
    else:
        blocks["HLIT 30: a code for symbol 286"] = [("dynamic", lits, steered_lengths(lf + [0], 287, {286: 15}), [0],
                                                     {"bad": True, "hlit": 30}, True)]
    # the first match of three bytes a greedy parse finds, under a distance code of its one symbol: that code's bit is
    # sent as 1, the pattern without a symbol
    toks = tokenise(rest, max_len=3)
    k = next(k for k, t in enumerate(toks) if not isinstance(t, int))
    p, (sym, extra, width) = k, distance_symbol(toks[k][1])       # the tokens before the first match are literals
    one = lits[:p] + [("sym", 257), ("bits", int(not repaired), 1)] + ([("bits", extra, width)] if width else []) + lits[p + 3:]
    blocks["unused pattern of a lone distance code"] = [("dynamic", one, steered_lengths(frequencies(one)[0], 286, {}),
                                                         [0] * sym + [1], {}, True)]
    out = {k: good + I.member(rest, raw=write(b)) for k, b in blocks.items()}
    # a match that starts one byte before its member, which is cut where the page's bytes allow one: the bytes the
    # match stands for are the ones a reader of the whole page would copy from the end of the first member
    c, at = next((c, at) for c in range(cut, 0, -1) for at in [data.find(data[c - 1:c + 2], c + 3, c + 32000)] if at > 0)
    tail, p = list(data[c:]), at - c
    far = dynamic(tail[:p] + [(3, p + 1)] + tail[p + 3:], final=True)
    if repaired:
        out["distance past the member's start"] = I.member(data, raw=write([dynamic(tokenise(data[:c])), far]))
    else:
        out["distance past the member's start"] = I.member(data[:c], level=9) + I.member(data[c:], raw=write([far]))
    assert sorted(out) == sorted(REFUSALS)
    _refused[key] = out
    return out
