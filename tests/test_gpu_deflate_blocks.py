"""Steered DEFLATE blocks through k_inflate: the parts of RFC 1951 that zlib's compressor does not write (codes
longer than the lookup tables, a lone one-bit distance code, blocks without a distance code, the corners of the
dynamic header, length 258 as symbol 284) and the kernel's own machinery (why a round ends, the ring's wrap, the
window, stored copies), each on a body whose form is asserted with deflate_steer.walk_body() on the bytes that
are sent -- not assumed -- and, for the rounds, with a model of inflate_decode's round boundaries (_rounds).

The table is one (config 3 at scale 0.001, seed 3) whose add.stats is steered: its only page (DATA_PAGE_V2, PLAIN,
no dictionary, so the levels stay outside the body) holds a row with multi-byte UTF-8, a row of runs of period 2, 3,
63, 64 and 65 placed so that the period-2 run lies across output position INF_RING, a run of 98,400 'Z' (longer than
65,536 + 32,768), the stretch of 68,921 bytes without a repeated three-byte string, and a marker row that repeats at
distance exactly 32,768. Bodies go in with lz4_corpus.rewrite (codec 2), so their length is free; the bytes around a
steered member go into members zlib writes. The SNAPPY twin of the same table is the expectation: export(0),
export(1) and the state against the oracle. Bodies are shared between cases, and each is replayed once.

What the kernel's design decides about two of the cases: a round stages 4 KiB of input, so 16,384 literals end a
round by its span only where a literal costs under two bits -- the span case takes its literals from the 'Z' run
(one bit each), and the stretch, at five bits and more a literal, ends its rounds by the window; and since every
round stages its window where the round before stopped, a block header comes near a window's end only behind about
3.5 KiB of one block's symbols -- the small-blocks body holds blocks of that size next to its few hundred small ones.

A page's input phase is its body's file offset plus a constant (the file is copied to one device allocation, aligned
far beyond 16 bytes), so sixteen residues of the offsets are sixteen window phases (test_input_phases_and_tiny_members).
The output phase is the length of a page's level bytes mod 16, which the planner does not let a test choose: B is
not asserted.

Measured on an MI355X: the file's 30 cases take 11.6 s, 2.6 s of it the module's table; the slowest case (a page-sized
body's first replay, or the 4 KiB variant with its 130 re-written pages) 1.0 to 1.1 s, next to 0.95 to 1.05 s for the
slowest case of tests/test_gpu_gzip_pages.py in the same runs."""
import os
import re
import shutil
import zlib

import pytest

from tests import deflate_steer as T
from tests import inflate_corpus as I
from tests import lz4_corpus as L
from tests.test_gpu_parity import _assert_same
from tests.test_gpu_zstd_blocks import FILL, STRETCH, W, _random, build_base

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constant(name, source="k_inflate.hip"):
    src = open(os.path.join(ROOT, "delta_amd", "csrc", source)).read()
    return re.search(r"constexpr uint32_t %s = ([^;]+);" % name, src).group(1)


WIN, RING, SPAN, BATCH = (int(_constant(k)) for k in ("INF_WIN", "INF_RING", "INF_SPAN", "INF_BATCH"))
assert _constant("BLOCK_HEADER_MAX_BYTES", "deflate_fmt.h") == "(17 + 57 + MAX_LENS * 14 + 7) / 8 + 8"
HEADER_ROOM = (17 + 57 + 320 * 14 + 7) // 8 + 8 + 8     # what PH_BLOCK asks of the window
ZRUN = 98400
MARKER = '{"numRecords":0,"tags":"%s"}' % _random(300, 1)
UTF8 = '{"tags":"é€ÿ \U0001d11e ü中"}'
P2, P3 = "ab" * 300, ("xyz" * 101)[:301]
P63, P64, P65 = (_random(63, 163) * 6)[:300], (_random(64, 164) * 6)[:300], (_random(65, 165) * 6)[:301]
SEG = "ab" * 50
PERIODS_ROW = '{"tags":"%s"}' % "|".join((P2, P3, P63, P64, P65, SEG))
PAD = '{"numRecords":%07d,"tags":"f%s"}'


# ---- the steered table -------------------------------------------------------------------------------------------
def rows_of(n, shown):
    """{row: value}: see the module's docstring. shown[i]: the live state takes valid row i's stats from the checkpoint,
    so that export(0) shows what the decoder made of it; every steered row is such a row. Fillers are W bytes with their
    length prefix; a filler with a longer tag brings the next row to the byte it is meant for."""
    rows, at = {}, [0, 0]   # next row, its byte position in the page

    def put(text):
        rows[at[0]] = text
        at[0] += 1
        at[1] += 4 + len(text.encode())

    def put_shown(text):
        while not shown[at[0]]:
            put(FILL % at[0])
        put(text)

    def fill_to(target):
        """Fillers, then one padded filler, so that the next row starts at byte `target` and is a shown one."""
        last = max(i for i in range(at[0] + 1, at[0] + (target - at[1]) // W + 1) if shown[i])
        while at[0] < last - 1:
            put(FILL % at[0])
        assert target - at[1] >= W
        put(PAD % (at[0], "f" * (target - at[1] - W)))
        assert at[1] == target and shown[at[0]]

    put_shown(UTF8)
    fill_to(RING - 300 - 13)                      # the period-2 run: [RING - 300, RING + 300)
    put(PERIODS_ROW)
    put_shown('{"tags":"%s"}' % ("Z" * ZRUN))
    put_shown('{"tags":"%s"}' % STRETCH)
    put_shown(MARKER)
    m1 = at[1] - 4 - len(MARKER)
    fill_to(m1 + 32768)
    put(MARKER)
    assert at[0] < n - 1000 and sum(shown) > 100
    return rows


class Page:
    """The add.stats page's bytes and where the steered rows lie in them."""

    def __init__(self, data):
        self.D = D = data
        self.p2 = D.index(P2.encode())
        self.seg = D.index(b"|" + SEG.encode() + b'"}') + 1
        self.z = D.index(b"Z" * ZRUN)
        self.stretch = D.index(STRETCH.encode())
        self.stretch_end = self.stretch + len(STRETCH)
        self.m1 = D.index(MARKER.encode()) - 4
        self.m2 = self.m1 + 32768
        self.mlen = len(MARKER) + 4
        assert self.p2 == RING - 300 and D[self.z + ZRUN] != 90 and D[self.z - 1] != 90
        assert all(D[i] == D[i - 32768] for i in range(self.m2, self.m2 + self.mlen))
        assert max(D) >= 144 and len(D) > self.m2 + 40000

    def around(self, a, member, n):
        """The page with D[a:a + n] sent as `member` and the rest as members zlib writes."""
        body = (I.member(self.D[:a], level=1) if a else b"") + member + (I.member(self.D[a + n:], level=1) if a + n < len(self.D) else b"")
        assert I.reference(body, len(self.D)) == self.D, "zlib does not read the steered body as the page"
        return body


def _run(n, alternate=False):
    """Matches at distance 1 that stand for n bytes: 258 at a time, every other one as symbol 284."""
    out = [(258, 1, 284) if alternate and k % 2 else (258, 1) for k in range(n // 258)]
    return out + ([(n % 258, 1)] if n % 258 >= 3 else [90] * (n % 258))


def _lone(tokens, final=False):
    """A dynamic block whose distance code is symbol 0 alone, at one bit."""
    return ("dynamic", tokens, T.steered_lengths(T.frequencies(tokens)[0], 286, {}), [1], {}, final)


def _literal_block(data, final=False, bits=None):
    """A dynamic block of literals whose distance lengths are one 0; bits: every code in use that long."""
    lf = T.frequencies(list(data))[0]
    lens = T.limited_lengths(lf, 15) if bits is None else T.steered_lengths(lf, 286, {s: bits for s in range(257) if lf[s]})
    return ("dynamic", list(data), lens, [0], {}, final)


def _rare(freq, lengths):
    used = sorted((s for s in range(len(freq)) if freq[s] and s != 256), key=lambda s: (freq[s], s))
    assert len(used) >= len(lengths) + 2
    return dict(zip(used, lengths))


# ---- the bodies ------------------------------------------------------------------------------------------------------
def body_codes(P):
    """One member over the whole page: codes of 10, 11, 15 (literal/length) and 8, 9, 15 bits (distance) in use; the lone
    one-bit distance code under 258 sent both ways; distances 32,768 and 24,577 under HLIT 29 / HDIST 29; a literals-only
    block without a distance code; a 16 and an 18 that cross into the distance lengths; the marker copied from 32,768."""
    D = P.D
    a = P.z + 1
    t = T.tokenise(D, distances=(W, 2, 3, 63, 64, 65), end=a)
    lf, df = T.frequencies(t)
    blocks = [T.dynamic(t, lit_forced=_rare(lf[:256], (10, 11, 15)), dist_forced=_rare(df, (8, 9, 15)))]
    blocks.append(_lone(_run(128 * 258, alternate=True)))
    c = a + 128 * 258
    t = T.tokenise(D, start=c, end=P.stretch, distances=(1,), forced={c: (258, 32768), c + 258: (258, 24577), c + 516: (3, 32768)})
    blocks.append(T.dynamic(t, hlit=29, hdist=29))
    blocks.append(_literal_block(D[P.stretch:P.stretch_end]))
    blocks.append(T._crossing(T.tokenise(D, start=P.stretch_end, end=P.m2, distances=(W,)), 16, final=False))
    e = P.m2 + P.mlen
    blocks.append(T.dynamic(T.tokenise(D, start=P.m2, end=e, distances=(32768,), far=False)))
    g = e + 100 * W
    blocks.append(T._crossing(T.demote(T.tokenise(D, start=e, end=g, distances=(W,), max_len=10, far=False), lambda n, d: d >= 5, D[:e]), 18,
                              final=False))
    blocks.append(T.dynamic(T.tokenise(D, start=g, distances=(W,), far=False), final=True))
    return T.member(blocks, D)


def _rounds_end(P):
    return P.z + 1 + 3 * 1100 + 130 * 258 + 40000 + 63 * 258 + 129 + 258


def body_rounds(P):
    """One steered member from the page's start into the 'Z' run, the rest by zlib. The period row lies across
    INF_RING. In the run, each in a block of its own (a block's first symbol starts a round): 1,100 matches of length 3;
    130 matches of 258 at distance 1; 40,000 literals of one bit; 63 matches of 258, one of 129 and one of 258 at
    distance 32,768, which end a round at INF_SPAN - 1 + 258."""
    D = P.D
    a = P.z + 1
    t = T.tokenise(D, distances=(2, 3, 63, 64, 65, W), end=a, forced={P.seg: (100, P.seg - (RING - 40))})
    blocks = [T.dynamic(t), _lone([(3, 1)] * 1100), _lone(_run(130 * 258)), _literal_block(b"Z" * 40000),
              T.dynamic(_run(63 * 258) + [(129, 1), (258, 32768)], final=True)]
    end = _rounds_end(P)
    assert end < P.z + ZRUN
    return P.around(0, T.member(blocks, D[:end]), end)


def body_window(P):
    """zlib's member up to the stretch; then one member: the stretch with every literal at 15 bits; 330 dynamic blocks
    of 102 bytes each; six fixed blocks of 3,600 to 3,850 literals, behind each of which the next block's header
    stands within BLOCK_HEADER_MAX_BYTES + 8 of the window's end."""
    D, a = P.D, P.stretch
    local = D[a:]
    n = len(STRETCH)
    blocks = [_literal_block(local[:n], bits=15)]
    at = n + 2 + 3 * W
    blocks.append(T.dynamic(T.tokenise(local, start=n, end=at, far=False)))
    for _ in range(330):
        blocks.append(T.dynamic(T.tokenise(local, start=at, end=at + 3 * W, distances=(W,), max_len=8, far=False)))
        at += 3 * W
    for k in range(6):
        blocks.append(("fixed", list(local[at:at + 3600 + 50 * k]), False))
        at += 3600 + 50 * k
    blocks.append(T.dynamic(T.tokenise(local, start=at, end=at + W, distances=(W,), far=False), final=True))
    at += W
    return P.around(a, T.member(blocks, local[:at]), at)


def body_stored(P):
    """zlib's member up to 20 bytes before the 'Z' run; then one member: a stored block of 65,535 bytes; a block whose
    first symbol is a match at distance 32,768 (into the stored block); an empty stored block between two coded blocks;
    eight stored blocks whose headers start at bits 0 to 7 of a byte."""
    D, a = P.D, P.z - 20
    local = D[a:]
    blocks = [("stored", local[:65535], False)]
    at = 65535
    blocks.append(T.dynamic(T.tokenise(local, start=at, end=at + 1000, distances=(1,), far=False, forced={at: (258, 32768)})))
    at += 1000
    blocks.append(("stored", b"", False))
    blocks.append(_lone(_run(600)))
    at += 600
    blocks.append(("stored", b"", False))
    for k in range(8):
        blocks += T.shift_to(k) + [("stored", local[at:at + 40 + k], False)]
        at += 40 + k
    blocks.append(("fixed", [], True))
    assert at < 20 + ZRUN
    return P.around(a, T.member(blocks, local[:at]), at)


BODIES = {"codes": body_codes, "rounds": body_rounds, "window": body_window, "stored": body_stored}


# ---- the rounds of inflate_decode ---------------------------------------------------------------------------------
def _rounds(members, n_in, A=0):
    """A model of where inflate_decode's rounds end, for rounds that end by the batch, the span, a block's end or
    build, a stored copy or a member's end: [{reason, nent (matches queued), out (bytes produced), walked (input bytes,
    rounded up), start (output position), bit (input position), last (the last token)}]. `members`: walk_body()'s;
    A: the 16-byte phase of the body's address, which only a stored copy's length depends on.

    The window is not modelled. A round of symbols cannot end by it, whatever A, while it has walked less than
    INF_WIN - 48 bytes (16 for room(16), 16 for the phase, 8 for what the reader holds, 8 to spare); a block header
    read in a round needs walked < INF_WIN - 48 - (BLOCK_HEADER_MAX_BYTES + 8). Where a caller relies on a round's end,
    it asserts that bound on `walked`. A coded block's build and a stored copy end a round wherever the window stood,
    so the model is exact again from every block's first symbol."""
    out = []
    cur = {"bit": 8 * members[0][0], "out": 0, "nent": 0}

    def end(reason, bit, produced, last=None):
        out.append(dict(reason=reason, nent=cur["nent"], out=produced - cur["out"], walked=(bit - cur["bit"] + 7) // 8,
                        start=cur["out"], bit=cur["bit"], last=last))
        cur.update(bit=bit, out=produced, nent=0)

    end("header", 8 * members[0][0], 0)
    for mi, (_, blocks, _, _) in enumerate(members):
        produced = blocks[0]["out"]
        for b in blocks:
            produced = b["out"]
            if b["kind"] == "stored":
                at, left = b["data_bit"] >> 3, b["length"]
                while left:
                    vb = ((cur["bit"] >> 3) + A) & ~15
                    avail = n_in - at if vb + WIN >= n_in + A else max(vb + WIN - A - at, 0)
                    n = min(left, avail, max(SPAN - (produced - cur["out"]), 0))
                    at, produced, left = at + n, produced + n, left - n
                    end("copy", 8 * at, produced)
                continue
            end("build", b["data_bit"], produced)
            last = None
            for t in b["tokens"] + [None]:
                if cur["nent"] >= BATCH:
                    end("batch", t[6] if t else b["eob_bit"], produced, last)
                elif produced - cur["out"] >= SPAN:
                    end("span", t[6] if t else b["eob_bit"], produced, last)
                if t:
                    cur["nent"] += 1 if t[1] else 0
                    produced += t[0] if t[1] else 1
                    last = t
        bit = (blocks[-1]["end_bit"] + 7) // 8 * 8 + 64
        end("done" if mi == len(members) - 1 else "member", 8 * members[mi + 1][0] if mi + 1 < len(members) else bit, produced)
    return out


def _within(rounds, a, b):
    return [r for r in rounds if a <= r["start"] < b]


# ---- what each form must show ----------------------------------------------------------------------------------------
def _all(w):
    return [b for _, blocks, _, _ in w.members for b in blocks]


def _ring(w, what):
    """Matches of the walk around a multiple of INF_RING, whatever the arena slot's phase: written across [wrap - 16,
    wrap]; with a source that spans it; of period 2 or 3, longer than a wave, across it."""
    for t in T.matches(_all(w)):
        n, d, at = t[0], t[1], t[7]
        wrap = (at + n) // RING * RING
        if what == "written" and wrap and at < wrap - 16 and at + n > wrap:
            return True
        if what == "period" and wrap == RING and at < wrap - 16 and at + n > wrap and d in (2, 3) and n > 64:
            return True
        s = at - d
        if what == "source" and d >= 17 and s < RING - 16 and s + min(d, n) > RING:
            return True
    return False


def _batch_rounds(w, P):
    a = P.z + 1
    rs = _within(w.rounds(), a, a + 3300)
    full = [r for r in rs if r["reason"] == "batch"]
    b = [b for b in _all(w) if b["out"] == a][0]
    return len(b["tokens"]) > 2 * BATCH and all(t[0] == 3 and t[1] for t in b["tokens"]) and len(full) >= 2 and all(
        r["nent"] == BATCH and r["out"] == 3 * BATCH and r["walked"] < WIN - 48 for r in full)


def _span_rounds(w, P, which):
    a = P.z + 1 + 3300
    if which == "matches":      # 64 matches of 258: the span and one match's rest
        rs = [r for r in _within(w.rounds(), a, a + 130 * 258) if r["reason"] == "span"]
        return len(rs) >= 2 and all(r["out"] == 64 * 258 > SPAN and r["nent"] == 64 and r["last"][1] == 1 and r["walked"] < WIN - 48 for r in rs)
    a += 130 * 258
    if which == "literals":
        rs = [r for r in _within(w.rounds(), a, a + 40000) if r["reason"] == "span"]
        return len(rs) >= 2 and all(r["out"] == SPAN and r["nent"] == 0 and r["walked"] < WIN - 48 for r in rs)
    a += 40000
    rs = [r for r in _within(w.rounds(), a, a + 1) if r["reason"] == "span"]
    return len(rs) == 1 and rs[0]["out"] == SPAN - 1 + 258 and rs[0]["last"][:2] == (258, 32768) and rs[0]["walked"] < WIN - 48 and \
        rs[0]["nent"] == 65


def _window_rounds(w, P):
    """Every round the model gives the 15-bit block would walk more input than a window holds before its span or its
    batch is full: what ends them is room(16), several times over."""
    b = [b for b in _all(w) if b["out"] == P.stretch][0]
    rs = _within(w.rounds(), P.stretch, P.stretch_end)
    return {t[3] for t in b["tokens"]} == {15} and not T.matches([b]) and (b["end_bit"] - b["data_bit"]) // 8 > 4 * WIN and all(
        r["walked"] > WIN - 48 and r["nent"] < BATCH for r in rs if r["reason"] in ("span", "batch")) and len(rs) >= 4


def _small_blocks(w):
    return len([b for b in _all(w) if b["kind"] == "dynamic" and 12 <= len(b["tokens"]) <= 60]) >= 300


def _header_near_the_windows_end(w):
    """A block header within BLOCK_HEADER_MAX_BYTES + 8 of the end of the window that was staged where the round before
    stopped (at the block's first symbol), for every phase of the address, with the block before it inside the window."""
    blocks, found = _all(w), 0
    for prev, b in zip(blocks, blocks[1:]):
        if prev["kind"] == "stored" or prev["n_out"] >= SPAN or len(T.matches([prev])) >= BATCH or b["bit"] < prev["data_bit"]:
            continue
        rs, h = prev["data_bit"] >> 3, b["bit"] >> 3
        ends = [((rs + A) & ~15) + WIN - A for A in range(16)]
        found += all(e - HEADER_ROOM < h <= e - 24 for e in ends)
    return found >= 3


def _stored(w, P, what):
    blocks = _all(w)
    if what == "long":
        return any(b["kind"] == "stored" and b["length"] == 65535 > max(WIN, SPAN) for b in blocks) and all(
            len([r for r in w.rounds(A) if r["reason"] == "copy" and r["out"] > WIN - 16]) >= 15 for A in (0, 15))
    if what == "empty":
        return any(b["kind"] == "stored" and b["length"] == 0 and a["kind"] != "stored" and c["kind"] != "stored" and a["tokens"] and c["tokens"]
                   for a, b, c in zip(blocks, blocks[1:], blocks[2:]))
    if what == "read":
        return any(a["kind"] == "stored" and b["tokens"] and b["tokens"][0][1] == 32768 and a["out"] <= b["out"] - 32768 < b["out"]
                   for a, b in zip(blocks, blocks[1:]))
    return {b["bit"] % 8 for b in blocks if b["kind"] == "stored" and 40 <= b["length"] < 48} == set(range(8))


def _codes(w, what):
    blocks = _all(w)
    m, lits = T.matches(blocks), T.literals(blocks)
    if what == "slow":
        return {10, 11, 15} <= {t[3] for t in lits} and {8, 9, 15} <= {t[5] for t in m}
    if what == "lone":
        return any(b["kind"] == "dynamic" and b["dist_lengths"] == [1] and {284, 285} <= {t[2] for t in b["tokens"] if t[0] == 258}
                   for b in blocks)
    if what == "literals only":
        return any(b["kind"] == "dynamic" and b["dist_lengths"] == [0] and len(b["tokens"]) == len(STRETCH) for b in blocks)
    if what == "far":
        return {(29, 32768), (29, 24577)} <= {(t[4], t[1]) for t in m} and any(b["kind"] == "dynamic" and b["hlit"] == 29 and b["hdist"] == 29
                                                                               for b in blocks)
    return {16, 18} <= {s for b in blocks if b["kind"] == "dynamic" for s in T.crossings(b)}


FORMS = {
    "codes beyond both lookup tables": ("codes", lambda w, P: _codes(w, "slow")),
    "the lone one-bit distance code, 258 both ways": ("codes", lambda w, P: _codes(w, "lone")),
    "a literals-only block without a distance code": ("codes", lambda w, P: _codes(w, "literals only")),
    "distances 32,768 and 24,577, HLIT 29, HDIST 29": ("codes", lambda w, P: _codes(w, "far")),
    "repeats that cross into the distance lengths": ("codes", lambda w, P: _codes(w, "crossings")),
    "a match written across a ring wrap (codes)": ("codes", lambda w, P: _ring(w, "written")),
    "rounds end at INF_BATCH matches": ("rounds", _batch_rounds),
    "rounds end at INF_SPAN literals": ("rounds", lambda w, P: _span_rounds(w, P, "literals")),
    "rounds end past the span with one match": ("rounds", lambda w, P: _span_rounds(w, P, "matches")),
    "a round ends at INF_SPAN - 1 + 258 at distance 32,768": ("rounds", lambda w, P: _span_rounds(w, P, "far")),
    "a match written across INF_RING": ("rounds", lambda w, P: _ring(w, "written")),
    "a match whose source spans INF_RING": ("rounds", lambda w, P: _ring(w, "source")),
    "period 2 or 3 longer than a wave across INF_RING": ("rounds", lambda w, P: _ring(w, "period")),
    "rounds end by the window": ("window", _window_rounds),
    "a few hundred small blocks": ("window", lambda w, P: _small_blocks(w)),
    "a block header near the window's end": ("window", lambda w, P: _header_near_the_windows_end(w)),
    "a stored block longer than the window and the span": ("stored", lambda w, P: _stored(w, P, "long")),
    "an empty stored block between coded blocks": ("stored", lambda w, P: _stored(w, P, "empty")),
    "a match at 32,768 into a stored block": ("stored", lambda w, P: _stored(w, P, "read")),
    "stored headers at bits 0 to 7": ("stored", lambda w, P: _stored(w, P, "bits")),
}


class Walked:
    def __init__(self, body):
        self.body = body
        self.members, self.data = T.walk_body(body)
        self._rounds = {}

    def rounds(self, A=0):
        if A not in self._rounds:
            self._rounds[A] = _rounds(self.members, len(self.body), A)
        return self._rounds[A]


_walked = {}


def walked_body(P, name):
    if name not in _walked:
        w = Walked(BODIES[name](P))
        assert w.data == P.D
        _walked[name] = w
    return _walked[name]


# ---- the fixtures ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    from delta_amd.delta_log import Engine
    return Engine.get(0)


def gzip_variant(base, d, page_size=1 << 20):
    """A copy of the twin's log with the checkpoint as GZIP, DATA_PAGE_V2; (log path, checkpoint path)."""
    import pyarrow.parquet as pq
    lp = os.path.join(str(d), "_delta_log")
    shutil.copytree(base[0], lp)
    kw = {"write_batch_size": 32} if page_size < 65536 else {}
    pq.write_table(base[2], os.path.join(lp, base[1]), compression="gzip", compression_level=1, use_dictionary=False, version="1.0",
                   data_page_version="2.0", data_page_size=page_size, write_statistics=False, **kw)
    return lp, os.path.join(lp, base[1])


def page_of(ck):
    pages = I.gzip_pages(ck, "add.stats")
    assert len(pages) == 1
    at, c, u = pages[0]
    data = zlib.decompress(open(ck, "rb").read()[at:at + c], 31)
    assert len(data) == u
    return Page(data)


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    return build_base(str(tmp_path_factory.mktemp("db_base")), rows_of)


@pytest.fixture(scope="module")
def good(base, tmp_path_factory):
    lp, ck = gzip_variant(base, tmp_path_factory.mktemp("db_good"))
    return lp, ck, page_of(ck)


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
        stats = [a.get("stats") or "" for a in live]
        assert sum(STRETCH in s for s in stats) == 1 and sum(s == MARKER for s in stats) == 2
        assert sum("Z" * ZRUN in s for s in stats) == 1 and PERIODS_ROW in stats and UTF8 in stats
        return live, st.export(1)
    finally:
        st.release()


def _replay_file(engine, base, twin, lp):
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


def _replay_body(engine, base, good, twin, tmp, bodies):
    lp = os.path.join(str(tmp), "_delta_log")
    shutil.copytree(good[0], lp)
    L.rewrite(good[1], os.path.join(lp, base[1]), {k: (2, b) for k, b in bodies.items()})
    _replay_file(engine, base, twin, lp)


@pytest.fixture(scope="module")
def replayed(engine, base, good, twin, tmp_path_factory):
    """replayed(name): the table with that body is replayed once; what that raised is raised again for every form that
    shares the body."""
    results = {}

    def get(name):
        if name not in results:
            try:
                _replay_body(engine, base, good, twin, tmp_path_factory.mktemp("db_body"), {("add.stats", 0): walked_body(good[2], name).body})
                results[name] = None
            except Exception as e:   # kept for the forms that follow
                results[name] = e
        if results[name] is not None:
            raise results[name]
    return get


@pytest.mark.parametrize("form", sorted(FORMS))
def test_form(good, replayed, form):
    """The body shows the form (asserted on its bytes and on the model of the rounds), and the table with that body
    replays as the twin."""
    name, shows = FORMS[form]
    assert shows(walked_body(good[2], name), good[2]), form
    replayed(name)


def test_every_body_has_a_form():
    assert {name for name, _ in FORMS.values()} == set(BODIES)


# ---- input phases and tiny members -------------------------------------------------------------------------------------
TINY = (1, 15, 16, 17)


def phased_body(k, data):
    """Page k of add.path: members whose output is 1, 15, 16 and 17 bytes (each ends a round, so each is flushed on its
    own: the head, the tail and one whole line), then the rest in a member written here; the first member's header has
    a FEXTRA field of k mod 16 bytes."""
    body, at = b"", 0
    for j, n in enumerate(TINY):
        if at + n > len(data) - 20:
            break
        kw = {"flags": I.FEXTRA, "extra": b"\0" * (k % 16)} if j == 0 else {}
        body += T.member([("fixed", list(data[at:at + n]), True)], data[at:at + n], **kw)
        at += n
    rest = data[at:]
    body += T.member([T.dynamic(T.tokenise(rest), final=True)], rest, **({} if at else {"flags": I.FEXTRA, "extra": b"\0" * (k % 16)}))
    assert I.reference(body, len(data)) == data
    return body


def phased_file(good4k, out):
    """Writes `out`: the 4 KiB variant with every add.path page re-written by phased_body; the pages' new offsets."""
    def body_of(leaf, k, codec, body, usize):
        if leaf != "add.path" or usize == 0:
            return None
        return phased_body(k, zlib.decompress(body, 31))
    L.rewrite(good4k, out, body_of=body_of)
    return I.gzip_pages(out, "add.path")


def test_input_phases_and_tiny_members(engine, base, twin, tmp_path):
    """The body's address on the device is its file offset plus a constant, so the sixteen residues asserted here are
    sixteen phases of the window (A in k_inflate)."""
    lp, ck = gzip_variant(base, tmp_path, page_size=4096)
    pages = phased_file(ck, ck)
    assert len(pages) > 100 and {at % 16 for at, c, u in pages if c} == set(range(16))
    buf = open(ck, "rb").read()
    sizes = {m[3] for at, c, u in pages[:8] for m in T.walk_body(buf[at:at + c])[0]}
    assert set(TINY) <= sizes
    _replay_file(engine, base, twin, lp)


# ---- refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", T.REFUSALS)
def test_refusals(engine, base, good, twin, tmp_path, kind):
    """Handled error returns: each body stands for the whole page apart from its one fault (its repaired twin is accepted),
    and is refused by zlib and by the host program under the sanitizers in tests/test_deflate_steer.py first; on the device it ends in DR_E_PARQUET naming the column, and a good table replays
    afterwards on the same engine."""
    from delta_amd.delta_log import DeltaError
    at, c, u = I.gzip_pages(good[1], "add.path")[0]
    data = zlib.decompress(open(good[1], "rb").read()[at:at + c], 31)
    body = T.refused_bodies(data)[kind]
    assert I.reference(body, len(data)) is None
    lp = os.path.join(str(tmp_path), "_delta_log")
    shutil.copytree(good[0], lp)
    L.rewrite(good[1], os.path.join(lp, base[1]), {("add.path", 0): (2, body)})
    with pytest.raises(DeltaError) as e:
        staged = engine.stage_log(lp)
        try:
            staged.replay(base[3]).release()
        finally:
            staged.release()
    assert e.value.code == "DR_E_PARQUET" and "gzip page in add.path" in str(e.value), str(e.value)
    _replay_file(engine, base, twin, good[0])
