"""Folded punctuation in the K1 line walker (delta_amd/csrc/json_lane.h), host build.

A ':' or ',' is not a token of its own: it rides as a flag on the token before it, which the
tokenizer holds back by one token until the next token or the line end; the DFA applies the flag
after the token's own transition. These cases aim at what that can get wrong: punctuation with no
token to ride on, the held-back token across window, flush and line ends, tokens whose length no
longer fits the (narrower) aux field, and every way of misplacing a ':' or ','.

Every line goes through the General walker (must equal Python's json plus the unwrap rules of
tests/test_json_lane.py), the Fast walker (equal to General in every field unless it defers the line
as `hard`), and the bulk kernel's two-phase walk restated on the host (tokens into a bounded buffer
that is flushed through the DFA) at the kernel's slots and at 32, which must equal the Fast walker
and never write past its buffer. That walk (jf_parse_buffered, tests/native/json_fold_host.cpp) is
a copy of walk_line's flush loop in k_json.hip for one lane, not the loop itself: its slots and
flush mark are read from k_json.hip's defaults below, but only tests/test_gpu_json_fold.py runs the
kernel's own loop (on the same lines: `fold_corpus()` is shared with it, and the library built with
the LDS index checks reports a token written past the buffer).
"""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

from tests.test_json_lane import K_ADD, K_ERROR, K_REMOVE, expected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "json_fold_host.cpp")
HDR = os.path.join(ROOT, "delta_amd", "csrc", "json_lane.h")
LIB = os.path.join(ROOT, "build", "libjsonfold_host.so")

TOK_MAX_AUX = 1023      # json_lane.h: longest string body / scalar in one T_STRING / T_SCALAR token
TOK_MAX_SCALAR = 4095   # json_lane.h: a longer scalar run is an error row (unchanged by the folding)
TF_COLON, TF_COMMA = 0x10, 0x20
T_COLON, T_COMMA, T_STR_OPEN, T_SCALAR_LONG = 4, 5, 6, 13


def _kernel_buffer():
    """(slots per lane, slots kept free behind the flush mark): the defaults of k_json.hip."""
    src = open(os.path.join(ROOT, "delta_amd", "csrc", "k_json.hip")).read()
    cap = int(re.search(r"^#define DR_JL_TOKCAP (\d+)", src, re.M).group(1))
    margin = int(re.search(r"^#define DR_JL_FLUSH \(DR_JL_TOKCAP - (\d+)\)", src, re.M).group(1))
    return cap, margin


TOKCAP, FLUSH_MARGIN = _kernel_buffer()
# (slots per lane, flush mark): the kernel's, and the 32-slot variant of DESIGN.md 4g
BUFFERS = [(TOKCAP, TOKCAP - FLUSH_MARGIN), (32, 32 - FLUSH_MARGIN)]

ADD = (b'{"add":{"path":"part-00000-3f6a.c000.snappy.parquet","partitionValues":{"k":"v"},"size":1234,'
       b'"modificationTime":1700000000000,"dataChange":true,"stats":"{\\"numRecords\\":10}"}}')
REMOVE = (b'{"remove":{"path":"part-00001-9b1c.c000.snappy.parquet","deletionTimestamp":1700000000001,'
          b'"dataChange":true,"extendedFileMetadata":true,"partitionValues":{"k":"v"},"size":99}}')


@pytest.fixture(scope="module")
def lib():
    stale = not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR))
    if stale:
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", LIB, SRC])
    L = C.CDLL(LIB)
    L.jf_parse.restype = C.c_int
    L.jf_tokens.restype = C.c_int
    L.jf_parse_buffered.restype = C.c_int
    return L


def _out():
    return (C.c_ubyte(), C.c_ubyte(), C.c_uint(), C.c_uint(), C.c_longlong(), C.c_longlong())


def raw_walk(lib, line, align, general):
    """(hard, kind, flags, path_off, path_len, size, delts)"""
    o = _out()
    hard = lib.jf_parse(line, len(line), align, int(general), *[C.byref(x) for x in o])
    return (hard,) + tuple(x.value for x in o)


def raw_buffered(lib, line, align, cap, flush):
    o = _out()
    nf = C.c_int()
    hard = lib.jf_parse_buffered(line, len(line), align, cap, flush, *[C.byref(x) for x in o], C.byref(nf))
    return (hard,) + tuple(x.value for x in o), nf.value


def tokens(lib, line, align=0, general=True):
    cap = len(line) + 8
    buf = (C.c_uint * cap)()
    n = lib.jf_tokens(line, len(line), align, int(general), buf, cap)
    return None if n < 0 else list(buf[:n])


def counts(toks):
    """(tokens, tokens if every folded ':' / ',' were one of its own)"""
    folded = sum(1 for t in toks if (t & 15) != T_SCALAR_LONG and (t & 0x30))
    return len(toks), len(toks) + folded


def view(line, raw):
    """A raw result as tests/test_json_lane.py's walk() renders it."""
    import json
    hard, kind, flags, po, pl, size, delts = raw
    out = {"kind": kind}
    if kind in (K_ADD, K_REMOVE):
        if flags & 8:
            path = None
        else:
            body = line[po:po + pl]
            path = json.loads(b'"' + body + b'"') if flags & 4 else body.decode("utf-8")
        out.update(path=path, size=size, delts=delts if flags & 1 else None)
    return out


def check(lib, line, align, stats, exp=None):
    exp = expected(line) if exp is None else exp
    gen = raw_walk(lib, line, align, True)
    assert gen[0] == 0 and view(line, gen) == exp, ("general", line, align, gen, exp)
    fast = raw_walk(lib, line, align, False)
    if fast[0]:
        stats["hard"] = stats.get("hard", 0) + 1
    else:
        assert fast == gen, ("fast", line, align, fast, gen)
    for cap, flush in BUFFERS:
        buf, nflush = raw_buffered(lib, line, align, cap, flush)
        assert buf[0] >= 0, ("token buffer overrun", cap, line, align)
        assert buf[0] == fast[0] and (fast[0] or buf == fast), ("buffered", cap, line, align, buf, fast)
        stats["flush%d" % cap] = max(stats.get("flush%d" % cap, 0), nflush)
    stats[exp["kind"]] = stats.get(exp["kind"], 0) + 1


# ---- the corpus ----------------------------------------------------------------------------------------
PUNCT_ERRORS = [b'{"a" "b"}', b'{"a"::1}', b'{"a":,}', b'{"a":1,}', b'{,}', b'[1,,2]', b'[1,]', b'[,1]', b'[1:2]',
                b'{"a":1 "b":2}', b'[1 2]', b'{"a":1},', b':{}', b',{}', b'{"a":1}:']
PUNCT_VALID = [b'{"a":"b"}', b'{"a":1}', b'{"a":1,"b":2}', b'[1,2]', b'{}', b'[]', b'{"a":[1,{"b":2}],"c":null}']


def punct_cases():
    out = []
    for s in PUNCT_ERRORS + PUNCT_VALID:
        out.append(s)                                                       # the line itself
        out.append(b'{"add":' + s + b'}')                                   # its members at depth 2
        out.append(b'{"remove":' + s + b'}')
        out.append((b'{"add":{"path":"p",' + s[1:] + b'}') if s[:1] == b"{" else b'{"add":{"path":"p","t":' + s + b'}}')
        out.append(b'{"add":{"path":"p","partitionValues":' + s + b',"size":1}}')     # at depth 3
        out.append(b'{"remove":{"partitionValues":' + s + b',"path":"q","deletionTimestamp":5}}')
    return out


def structurals(line):
    """Offsets of the bytes of `line` outside strings that are one of {}[]:, (a byte-wise restatement)."""
    out, in_str, i = [], False, 0
    while i < len(line):
        c = line[i]
        if in_str:
            if c == 0x5C:
                i += 1
            elif c == 0x22:
                in_str = False
        elif c == 0x22:
            in_str = True
        elif c in b"{}[]:,":
            out.append(i)
        i += 1
    return out


def boundaries(line):
    """Offsets between two tokens of `line`: before and after every structural byte and string."""
    out, in_str, i = {0, len(line)}, False, 0
    while i < len(line):
        c = line[i]
        if in_str:
            if c == 0x5C:
                i += 1
            elif c == 0x22:
                in_str = False
                out.add(i + 1)
        elif c == 0x22:
            in_str = True
            out.add(i)
        elif c in b"{}[]:,":
            out.update((i, i + 1))
        i += 1
    return sorted(out)


def whitespace_cases():
    out = []
    for base in (ADD, REMOVE, b'{"a":[1,"x",{"b":null},[]],"txn":{"appId":"a","version":3}}'):
        pos = [i for i in structurals(base) if base[i] in b":,"]
        for ws in (b" ", b"\t", b"\r", b"  ", b" \t\r "):
            for before, after in ((1, 0), (0, 1), (1, 1)):
                b = bytearray(base)
                for i in reversed(pos):
                    b[i:i + 1] = ws * before + bytes([base[i]]) + ws * after
                out.append(bytes(b))
        # whitespace around every token, not only the punctuation
        b = bytearray(base)
        for i in reversed(boundaries(base)):
            b[i:i] = b" "
        out.append(bytes(b))
    return out


def window_cases():
    """':' and ',' at byte 15 and byte 16 of the line (the last byte of a 16-byte window and the first
    of the next when the line starts a window), the window's rest filled with whitespace after the
    value, under a prefix of 0..31 spaces (with the caller's alignments: every window phase)."""
    base = [b'{"' + b"k" * 12 + b'":1,"b":2}', b'{"' + b"k" * 13 + b'":1,"b":2}',          # ':' at 15 / 16
            b'{"a":' + b"1234567890" + b',"b":2}', b'{"a":' + b"12345678901" + b',"b":2}',  # ',' at 15 / 16
            b'{"a":1' + b" " * 9 + b',"b":2}', b'{"a":1' + b" " * 10 + b',"b":2}',          # spaces, then ','
            b'{"a"' + b" " * 11 + b':1}', b'{"a"' + b" " * 12 + b':1}',                     # spaces, then ':'
            b'{"a":"' + b"s" * 8 + b'","b":[]}', b'{"a":"' + b"s" * 9 + b'","b":[]}',       # ',' after a string
            b'{"a":{"b":{"c":1}},"d":2}', b'{"add":{"path":"p"},"x":[[1],[2]] ,"y":1}']
    for b in base[:4]:
        assert b.index(b":" if b"kk" in b else b",") in (15, 16)
    return [b" " * pre + b for pre in range(32) for b in base]


def buffer_cases():
    """Lines of every token count around the token buffer's slots and flush marks, counted with and
    without the folding: members (three tokens each before folding, two after), array elements (two
    before, one after) and brackets (never folded onto by a writer's line)."""
    out = []
    for m in range(0, 46):
        mem = b",".join(b'"k%d":"v"' % i for i in range(m))
        out.append(b'{"add":{"path":"p","size":1,"tags":{' + mem + b'}}}')
        out.append(b'{"remove":{"path":"q","x":[' + b",".join(b"%d" % i for i in range(m)) + b'],"deletionTimestamp":7}}')
        out.append(b'{"x":' + b"[" * (m // 2) + b"]" * (m // 2) + b',"add":{"path":"r' + b"%d" % m + b'"}}')
        out.append(b'{"add":{"path":"p","size":1,"tags":{' + mem + b'},}}')   # a dangling ',' after the last batch
    return out


def overrun_lines(mark):
    """Lines that fill the token buffer to its last slot when the flush mark is `mark`, written for a
    line that starts a 16-byte window: mark + 1 brackets (mark tokens in the buffer, one held back) and
    a scalar in the last byte of their window, so the window ends with exactly `mark` tokens and no
    flush; then the most a window can add:
      a) the carried scalar and 16 brackets, the line ending there (17 tokens + the one held back);
      b) a long string (open / close pair) closing at byte 0, 14 brackets and a scalar left open at the
         line end (16 + 2);
      c) the carried scalar, 15 brackets and a string left open at the line end (16 + 2)."""
    head = b"[" * (mark + 1)
    carried = head + b" " * (15 - len(head) % 16) + b"1"
    body = 1024 + (-(len(head) + 1 + 1024)) % 16  # the closing quote at byte 0 of its window
    return [carried + b"[" * 16,
            head + b'"' + b"s" * body + b'"' + b"[" * 14 + b"1",
            carried + b"[" * 15 + b'"']


def overrun_cases(mark=TOKCAP - FLUSH_MARGIN):
    """overrun_lines under a prefix of 0..15 spaces, one of which starts the brackets on a window
    whatever the line's alignment. In a commit every case is followed by a blank line that rounds the
    pair to whole windows (so the alignment is the same for every prefix) and stands between 64 lines
    of `{}`: the kernel flushes a wave's 64 lanes together, and a wave of this case and 63 lines that
    never reach the flush mark leaves the case's own token count to decide."""
    out = [b"{}"] * 64
    for line in overrun_lines(mark):
        for pre in range(16):
            case = b" " * pre + line
            out.append(case)
            out.append(b" " * ((-(len(case) + 2)) % 16))
            out += [b"{}"] * 64
    return out


def long_cases():
    out = []
    lens = [TOK_MAX_AUX - 1, TOK_MAX_AUX, TOK_MAX_AUX + 1, TOK_MAX_AUX + 2, 4095, 4096]
    for n in lens:
        body = b"s" * n
        esc = b'\\"' + b"e" * (n - 2)          # the same body length with an escaped quote in it
        for s in (body, esc):
            out.append(b'{"add":{"path":"' + s + b'","size":3}}')                        # a long value, then ','
            out.append(b'{"add":{"size":3,"path":"' + s + b'"}}')                        # then '}'
            out.append(b'{"add":{"path":"p","partitionValues":{"' + s + b'":"v"},"size":4}}')  # a long key, then ':'
            out.append(b'{"' + s + b'":1,"remove":{"path":"v"}}')                        # at depth 1 (escaped: General)
            out.append(b'{"add":{"path":"' + s + b'" "size":3}}')                        # no ',' after it
            out.append(b'{"add":{"path":"p","partitionValues":{"' + s + b'" "v"}}}')     # no ':' after it
            out.append(b'{"add":{"path":"' + s + b'",,"size":3}}')
    for n in [TOK_MAX_AUX - 1, TOK_MAX_AUX, TOK_MAX_AUX + 1, TOK_MAX_AUX + 2, TOK_MAX_SCALAR - 1, TOK_MAX_SCALAR]:
        for sc in (b"1" * n, b"1." + b"5" * (n - 2), b"-" + b"7" * (n - 1), b"x" * n):
            out.append(b'{"a":' + sc + b',"add":{"path":"p"}}')      # then ','
            out.append(b'{"add":{"path":"p"},"a":' + sc + b'}')      # then '}'
            out.append(b'{"a":[' + sc + b',' + sc[:9] + b']}')
            out.append(b'{"a":' + sc + b',,"b":1}')                  # a second ',' after it
            out.append(b'{"a":' + sc + b':1}')
            out.append(b'{"add":{"path":"p","size":' + sc + b'}}')   # not a long
            out.append(b'{"a":' + sc)                                # runs to the line end
    return out


def end_cases():
    out = [b"", b" ", b"{", b"}", b":", b",", b'"', b'"a"', b'"a":', b'"a",', b"1", b"1,", b"1:", b"{}", b"{},", b"[1],"]
    for base in (ADD, REMOVE):
        out += [base[:k] for k in range(1, len(base))]          # every truncation
        out += [base + t for t in (b",", b":", b" ", b"}", b"x", b'"', b",{}")]
    return out


def _mutations(line):
    """Every single misplacement of a ':' or ',' in `line`."""
    out = []
    for i in structurals(line):
        if line[i] in b":,":
            out.append(line[:i] + line[i + 1:])                                      # deleted
            out.append(line[:i] + line[i:i + 1] + line[i:])                          # doubled
            out.append(line[:i] + (b"," if line[i] == 0x3A else b":") + line[i + 1:])  # swapped
    for i in boundaries(line):
        out.append(line[:i] + b":" + line[i:])
        out.append(line[:i] + b"," + line[i:])
    return out


def mutation_cases(n_random=3000, seed=0xF01D):
    rng = random.Random(seed)
    out = []
    for base in (ADD, REMOVE):
        out += _mutations(base)
    while len(out) < n_random:  # two to four misplacements at once
        line = rng.choice((ADD, REMOVE))
        for _ in range(rng.randint(2, 4)):
            ms = _mutations(line)
            line = ms[rng.randrange(len(ms))]
        out.append(line)
    return out


def fold_corpus():
    return (punct_cases() + whitespace_cases() + window_cases() + buffer_cases() + long_cases() + end_cases() +
            mutation_cases() + overrun_cases())


# ---- the tests -----------------------------------------------------------------------------------------
def test_writer_lines_fold_to_fewer_tokens(lib):
    """The token counts DESIGN.md §4g quotes: a writer's add line is 33 tokens with stand-alone
    punctuation and 20 with it folded; no stand-alone ':' or ',' is left in a writer's line."""
    for line, before, after in ((ADD, 33, 20), (REMOVE, 33, 20)):
        toks = tokens(lib, line)
        assert counts(toks) == (after, before), counts(toks)
        assert not [t for t in toks if (t & 15) in (T_COLON, T_COMMA)]
        assert toks == tokens(lib, line, general=False)


def test_punctuation_grammar(lib):
    stats = {}
    for line in punct_cases():
        for align in (0, 5, 15):
            check(lib, line, align, stats)
    for line in PUNCT_ERRORS:
        assert expected(line)["kind"] == K_ERROR
        assert expected(b'{"add":' + line + b'}')["kind"] == K_ERROR
    assert stats.get("hard", 0) == 0 and stats[K_ERROR] > 200 and stats[K_ADD] > 10, stats


def test_whitespace_around_punctuation(lib):
    stats = {}
    cases = whitespace_cases()
    for line in cases:
        for align in (0, 7, 15):
            check(lib, line, align, stats)
    # tab / CR lines are the General walker's; the others fold exactly like the writer's line
    assert stats.get(K_ERROR, 0) == 0 and 0 < stats["hard"] < 3 * len(cases), stats
    for base in (ADD, REMOVE):
        want = [t & 0x3F for t in tokens(lib, base)]
        pos = [i for i in structurals(base) if base[i] in b":,"]
        b = bytearray(base)
        for i in reversed(pos):
            b[i:i + 1] = b" \t" + bytes([base[i]]) + b"\r "
        assert [t & 0x3F for t in tokens(lib, bytes(b))] == want


def test_punctuation_at_window_boundaries(lib):
    stats = {}
    for line in window_cases():
        for align in range(16):
            check(lib, line, align, stats)
    assert stats.get("hard", 0) == 0 and stats.get(K_ERROR, 0) == 0, stats


def test_token_buffer_boundaries(lib):
    stats = {}
    seen_after, seen_before = set(), set()
    for line in buffer_cases():
        toks = tokens(lib, line)
        a, b = counts(toks)
        seen_after.add(a)
        seen_before.add(b)
        for align in range(16):
            check(lib, line, align, stats)
    need = {39, 40, 41} | {c + d for c, _ in BUFFERS for d in (-1, 0, 1)} | {f + d for _, f in BUFFERS for d in (0, 1, 2)}
    slots = {c + d for c, _ in BUFFERS for d in (-1, 0, 1)}
    assert need <= seen_after and slots <= seen_before, (sorted(seen_after), sorted(seen_before))
    assert stats["flush40"] >= 3 and stats["flush32"] >= 4, stats  # lines that cross several flushes
    assert stats.get("hard", 0) == 0, stats


def test_a_window_fills_the_token_buffer_to_its_last_slot(lib):
    """The flush mark is tight: a line whose window ends with exactly `flush` tokens in the buffer and
    is followed by the most a window can add (overrun_lines) fits at the kernel's mark, and the same
    construction for a mark one higher writes past the buffer."""
    for cap, flush in BUFFERS:
        for align in range(16):
            pre = b" " * ((-align) % 16)
            for k, line in enumerate(overrun_lines(flush)):
                fast = raw_walk(lib, pre + line, align, False)
                assert fast[:2] == (0, K_ERROR) and expected(pre + line)["kind"] == K_ERROR
                buf, nflush = raw_buffered(lib, pre + line, align, cap, flush)
                assert buf == fast and nflush == 1, (cap, flush, align, k, buf, nflush)
                # one slot fewer does not hold it: every slot was used
                assert raw_buffered(lib, pre + line, align, cap - 1, flush)[0][0] == -1, (cap, flush, align, k)
            for k, line in enumerate(overrun_lines(flush + 1)):
                assert raw_buffered(lib, pre + line, align, cap, flush + 1)[0][0] == -1, (cap, flush, align, k)
                buf, nflush = raw_buffered(lib, pre + line, align, cap, flush)
                assert buf[0] == 0 and buf[1] == K_ERROR and nflush == 2, (cap, flush, align, k, buf, nflush)
    stats = {}
    cases = overrun_cases()
    for n, line in enumerate(cases):
        check(lib, line, n % 16, stats)
    assert stats[K_ERROR] == 48 and stats.get("hard", 0) == 0, stats
    # in a commit, every case starts at the same alignment
    at, starts = 0, set()
    for line in cases:
        if line.lstrip(b" ").startswith(b"["):
            starts.add((at + len(line) - len(line.lstrip(b" "))) % 16)
        at += len(line) + 1
    assert len(starts) == 16, sorted(starts)


def test_long_strings_and_scalars(lib):
    stats = {}
    for line in long_cases():
        check(lib, line, len(line) % 16, stats)
    assert stats[K_ADD] > 20 and stats[K_REMOVE] > 5 and stats[K_ERROR] > 50 and stats["hard"] > 0, stats
    # the token shapes on both sides of the aux limit
    for n, nt in ((TOK_MAX_AUX, 1), (TOK_MAX_AUX + 1, 2)):
        toks = tokens(lib, b'{"' + b"k" * n + b'":"' + b"v" * n + b'","b":1}')
        assert counts(toks)[0] == 2 + 2 * nt + 2, counts(toks)
        key, val = toks[nt], toks[2 * nt]
        assert key & TF_COLON and val & TF_COMMA, (hex(key), hex(val))
        assert ((toks[1] & 15) == T_STR_OPEN) == (nt == 2)
    for n in (TOK_MAX_AUX, TOK_MAX_AUX + 1, TOK_MAX_SCALAR):
        toks = tokens(lib, b'{"a":' + b"1" * n + b',"b":1}')
        long = n > TOK_MAX_AUX
        assert ((toks[2] & 15) == T_SCALAR_LONG) == long and ((toks[3] & 15) == T_COMMA) == long
        if long:
            assert (toks[2] >> 4) & 0xFFF == n
    # a scalar run past TOK_MAX_SCALAR stays what it was before the folding: an error row
    for sc in (b"1" * (TOK_MAX_SCALAR + 1), b"1." + b"5" * TOK_MAX_SCALAR):
        line = b'{"a":' + sc + b',"add":{"path":"p"}}'
        for general in (False, True):
            assert raw_walk(lib, line, 3, general)[:2] == (0, K_ERROR)


def test_line_ends(lib):
    stats = {}
    for line in end_cases():
        for align in (0, 9):
            check(lib, line, align, stats)
    assert stats.get("hard", 0) == 0 and stats[K_ERROR] > 500 and stats[0] >= 4, stats


def test_misplaced_punctuation_sweep(lib):
    stats = {}
    cases = mutation_cases()
    assert len(cases) >= 3000
    rng = random.Random(0xA11)
    for line in cases:
        check(lib, line, rng.randrange(16), stats)
    assert stats.get("hard", 0) == 0, stats
    # nearly every misplacement is an error row; the few that are not land inside a string
    assert stats[K_ERROR] > len(cases) // 2 and stats.get(K_ADD, 0) > 0 and stats.get(K_REMOVE, 0) > 0, stats


def over_the_line_limit_cases():
    """Lines over TOK_MAX_LINE (65535 bytes), which only the General walker takes: a token's offset field has 16
    bits, so every member here lies behind a string that pushes it past offset 65535, or past 2 * 65536 -- the
    keys the walker must match (path, size, deletionTimestamp), their values, a null among the tags, an escaped
    path, a scalar the grammar refuses."""
    out = []
    for pad in (65525, 65536, 2 * 65536 + 100, 3 * 65536 - 40):
        s = b'"' + b"s" * pad + b'"'
        out += [b'{"add":{"stats":' + s + b',"tags":{"u":null}}}',
                b'{"add":{"stats":' + s + b',"path":"late/p\\u0041th","size":9007199254740993,"tags":{"t":"x","u":null}}}',
                b'{"add":{"path":"early","stats":' + s + b',"partitionValues":{"p":null},"size":-5,"path":"last wins"}}',
                b'{"remove":{"tags":{"k":' + s + b'},"path":"r","deletionTimestamp":1700000000001,"size":12}}',
                b'{"commitInfo":{"x":' + s + b'},"remove":{"path":"r2","deletionTimestamp":null}}',
                b'{"add":{"stats":' + s + b',"size":1.5}}',
                b'{"add":{"stats":' + s + b',"tags":{"u":nul}}}',
                b'{"metaData":{"id":' + s + b',"x":[null,true,false,{"y":null}]}}',
                b' ' * pad + b'{"add":{"path":"behind blanks","size":3,"tags":{"u":null}}}']
    return out


def test_lines_over_the_token_offset_limit(lib):
    stats = {}
    for line in over_the_line_limit_cases():
        assert len(line) > 65535
        for align in (0, 7):
            check(lib, line, align, stats)
    assert stats["hard"] == 2 * len(over_the_line_limit_cases())      # every one is the General walker's
    assert stats[K_ADD] and stats[K_REMOVE] and stats[K_ERROR]
