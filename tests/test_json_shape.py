"""The writer-shape matcher of the K1 line walker (match_writer_line, delta_amd/csrc/json_lane.h), host build.

The bulk kernel decides a writer-serialised add / remove line from its token column without stepping
the DFA; whatever the matcher does not recognise it declines, and the DFA decides the line as before.
So the one property that matters is

    accept  =>  every LineOut field equals the General walker's, whose kind is add or remove

checked here for every line at each of the 16 alignments (tests/native/json_shape_host.cpp tokenizes
the line with the fast tokenizer into a strided buffer, runs the matcher over it and, independently,
parse_line_general). Coverage conditions keep the property from holding vacuously: unmutated writer
lines are accepted, and of the seeded mutations at least a tenth is accepted and three tenths declined.
The same source with its own main() runs under AddressSanitizer + UBSan as a child process.
"""
import ctypes as C
import glob
import os
import random
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import test_json_fold as F
from tests import test_json_lane as JL
from tests.test_json_lane import K_ADD, K_REMOVE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "json_shape_host.cpp")
HDR = os.path.join(ROOT, "delta_amd", "csrc", "json_lane.h")
LIB = os.path.join(ROOT, "build", "libjsonshape_host.so")
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def lib():
    stale = not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR))
    if stale:
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", LIB, SRC])
    L = C.CDLL(LIB)
    L.js_check.restype = C.c_int
    return L


_R7 = C.c_longlong * 7


def check(lib, line, stats=None, aligns=range(16)):
    """The property at each alignment; returns whether the line was accepted (the same at all)."""
    acc = set()
    for align in aligns:
        m, g = _R7(), _R7()
        a = lib.js_check(line, len(line), align, m, g)
        if a:
            assert list(m) == list(g) and g[0] in (K_ADD, K_REMOVE), (line, align, list(m), list(g))
        acc.add(a)
    assert len(acc) == 1, ("acceptance depends on the alignment", line)
    a = acc.pop()
    if stats is not None:
        stats["accepted" if a else "declined"] = stats.get("accepted" if a else "declined", 0) + 1
    return bool(a)


# ---- writer lines ---------------------------------------------------------------------------------------
_PV = re.compile(rb'"partitionValues":\{[^}]*\}')


def writer_lines(ncols, n=12, seed=7):
    """(adds, removes) as the synth writers emit them, with `ncols` partition columns (0 and 1 by
    rewriting the two-column object; the fourth of four is null for about one line in a hundred, so
    one is forced)."""
    from delta_amd.testing import synth as S
    pool = S.FilePool(np.random.default_rng(seed), n, 4 if ncols == 4 else 2)
    if ncols == 4:
        pool.p2null[0] = True
    adds = [S.add_line(pool, i, 1700000000000 + i).encode() for i in range(n)]
    rms = [S.remove_line(pool, i, 1700000001000 + i).encode() for i in range(n)]
    if ncols < 2:
        pv = b'"partitionValues":{}' if ncols == 0 else b'"partitionValues":{"p0":"2020-03-01"}'
        adds = [_PV.sub(pv, x, count=1) for x in adds]
        rms = [_PV.sub(pv, x, count=1) for x in rms]
    return adds, rms


def golden_lines():
    out = []
    for fn in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ref", "**", "_delta_log", "*.json"), recursive=True)):
        with open(fn, "rb") as f:
            out += f.read().split(b"\n")
    return out


def members(line):
    """(head, [member bytes], tail) of the line's file object, split at its top-level commas."""
    head = line.index(b":{") + 2
    tail = len(line) - 2
    assert line[tail:] == b"}}"
    body, out, depth, in_str, start, i = line[head:tail], [], 0, False, 0, 0
    while i < len(body):
        c = body[i]
        if in_str:
            if c == 0x5C:
                i += 1
            elif c == 0x22:
                in_str = False
        elif c == 0x22:
            in_str = True
        elif c in b"{[":
            depth += 1
        elif c in b"}]":
            depth -= 1
        elif c == 0x2C and depth == 0:
            out.append(body[start:i])
            start = i + 1
        i += 1
    out.append(body[start:])
    return line[:head], out, line[tail:]


def _join(head, mem, tail):
    return head + b",".join(mem) + tail


LETTERS = b"abcdefghijklmnopqrstuvwxyz"


def mutate(rng, line):
    """One single-byte or single-token change of a writer's line."""
    op = rng.randrange(11)
    head, mem, tail = members(line)
    b = bytearray(line)
    if op == 0:                                   # a byte deleted
        del b[rng.randrange(len(b))]
    elif op == 1:                                 # a byte doubled
        i = rng.randrange(len(b))
        b.insert(i, b[i])
    elif op == 2:                                 # two members swapped
        i, j = rng.sample(range(len(mem)), 2)
        mem[i], mem[j] = mem[j], mem[i]
        return _join(head, mem, tail)
    elif op == 3:                                 # a member twice
        i = rng.randrange(len(mem))
        mem.insert(rng.randrange(len(mem) + 1), mem[i])
        return _join(head, mem, tail)
    elif op == 4:                                 # a member dropped
        del mem[rng.randrange(len(mem))]
        return _join(head, mem, tail)
    elif op == 5:                                 # a letter of a member name changed
        i = rng.randrange(len(mem))
        k = rng.randrange(1, mem[i].index(b'":'))
        m = bytearray(mem[i])
        m[k] = rng.choice(LETTERS)
        mem[i] = bytes(m)
        return _join(head, mem, tail)
    elif op == 6:                                 # a digit becomes a letter
        at = [i for i, c in enumerate(b) if 0x30 <= c <= 0x39]
        b[rng.choice(at)] = rng.choice(b"ex" + LETTERS)
    elif op == 7:                                 # a quote removed
        at = [i for i, c in enumerate(b) if c == 0x22]
        del b[rng.choice(at)]
    elif op == 8:                                 # a value becomes null / a null becomes a string
        i = rng.randrange(len(mem))
        k = mem[i].index(b'":') + 2
        mem[i] = mem[i][:k] + (b'"x"' if mem[i][k:] == b"null" else b"null")
        return _join(head, mem, tail)
    elif op == 9:                                 # a letter inside the path or the stats (the shape stays)
        at = [i for i, c in enumerate(b) if c in LETTERS and i > line.index(b'"path":"') + 8]
        b[rng.choice(at)] = rng.choice(LETTERS + b"0123456789 /=%")
    else:                                         # a structural byte replaced
        at = [i for i, c in enumerate(b) if c in b'{}[]:,"\\']
        b[rng.choice(at)] = rng.choice(b'{}[]:,"\\ \t')
    return bytes(b)


def mutated_lines(count, seed):
    rng = random.Random(seed)
    base = [x for nc in (0, 1, 2, 4) for side in writer_lines(nc, n=6) for x in side]
    out = []
    while len(out) < count:
        m = mutate(rng, rng.choice(base))
        if b"\n" not in m:
            out.append(m)
    return out


# ---- the property ---------------------------------------------------------------------------------------
def test_golden_logs(lib):
    stats = {}
    lines = golden_lines()
    for line in lines:
        check(lib, line, stats)
    # every reference add matches, and every remove but delta-0.1.0's, which have no deletionTimestamp
    files = [x for x in lines if x.startswith(b'{"add"') or (x.startswith(b'{"remove"') and b'"deletionTimestamp"' in x)]
    old = [x for x in lines if x.startswith(b'{"remove"') and b'"deletionTimestamp"' not in x]
    assert len(files) >= 15 and len(old) == 4 and stats["accepted"] == len(files), (stats, len(files))


def test_existing_corpora(lib):
    """The fold and lane corpora (punctuation, whitespace, window, buffer, long-string, line-end and
    mutation cases): what the matcher accepts of them equals the general walk."""
    stats = {}
    for line in F.fold_corpus() + JL.corpus():
        check(lib, line, stats)
    assert stats["declined"] > stats["accepted"] > 20, stats


@pytest.mark.parametrize("ncols", [0, 1, 2, 4])
def test_synth_writer_lines_are_accepted(lib, ncols):
    adds, rms = writer_lines(ncols)
    for line in adds + rms:
        # every unmutated writer line matches (the bulk kernel's wave flushes a line of more than 22
        # tokens before the matcher sees it; the matcher itself takes any number of columns)
        assert check(lib, line), line
    m, g = _R7(), _R7()
    assert lib.js_check(rms[0], len(rms[0]), 3, m, g) == 1 and m[0] == K_REMOVE and m[1] & 1 and m[6] == 1700000001000
    assert lib.js_check(adds[0], len(adds[0]), 3, m, g) == 1 and m[0] == K_ADD and m[1] == 0 and m[5] > 0
    if ncols == 4:
        assert b'"p2":null' in adds[0]


def test_mutations(lib):
    stats = {}
    lines = mutated_lines(20000, 0x5A4E)
    for line in lines:
        check(lib, line, stats)
    n = len(lines)
    assert n >= 20000 and stats["accepted"] * 10 >= n and stats["declined"] * 10 >= 3 * n, stats


ADD2 = (b'{"add":{"path":"p0=2020-01-05/p1=7/part-00001-aa.c000.snappy.parquet","partitionValues":{"p0":"2020-01-05",'
        b'"p1":"7"},"size":1234,"modificationTime":1700000000000,"dataChange":true,"stats":"{\\"numRecords\\":3}"}}')
RM2 = (b'{"remove":{"path":"p0=2020-01-05/p1=7/part-00001-aa.c000.snappy.parquet","deletionTimestamp":1700000000001,'
       b'"dataChange":true,"extendedFileMetadata":true,"partitionValues":{"p0":"2020-01-05","p1":"7"},"size":99}}')


def named_cases():
    """(line, accepted or None): None where either is right; the property holds for all of them."""
    sz = lambda v: ADD2.replace(b'"size":1234', b'"size":' + v)
    return [
        (ADD2, True), (RM2, True),
        (ADD2.replace(b'"path":"p0=2020-01-05/p1=7/part-00001-aa.c000.snappy.parquet"', b'"path":null'), False),
        (ADD2.replace(b'"path"', b'"p\\u0061th"'), False),
        (ADD2.replace(b'"size":1234', b'"size":1234,"size":5'), False),
        (ADD2.replace(b',"modificationTime"', b',"size":5,"modificationTime"'), False),
        (sz(b'"12"'), False), (sz(b"1.0"), False), (sz(b"1e3"), False), (sz(b"9223372036854775808"), False),
        (sz(b"9223372036854775807"), True), (sz(b"null"), None), (sz(b"01"), False),
        (RM2.replace(b'"deletionTimestamp":1700000000001,', b""), False),
        (RM2.replace(b"1700000000001", b"null"), None),
        (ADD2[:-1] + b',"remove":' + RM2[len(b'{"remove":'):-1] + b"}", False),
        (ADD2[:-1] + b',"commitInfo":{"operation":"WRITE"}}', False),
        (b'{"commitInfo":{"operation":"WRITE"},' + ADD2[1:], False),
        (ADD2.replace(b'{\\"numRecords\\":3}', b"s" * 1100), False),   # a string token pair (open / close)
        (ADD2 + b" ", None), (ADD2 + b"\r", False), (b" " + ADD2, None), (ADD2.replace(b'"size":', b'"size": '), None),
        (ADD2.replace(b'{"p0":"2020-01-05","p1":"7"}', b"{}"), True),
        (ADD2.replace(b'"p1":"7"', b'"p1":null'), True), (ADD2.replace(b'"p1":"7"', b'"p1":7'), False),
        (ADD2.replace(b'"p1":"7"}', b'"p1":"7",}'), False), (ADD2.replace(b'"p1":"7"', b'"p\\u0031":"7"'), False),
        (ADD2.replace(b',"stats":"{\\"numRecords\\":3}"', b""), True),
        (ADD2.replace(b',"stats"', b',"tags":{"a":"b"},"stats"'), False), (ADD2[:-2] + b',"tags":{"a":"b"}}}', False),
        (ADD2[:-2] + b",}}", False), (ADD2[:-1], False), (ADD2 + b"}", False), (ADD2.replace(b"true", b"tru"), False),
        (ADD2.replace(b'"path":"p0', b'"path":"\\u0070'), True),      # an escaped path: F_PATH_ESCAPED
        (RM2.replace(b',"extendedFileMetadata":true,"partitionValues":{"p0":"2020-01-05","p1":"7"},"size":99', b""), True),
        (RM2.replace(b',"size":99', b""), False), (b"", False), (b"{}", False), (b'{"add":{}}', False),
        (b'{"add":null}', False),
    ]


def test_named_cases(lib):
    for line, want in named_cases():
        got = check(lib, line)
        assert want is None or got == want, (line, got, want)
    m, g = _R7(), _R7()
    esc = ADD2.replace(b'"path":"p0', b'"path":"\\u0070')
    assert lib.js_check(esc, len(esc), 0, m, g) == 1 and m[1] == 4   # F_PATH_ESCAPED from the token's class


# ---- the stand-alone sanitizer program -------------------------------------------------------------------
def test_sanitizer_program(tmp_path):
    exe = str(tmp_path / "json_shape_host")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-DJS_MAIN"] + ASAN + [SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = golden_lines() + [x for nc in (0, 1, 2, 4) for side in writer_lines(nc) for x in side]
    lines += [x for x, _ in named_cases()] + mutated_lines(2000, 0xA5A)
    data = str(tmp_path / "lines.bin")
    with open(data, "wb") as f:
        for x in lines:
            f.write(struct.pack("<I", len(x)) + x)
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    got = re.fullmatch(r"lines (\d+) accepted (\d+)\n", r.stdout)
    assert got and int(got.group(1)) == len(lines) and int(got.group(2)) >= 16 * 100, r.stdout
