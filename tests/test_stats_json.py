"""The statistics locator (delta_amd/csrc/stats_json.h), host build, against Python's json.loads with hooks
that keep every token's text: a hand-made corpus covering each of its rules, then 20 000 seeded
single-byte mutations and truncations of that corpus.

Where json.loads accepts a string the results must agree token for token. Where it refuses, the header
answers ALL-ABSENT -- that is the one of the two permitted behaviours implemented here (never the values
of a prefix it had already passed): locate() is a strict reader and wipes its results on the first bad
byte. The same program, built with -fsanitize=address,undefined, runs stand-alone over the same cases."""
import json
import os
import random
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "stats_json_host.cpp")
HDRS = [os.path.join(ROOT, "delta_amd", "csrc", h) for h in ("stats_json.h", "filter_plan.h")]
ABSENT, NULL, NUMBER, RAW, ESCAPED, OTHER = range(6)
MIN, MAX, NULLCOUNT, NUMRECORDS = 1, 2, 3, 4
GROUP = {MIN: "minValues", MAX: "maxValues", NULLCOUNT: "nullCount", NUMRECORDS: "numRecords"}
EIGHT = tuple("abcdefgh")
WANTS = [(MIN, ("id",)), (MAX, ("id",)), (NULLCOUNT, ("id",)), (NUMRECORDS, ()), (MIN, ("s",)), (MIN, ("n", "x")),
         (MAX, ("n", "y", "z")), (MIN, EIGHT), (MIN, ('we"ird',)), (MIN, ("é",)), (MIN, ("n",)), (MAX, ("s",))]

CORPUS = [
    b"", b"{}", b" { } ", b"null", b"[1,2]", b"7", b'"x"', b"   ",
    b'{"numRecords":3,"minValues":{"id":1,"s":"a"},"maxValues":{"id":9,"s":"z"},"nullCount":{"id":0}}',
    b' {\t"numRecords" :\n5 , "minValues" : { "id" : -2.5e+3 , "s" : "b" } ,\r\n "maxValues":{ "id":8 } , "nullCount" : { "id" : null } } ',
    # escaped keys
    b'{"minValues":{"\\u0069d":5,"we\\"ird":"q","\\u00e9":true,"\\u00E9x":1},"m\\u0061xValues":{"i\\u0064":6,"\\u0073":"esc\\n"}}',
    b'{"minValues":{"\\ud83d\\ude00":1,"\xc3\xa9":"raw utf8","s":"caf\\u00e9 \\" \\\\ \\/ \\b\\f\\n\\r\\t"}}',
    # }{ and \" inside skipped strings, nested skipped values
    b'{"skip":"}{","also":{"a":"\\"}","b":[1,{"c":"]"},[[]],{}]},"minValues":{"s":"}{\\"}{","id":4},"t":[true,false,null,-0.0e-1]}',
    # duplicate keys at each level
    b'{"numRecords":1,"numRecords":7,"minValues":{"id":1,"id":2},"maxValues":{"id":3},"maxValues":{"id":4,"id":"5"}}',
    b'{"minValues":{"id":1,"s":"x"},"minValues":{"s":"later"},"maxValues":{"id":9},"maxValues":5}',
    b'{"minValues":{"n":{"x":1},"n":{"y":{"z":"q"}}},"maxValues":{"n":{"y":{"z":"a"},"y":{"z":"b","z":"c"}}}}',
    # a non-object on the path; an object where a leaf is wanted
    b'{"minValues":{"n":5},"maxValues":{"n":{"y":"flat"}},"nullCount":[{"id":1}],"numRecords":{"id":1}}',
    b'{"minValues":{"n":{"x":{"deep":[1]}},"id":{"a":1},"s":[1]},"maxValues":null,"nullCount":{"id":[]}}',
    # 8 segments
    b'{"minValues":{"a":{"b":{"c":{"d":{"e":{"f":{"g":{"h":"leaf","i":0}}}}}}},"id":3}}',
    b'{"minValues":{"a":{"b":{"c":{"d":{"e":{"f":{"g":{"h":{"one":"more"}}},"f":{"g":{"h":-1E9}}}}}}}}}',
    # numbers of every shape
    b'{"numRecords":-0,"minValues":{"id":1.5E-7},"maxValues":{"id":123456789012345678901234567890},"nullCount":{"id":0.0}}',
]


class Num(str):
    pass


def _refuse(name):
    raise ValueError(name)


def _expected(raw: bytes):
    """Per want: None (absent) or the Python value; all None when json.loads refuses or finds no object."""
    try:
        v = json.loads(raw.decode("utf-8", "surrogateescape"), parse_int=Num, parse_float=Num, parse_constant=_refuse)
    except (ValueError, RecursionError):
        return [KeyError] * len(WANTS)
    out = []
    for src, path in WANTS:
        cur = v
        for key in (GROUP[src],) + path:
            if not isinstance(cur, dict) or key not in cur:
                cur = KeyError
                break
            cur = cur[key]
        out.append(cur)
    return out


def _agrees(raw: bytes, want, got) -> bool:
    kind, off, length = got
    span = raw[off:off + length] if off >= 0 else b""
    if want is KeyError:
        return got == (ABSENT, -1, 0)
    if want is None:
        return kind == NULL
    if isinstance(want, Num):
        return kind == NUMBER and span.decode("ascii") == want
    if isinstance(want, str):
        text = span.decode("utf-8", "surrogateescape")
        if kind == RAW:
            return b"\\" not in span and text == want and raw[off - 1:off] == b'"' and raw[off + length:off + length + 1] == b'"'
        return kind == ESCAPED and b"\\" in span and json.loads('"' + text + '"') == want
    return kind == OTHER and raw[off:off + 1] in (b"{", b"[", b"t", b"f")


def _cases():
    rng = random.Random(20240607)
    cases = list(CORPUS)
    alphabet = b'{}[]":,\\ \t\n0123456789-+.eEunltrfasxz\x00\x1f\x7f\x80\xc3\xa9\xff'
    for _ in range(20000):
        s = bytearray(rng.choice(CORPUS[8:]))
        how = rng.randrange(4)
        at = rng.randrange(len(s))
        if how == 0:
            s[at] = rng.choice(alphabet) if rng.random() < 0.8 else rng.randrange(256)
        elif how == 1:
            del s[at]
        elif how == 2:
            s.insert(at, rng.choice(alphabet))
        else:
            del s[at:]  # a truncation
        cases.append(bytes(s))
    return cases


def _case_file(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(WANTS)))
        for src, segs in WANTS:
            p = "\x01".join(segs).encode("utf-8")
            f.write(struct.pack("<iI", src, len(p)) + p)
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            f.write(struct.pack("<I", len(c)) + c)


def _run(tmp_path, cases, flags):
    exe = str(tmp_path / "stats_json_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g"] + flags + ["-o", exe, SRC])
    _case_file(str(tmp_path / "cases.bin"), cases)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(tmp_path / "cases.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    assert r.returncode == 0, r.stderr.decode("utf-8", "replace")[-4000:]
    lines = r.stdout.decode("ascii").splitlines()
    assert len(lines) == len(cases)
    return [[tuple(int(x) for x in tok.split(":")) for tok in line.split(" ")] for line in lines]


@pytest.fixture(scope="module")
def cases():
    cs = _cases()
    exp = [_expected(c) for c in cs]
    accepted = sum(any(e is not KeyError for e in ex) for ex in exp)
    assert len(cs) == len(CORPUS) + 20000 and 2000 < accepted < len(cs) - 2000  # both sides are well covered
    return cs, exp


def _compare(cs, exp, got):
    for raw, ex, g in zip(cs, exp, got):
        for (src, path), want, one in zip(WANTS, ex, g):
            assert _agrees(raw, want, one), (raw, src, path, want, one)


def test_corpus_covers_the_rules(cases):
    cs, exp = cases
    by = dict(zip(cs[:len(CORPUS)], exp[:len(CORPUS)]))
    at = lambda raw, k: by[raw][k]  # noqa: E731
    assert at(CORPUS[10], 0) == "5" and at(CORPUS[10], 1) == "6" and at(CORPUS[10], 8) == "q" and at(CORPUS[10], 9) is True
    assert at(CORPUS[12], 4) == '}{"}{' and at(CORPUS[12], 0) == "4"
    assert at(CORPUS[13], 3) == "7" and at(CORPUS[13], 0) == "2" and at(CORPUS[13], 1) == "5"
    assert at(CORPUS[14], 0) is KeyError and at(CORPUS[14], 4) == "later" and at(CORPUS[14], 1) is KeyError
    assert at(CORPUS[15], 5) is KeyError and at(CORPUS[15], 6) == "c"
    assert at(CORPUS[18], 7) == "leaf" and at(CORPUS[19], 7) == "-1E9"


def test_locator_agrees_with_json_loads(tmp_path, cases):
    cs, exp = cases
    _compare(cs, exp, _run(tmp_path, cs, []))


def test_locator_under_asan_ubsan(tmp_path, cases):
    cs, exp = cases
    _compare(cs, exp, _run(tmp_path, cs, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]))
