"""The K5 pattern matcher (delta_amd/csrc/like_lane.h: like_match, the bytewise tests and the host's
pattern compiler), host build, against the corpus's two evaluators (tests/filter_like_corpus.py):
(a) StringUtils.escapeLikeRegex restated in Python `re`, (b) the byte-level character definition.
The matcher is the device code of k_filter_leaf_x / k_dict_leaf / k_filter_typed; here it is compiled
with g++ and run on the corpus pairs, a seeded fuzz of valid UTF-8 pairs against (a) and of random
bytes against (b). A stand-alone program runs the same kind of fuzz under AddressSanitizer and
UndefinedBehaviorSanitizer."""
import ctypes as C
import os
import random
import subprocess

import pytest

from tests import filter_like_corpus as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "build", "liblikelane_host.so")
HDR = os.path.join(ROOT, "delta_amd", "csrc", "like_lane.h")
KINDS = {0: "eq", 1: "startswith", 2: "endswith", 3: "contains", 4: "program"}


def _stale(out, *srcs):
    return not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs)


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(ROOT, "tests", "native", "like_lane_host.cpp")
    if _stale(LIB, src, HDR):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", LIB, src])
    L = C.CDLL(LIB)
    L.lk_compile.restype = C.c_int
    L.lk_eval.restype = C.c_int
    return L


def compile_pattern(lib, pattern: bytes, escape: int):
    """(kind, bytes) of a valid pattern, or the error text."""
    kind, n = C.c_int(), C.c_uint()
    out, err = C.create_string_buffer(4096), C.create_string_buffer(512)
    rc = lib.lk_compile(pattern, len(pattern), escape, C.byref(kind), out, 4096, C.byref(n), err, 512)
    assert rc in (0, 1)
    return err.value.decode("utf-8") if rc else (kind.value, out.raw[:n.value])


def match(lib, value: bytes, compiled) -> bool:
    # the value in a buffer of exactly its length
    buf = (C.c_ubyte * max(len(value), 1)).from_buffer_copy(value or b"\0")
    return bool(lib.lk_eval(compiled[0], buf, len(value), compiled[1], len(compiled[1])))


def test_corpus_evaluators_agree():
    """(a) and (b) agree on every (value, pattern) pair of the corpus (all valid UTF-8)."""
    for p, e in F.LIKE_PATTERNS:
        for v in F.VALUES:
            if v is None:
                continue
            a = F.like_str(v, p, e)
            assert a == F.like_bytes(v.encode("utf-8"), p.encode("utf-8"), e.encode("utf-8")), (v, p, e)


def test_corpus_predicates_select_some_but_not_all():
    """Every predicate but the listed always-NULL and never-TRUE ones selects at least one live file
    and fewer than all."""
    files = F.live_files()
    assert len(files) == F.N_LIVE
    for preds in F.PREDICATES:
        n = len(F.expected(files, preds))
        assert 0 < n < F.N_LIVE, (preds, n)
    for preds in F.ALWAYS_NULL + F.NEVER_TRUE:
        assert F.expected(files, preds) == []


def test_corpus_pairs(lib):
    for p, e in F.LIKE_PATTERNS:
        c = compile_pattern(lib, p.encode("utf-8"), ord(e))
        assert not isinstance(c, str), (p, c)
        for v in F.VALUES:
            if v is not None:
                assert match(lib, v.encode("utf-8"), c) == F.like_str(v, p, e), (v, p, e, KINDS[c[0]])


def test_simple_shapes_fold(lib):
    """No wildcard: EQ; `abc%`: STARTSWITH; `%abc`: ENDSWITH; `%abc%`: CONTAINS; `%` alone: STARTSWITH of
    the empty string (TRUE for every non-NULL value, NULL for NULL -- IS NOT NULL would turn TRUE
    under NOT for a NULL value); anything else a program."""
    cases = [("", "eq", b""), ("abc", "eq", b"abc"), ("a\\%c\\\\", "eq", b"a%c\\"), ("abc%", "startswith", b"abc"),
             ("%abc", "endswith", b"abc"), ("%%abc%", "contains", b"abc"), ("%", "startswith", b""),
             ("%%%", "startswith", b""), ("\\_x%", "startswith", b"_x")]
    for p, kind, text in cases:
        c = compile_pattern(lib, p.encode("utf-8"), 92)
        assert (KINDS[c[0]], c[1]) == (kind, text), p
    for p in ("_", "a%b", "%a_", "_%", "%a%b%", "a_"):
        assert KINDS[compile_pattern(lib, p.encode("utf-8"), 92)[0]] == "program", p


def test_invalid_patterns(lib):
    for p, e, msg in F.INVALID_PATTERNS:
        got = compile_pattern(lib, p.encode("utf-8"), ord(e))
        assert isinstance(got, str) and msg in got and ("the pattern '%s' is invalid" % p) in got, (p, got)
        with pytest.raises(F.PatternInvalid):
            F.like_regex(p, e)
    for bad in (b"\xff", b"a\xc3", b"\x80abc", b"\xed\xa0\x80", b"\xc0\xaf", b"\xf4\x90\x80\x80"):
        got = compile_pattern(lib, bad, 92)
        assert isinstance(got, str) and "not valid UTF-8" in got, bad
    for esc in (0, 0x10000, 0xD800, 0xDFFF):
        got = compile_pattern(lib, b"abc", esc)
        assert isinstance(got, str) and "escape character" in got, esc


def _random_text(rng, alphabet, maxlen):
    return "".join(rng.choice(alphabet) for _ in range(rng.randrange(maxlen + 1)))


def test_fuzz_valid_utf8_against_regex(lib):
    """Seeded pairs over a four-letter alphabet (so matches are common) plus the metacharacters, the
    escape, a newline and multi-byte characters."""
    rng = random.Random(20240301)
    matched = programs = 0
    for escape in ("\\", "#", "é"):
        plain = ["a", "b", "c", "d"]
        pat_alpha = plain * 2 + ["%", "%", "_", "_", escape, "é", "€", "😀", "\n"]
        val_alpha = plain * 4 + ["%", "_", escape, "é", "€", "😀", "\n"]
        for _ in range(12000):
            p, v = _random_text(rng, pat_alpha, 6), _random_text(rng, val_alpha, 9)
            try:
                want = F.like_str(v, p, escape)
            except F.PatternInvalid:
                assert isinstance(compile_pattern(lib, p.encode("utf-8"), ord(escape)), str), (p, escape)
                continue
            c = compile_pattern(lib, p.encode("utf-8"), ord(escape))
            assert not isinstance(c, str), (p, c)
            assert match(lib, v.encode("utf-8"), c) == want, (v, p, escape, KINDS[c[0]])
            matched += want
            programs += c[0] == 4
    print("matched", matched, "programs", programs)
    assert matched > 1000 and programs > 5000  # the fuzz does reach matches, and the matcher proper


def test_fuzz_random_bytes_against_character_definition(lib):
    """Values of any bytes (continuation bytes first, truncated and stray lead bytes) against (b).
    Only programs: the folded bytewise tests are UTF8String's own on any bytes."""
    rng = random.Random(7)
    pat_alpha = ["a", "b", "%", "_", "_", "é"]
    pool = [0x61, 0x62, 0x80, 0xA9, 0xBF, 0xC3, 0xE2, 0xF0, 0xFF, 0x0A]
    done = 0
    for _ in range(20000):
        p = _random_text(rng, pat_alpha, 7).encode("utf-8")
        c = compile_pattern(lib, p, ord("#"))
        if c[0] != 4:
            continue
        v = bytes(rng.choice(pool) for _ in range(rng.randrange(11)))
        assert match(lib, v, c) == F.like_bytes(v, p, b"#"), (v, p)
        done += 1
    assert done > 8000


def test_sanitized_standalone_fuzz():
    """tests/native/like_lane_fuzz.cpp under ASan + UBSan, run directly: every value lives in a heap
    block of exactly its length."""
    src = os.path.join(ROOT, "tests", "native", "like_lane_fuzz.cpp")
    exe = os.path.join(ROOT, "build", "like_lane_fuzz")
    if _stale(exe, src, HDR):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, src])
    r = subprocess.run([exe, "60000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fuzz ok" in r.stdout, r.stdout + r.stderr
