"""Partition-pruning corpus for the string pattern predicates (LIKE, StartsWith, EndsWith,
Contains): one table of 2,113 live files (two 1,024-file leaf tiles, one 64-file mask word, and one
more file) whose string partition column cycles through the values that break a matcher -- the
8-byte register prefix boundary, the long-string gather, shared prefixes, multi-byte characters at
every position, the pattern metacharacters themselves, NULL -- beside an integer column for
AND / OR / NOT combinations.

The oracle has no pattern ops, so the expected values come from here, twice over:
  (a) `like_regex`: the pattern translated to Python `re` as StringUtils.escapeLikeRegex translates
      it to a Java regex, matched with re.DOTALL and fullmatch on `str` (code points, as Java's `.`);
  (b) `like_bytes`: the byte-level definition the device follows -- a character is one
      non-continuation byte plus the continuation bytes after it, continuation bytes before the first
      other byte are one character each -- matched by a dynamic program over characters.
They agree on every valid UTF-8 (value, pattern) pair of the corpus (tests/test_like_lane.py)."""
import json
import os
import re

from delta_amd.testing import synth as S
from oracle import delta_oracle as O

PTYPES = {"s": "string", "part": "integer"}
SCHEMA = {"type": "struct", "fields": [{"name": "id", "type": "long", "nullable": True, "metadata": {}}] + [
    {"name": c, "type": t, "nullable": True, "metadata": {}} for c, t in PTYPES.items()]}
METADATA = {"id": "filter-like-corpus", "format": {"provider": "parquet", "options": {}},
            "schemaString": json.dumps(SCHEMA, separators=(",", ":")), "partitionColumns": list(PTYPES),
            "configuration": {}, "createdTime": 1600000000000}
PROTOCOL = {"minReaderVersion": 1, "minWriterVersion": 2}
N_LIVE = 2113

V16 = "abcdefgh01234567"
V17 = "abcdefgh012345678"
V40 = "z" * 23 + V17                      # 40 bytes, ends with the 17-byte needle
V42 = V17 + "-and-a-long-tail-of-bytes"   # 42 bytes, begins with it
VALUES = [
    # lengths 0, 1, 7, 8, 9 (two sharing the 8-byte prefix), 16, 17, ~40; NULL
    "", "a", "abcdefg", "abcdefgh", "abcdefghi", "abcdefghX", V16, V17, V40, V42, None,
    # the retry and overlap shapes
    "aa", "ab", "aba", "abab", "aaab", "abc", "aXbXc", "xay", "ba", "abcabc",
    # 2-, 3- and 4-byte characters at the start, in the middle and at the end
    "é", "éa", "aé", "aéb", "aéé", "éé", "€uro", "eu€ro", "euro€", "😀ab", "a😀b", "ab😀", "abcdefg€", "abcdefgé!", "é€😀",
    # the metacharacters, a backslash, a newline
    "%", "_", "\\", "100%", "a_c", "a%c", "a\nc", "\n", "back\\slash", "50%_off",
    # quotes and a non-ASCII character: JSON-escaped in the log (\" always, é in the lines
    # written with ensure_ascii), so the unescaped bytes are what is matched
    'say "é"',
    # region- and date-like values
    "eu-west-1", "eu-central-1", "us-east-1", "2024-03-01", "2024-03-15", "2024-04-01",
]
assert len(VALUES) == 53  # a prime: every (value, part) combination of the strides below occurs


def _pv(i):
    return {"s": VALUES[(i * 7 + 3) % len(VALUES)], "part": str(i % 5)}


def _add(i):
    return {"path": "f-%05d.parquet" % i, "partitionValues": _pv(i), "size": 100 + i,
            "modificationTime": 1600000000000 + i, "dataChange": True, "stats": None}


def _line(a, i):
    return json.dumps(a, separators=(",", ":"), ensure_ascii=bool(i % 2))  # raw UTF-8 / \\u escapes by turns


N_ADDS = 2238  # adds written; every 9th of the first half is removed again


def live_indices():
    """The `_add` indices of the table's live files, as `build` leaves them."""
    removed = set(range(0, N_ADDS // 2, 9))
    return [i for i in range(N_ADDS) if i not in removed]


def live_files():
    return [_add(i) for i in live_indices()]


def build(table_dir, checkpoint=False):
    """Returns the _delta_log path of the N_LIVE-file table. v0: protocol, metadata, the first half
    of the adds; v1: removes every 9th of those and adds most of the rest; v2: the last 30 adds.
    With `checkpoint`, a checkpoint of the v1 state: its files' values are then read from the
    checkpoint's partitionValues map column, the last 30 from JSON."""
    log = os.path.join(table_dir, "_delta_log")
    os.makedirs(log, exist_ok=True)
    n = N_ADDS
    h = n // 2
    removed = list(range(0, h, 9))
    assert len(live_indices()) == n - len(removed) == N_LIVE
    with open(os.path.join(log, "%020d.json" % 0), "w", encoding="utf-8") as f:
        f.write(_line({"protocol": PROTOCOL}, 0) + "\n" + _line({"metaData": METADATA}, 0) + "\n")
        for i in range(h):
            f.write(_line({"add": _add(i)}, i) + "\n")
    with open(os.path.join(log, "%020d.json" % 1), "w", encoding="utf-8") as f:
        for i in removed:
            f.write(_line({"remove": {"path": "f-%05d.parquet" % i, "deletionTimestamp": 1600000001000,
                                      "dataChange": True}}, i) + "\n")
        for i in range(h, n - 30):
            f.write(_line({"add": _add(i)}, i) + "\n")
    with open(os.path.join(log, "%020d.json" % 2), "w", encoding="utf-8") as f:
        for i in range(n - 30, n):
            f.write(_line({"add": _add(i)}, i) + "\n")
    if checkpoint:
        live = [_add(i) for i in live_indices() if i < n - 30]
        S.write_checkpoint_records(os.path.join(log, "%020d.checkpoint.parquet" % 1), PROTOCOL, METADATA, live,
                                   row_group_size=700, use_dictionary=True)
        with open(os.path.join(log, "_last_checkpoint"), "w") as f:
            f.write('{"version":1,"size":%d}\n' % (len(live) + 2))
    return log


# ---- (a) StringUtils.escapeLikeRegex in Python re ---------------------------------------------------
class PatternInvalid(ValueError):
    pass


def like_regex(pattern: str, escape: str = "\\") -> str:
    out, i = [], 0
    while i < len(pattern):
        c = pattern[i]
        if c == escape:
            if i + 1 == len(pattern):
                raise PatternInvalid("it is not allowed to end with the escape character")
            c = pattern[i + 1]
            if c not in ("_", "%", escape):
                raise PatternInvalid("the escape character is not allowed to precede '%s'" % c)
            out.append(re.escape(c))
            i += 2
            continue
        out.append("." if c == "_" else ".*" if c == "%" else re.escape(c))
        i += 1
    return "".join(out)


def like_str(value: str, pattern: str, escape: str = "\\") -> bool:
    return re.compile(like_regex(pattern, escape), re.DOTALL).fullmatch(value) is not None


# ---- (b) the byte-level character definition ----------------------------------------------------------
def chars(b: bytes):
    """One non-continuation byte plus the continuation bytes (10xxxxxx) after it; continuation bytes
    before the first other byte are one character each."""
    out = []
    for x in b:
        if x & 0xC0 == 0x80 and out and out[-1][0] & 0xC0 != 0x80:
            out[-1] += bytes([x])
        else:
            out.append(bytes([x]))
    return out


def like_bytes(value: bytes, pattern: bytes, escape: bytes = b"\\") -> bool:
    """`pattern` (valid UTF-8) against any bytes: set of reachable character positions per token."""
    toks, pc, i = [], chars(pattern), 0
    while i < len(pc):
        c = pc[i]
        if c == escape:
            if i + 1 == len(pc):
                raise PatternInvalid("it is not allowed to end with the escape character")
            if pc[i + 1] not in (b"_", b"%", escape):
                raise PatternInvalid("the escape character is not allowed to precede %r" % pc[i + 1])
            toks.append(("lit", pc[i + 1]))
            i += 2
            continue
        toks.append(("one",) if c == b"_" else ("any",) if c == b"%" else ("lit", c))
        i += 1
    v = chars(value)
    cur = {0}
    for t in toks:
        if t[0] == "any":
            cur = set(range(min(cur), len(v) + 1)) if cur else cur
        else:
            cur = {k + 1 for k in cur if k < len(v) and (t[0] == "one" or v[k] == t[1])}
    return len(v) in cur


# ---- three-valued evaluation of a predicate tree -------------------------------------------------------
def like_eval(expr, pv, schema=PTYPES):
    """O.eval_predicate's tree walk (None is NULL) with the four pattern ops, by evaluator (a)."""
    op = expr[0]
    if op == "col":
        field = next(f for f in schema if f.lower() == expr[1].strip("`").lower())
        return O.cast_string((pv or {}).get(field), schema[field])
    if op == "lit":
        return expr[2]
    if op in ("startswith", "endswith", "contains", "like"):
        a, b = like_eval(expr[1], pv, schema), like_eval(expr[2], pv, schema)
        if a is None or b is None:
            return None
        ab, bb = a.encode("utf-8"), b.encode("utf-8")
        if op == "like":
            return like_str(a, b, expr[3] if len(expr) > 3 else "\\")
        return ab.startswith(bb) if op == "startswith" else ab.endswith(bb) if op == "endswith" else bb in ab
    if op in ("=", "!=", "<", "<=", ">", ">="):
        a, b = like_eval(expr[1], pv, schema), like_eval(expr[2], pv, schema)
        if a is None or b is None:
            return None
        if isinstance(a, str):
            a, b = a.encode("utf-8"), b.encode("utf-8")
        return {"=": a == b, "!=": a != b, "<": a < b, "<=": a <= b, ">": a > b, ">=": a >= b}[op]
    if op in ("isnull", "isnotnull"):
        return (like_eval(expr[1], pv, schema) is None) == (op == "isnull")
    if op == "in":
        a = like_eval(expr[1], pv, schema)
        vals = [like_eval(l, pv, schema) for l in expr[2]]
        if a is None:
            return None
        return True if a in [v for v in vals if v is not None] else (None if None in vals else False)
    if op == "not":
        a = like_eval(expr[1], pv, schema)
        return None if a is None else (not a)
    a, b = like_eval(expr[1], pv, schema), like_eval(expr[2], pv, schema)
    if op == "and":
        return False if (a is False or b is False) else (None if (a is None or b is None) else True)
    if op == "or":
        return True if (a is True or b is True) else (None if (a is None or b is None) else False)
    raise ValueError(op)


def expected(files, preds, schema=PTYPES):
    """The files `preds` (ANDed) select: those where every conjunct is TRUE."""
    return [f for f in files if all(like_eval(e, f["partitionValues"], schema) is True for e in preds)]


C = lambda n: ("col", n)  # noqa: E731
L = lambda t, v: ("lit", t, v)  # noqa: E731
STR = lambda v: L("string", v)  # noqa: E731
LIKE = lambda p, *esc: ("like", C("s"), STR(p)) + esc  # noqa: E731
PART = lambda op, v: (op, C("part"), L("integer", v))  # noqa: E731

# (pattern, escape) of every LIKE in the corpus, for the matcher tests
LIKE_PATTERNS = [(p, "\\") for p in (
    "", "%", "%%", "_", "__", "_%", "%_", "_%_", "a%", "%a", "%a%", "a%a", "%ab%ab", "%aab", "a_c", "%_é", "é_%",
    "a%b%c", "100\\%", "%\\%%", "a\\_c", "%\\_%", "\\\\", "%\\\\%", "abcdefgh_1234567", "%h01234567_", "z%_bcdefgh012345678",
    "abcdefgh%", "%01234567", "%fgh0123%", "abcdefgh", "_bcdefgh_", "%_€%", "😀__", "%😀", "_😀_", "eu-%-1", "2024-03-%",
    "2024-0_-01", "%\n%", "_\n_", "a%é", "%é%é", "say \"_\"", "________%", "%_________", "%b_", "_b%")] + [
    ("a#_c", "#"), ("%#%#_%", "#"), ("#%%", "#"), ("aé_c", "é"), ("éé%", "é"), ("%%", "%"), ("a%_c", "%"), ("100€%", "€")]

# always NULL: nothing is selected, with or without NOT
ALWAYS_NULL = [
    [("like", C("s"), L("string", None))],
    [("not", ("like", C("s"), L("string", None)))],
    [("startswith", C("s"), L("string", None))],
    [("not", ("endswith", C("s"), L("string", None)))],
    [("contains", C("s"), L("integer", None))],
]

# TRUE for every non-NULL value, so FALSE or NULL under NOT: nothing is selected either (`%` must not
# become IS NOT NULL, whose NOT is TRUE for a NULL value)
NEVER_TRUE = [[("not", LIKE("%"))], [("not", LIKE("%%"))], [("not", ("startswith", C("s"), STR("")))],
              [("not", ("endswith", C("s"), STR("")))], [("not", ("contains", C("s"), STR("")))]]

NEEDLES = ["", "a", "abcdefgh", "abcdefghi", V17]  # 0, 1, 8, 9 and 17 bytes
PREDICATES = (
    [[LIKE(p) if e == "\\" else LIKE(p, e)] for p, e in LIKE_PATTERNS] +
    [[("startswith", C("s"), STR(n))] for n in NEEDLES + ["é", "😀", "eu-", "abcdefgh0", "\\"]] +
    [[("endswith", C("s"), STR(n))] for n in ["", "a", "01234567", "h01234567", V17, "é", "€", "😀", "-1", "%", "c"]] +
    [[("contains", C("s"), STR(n))] for n in NEEDLES + ["é", "€", "b😀", "\n", "%_", "\"", "fgh01234567", "-a-long-tail-of-"]] +
    # each op under NOT (a NULL value stays NULL: not selected)
    [[("not", LIKE("a%"))], [("not", LIKE("a_c"))], [("not", LIKE("%_é"))],
     [("not", ("startswith", C("s"), STR("abcdefgh")))], [("not", ("endswith", C("s"), STR("c")))],
     [("not", ("contains", C("s"), STR("é")))]] +
    # inside AND / OR with a comparison on the other column
    [[("and", LIKE("a%"), PART("=", 3))], [("or", LIKE("%é"), PART("=", 1))],
     [("and", ("startswith", C("s"), STR("eu-")), PART("<", 2))],
     [("or", ("endswith", C("s"), STR("-1")), ("and", ("contains", C("s"), STR("%")), PART(">=", 3)))],
     [("and", ("not", LIKE("_b%")), ("in", C("part"), [L("integer", 0), L("integer", 4)]))],
     [("or", ("not", ("contains", C("s"), STR("a"))), ("isnull", C("s")))],
     [LIKE("abcdefgh%"), ("not", LIKE("%_X")), PART("!=", 0)],
     [("or", ("like", C("s"), L("string", None)), PART("=", 2))],
     [("and", ("or", LIKE("a#%c", "#"), LIKE("%\\_%")), ("!=", C("s"), STR("_")))],
     [("=", C("s"), STR("abcdefgh")), ("like", C("S"), STR("abcdefg_"))]]
)

INVALID_PATTERNS = [("abc\\", "\\", "it is not allowed to end with the escape character"),
                    ("a\\bc", "\\", "the escape character is not allowed to precede 'b'"),
                    ("#", "#", "it is not allowed to end with the escape character"),
                    ("a#é", "#", "the escape character is not allowed to precede 'é'"),
                    ("é€", "é", "the escape character is not allowed to precede '€'")]
