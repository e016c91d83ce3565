"""The data-skipping rewrite (delta_amd/skipping.py): its table row by row, NOT pushdown, the dropped side
under AND and TRUE under OR, the IS NULL guards, the 999 microsecond rule, and soundness -- over random
files with real rows and statistics derived from them (strings truncated to 32 characters, timestamps to
milliseconds), every file that holds a row matching a random predicate is kept by the rewritten one,
evaluated here with three-valued logic."""
import random

from delta_amd import skipping as K
from delta_amd import predicates as P

MIN, MAX, NC, NR = K.MIN, K.MAX, K.NULLCOUNT, K.NUMRECORDS
SCHEMA = {("i",): "integer", ("d",): "double", ("s",): "string", ("dt",): "date", ("ts",): "timestamp", ("n", "x"): "long",
          ("flag",): "boolean", ("bin",): "binary"}
PARTS = ["p"]
C = lambda n: ("col", n)  # noqa: E731
L = lambda t, v: ("lit", t, v)  # noqa: E731
S = lambda src, path, typ: ("stats", src, tuple(path), typ)  # noqa: E731
I_MIN, I_MAX = S(MIN, ["i"], "integer"), S(MAX, ["i"], "integer")
FIVE = L("integer", 5)


def g(e, *cols):
    for c in cols:
        e = ("or", e, ("isnull", c))
    return e


def rw(e):
    return K.rewrite(e, SCHEMA, PARTS)


def test_table_row_by_row():
    assert rw(("=", C("i"), FIVE)) == g(("and", ("<=", I_MIN, FIVE), (">=", I_MAX, FIVE)), I_MIN, I_MAX)
    assert rw(("<", C("i"), FIVE)) == g(("<", I_MIN, FIVE), I_MIN)
    assert rw(("<=", C("i"), FIVE)) == g(("<=", I_MIN, FIVE), I_MIN)
    assert rw((">", C("i"), FIVE)) == g((">", I_MAX, FIVE), I_MAX)
    assert rw((">=", C("i"), FIVE)) == g((">=", I_MAX, FIVE), I_MAX)
    assert rw(("!=", C("i"), FIVE)) == g(("or", ("!=", I_MIN, FIVE), ("!=", I_MAX, FIVE)), I_MIN, I_MAX)
    assert rw((">", FIVE, C("i"))) == rw(("<", C("i"), FIVE))  # lit op col
    seven = L("integer", 7)
    assert rw(("in", C("i"), [FIVE, seven])) == ("or", rw(("=", C("i"), FIVE)), rw(("=", C("i"), seven)))
    assert rw(("in", C("i"), [L("integer", k) for k in range(16)])) is not None
    assert rw(("in", C("i"), [L("integer", k) for k in range(17)])) is None
    nc, nr = S(NC, ["i"], "long"), S(NR, [], "long")
    assert rw(("isnull", C("i"))) == g((">", nc, L("long", 0)), nc)
    assert rw(("isnotnull", C("i"))) == g(("<", nc, nr), nc, nr)
    assert rw(("=", C("N.X"), L("long", 1))) == g(("and", ("<=", S(MIN, ["n", "x"], "long"), L("long", 1)),
                                                   (">=", S(MAX, ["n", "x"], "long"), L("long", 1))),
                                                  S(MIN, ["n", "x"], "long"), S(MAX, ["n", "x"], "long"))
    # anything else: TRUE
    for e in [("like", C("s"), L("string", "a%")), ("startswith", C("s"), L("string", "a")), ("=", ("year", C("dt")), FIVE),
              ("=", C("i"), L("integer", None)), ("<=>", C("i"), FIVE), ("=", C("flag"), L("boolean", True)),
              ("=", C("bin"), L("binary", b"x")), ("=", C("p"), FIVE), ("=", C("nosuch"), FIVE), ("=", C("i"), C("i")),
              ("=", C("i"), L("string", "5")), ("in", C("i"), [FIVE, L("integer", None)]), ("isnull", C("p")),
              ("not", ("in", C("i"), [FIVE]))]:
        assert rw(e) is None, e


def test_and_or_not():
    a, b, like = ("<", C("i"), FIVE), (">", C("d"), L("double", 1.5)), ("like", C("s"), L("string", "a%"))
    assert rw(("and", a, b)) == ("and", rw(a), rw(b))
    assert rw(("and", a, like)) == rw(a) and rw(("and", like, b)) == rw(b) and rw(("and", like, like)) is None
    assert rw(("or", a, b)) == ("or", rw(a), rw(b))
    assert rw(("or", a, like)) is None and rw(("or", like, b)) is None
    # NOT goes to the leaves: flipped comparisons, De Morgan, IS [NOT] NULL swapped
    flips = {"<": ">=", "<=": ">", ">": "<=", ">=": "<", "=": "!=", "!=": "="}
    for op, neg in flips.items():
        assert rw(("not", (op, C("i"), FIVE))) == rw((neg, C("i"), FIVE))
    assert rw(("not", ("not", a))) == rw(a)
    assert rw(("not", ("and", a, b))) == ("or", rw(("not", a)), rw(("not", b)))
    assert rw(("not", ("or", a, b))) == ("and", rw(("not", a)), rw(("not", b)))
    assert rw(("not", ("isnull", C("s")))) == rw(("isnotnull", C("s")))
    assert rw(("not", ("and", a, like))) is None            # NOT a OR TRUE
    assert rw(("not", ("or", a, like))) == rw(("not", a))   # NOT a AND TRUE
    assert rw(("not", like)) is None

    def has_not(e):
        return isinstance(e, tuple) and (e[0] == "not" or any(has_not(x) for x in e[1:] if isinstance(x, tuple)))
    assert not has_not(rw(("not", ("or", ("and", a, ("not", b)), ("isnotnull", C("dt"))))))


def test_timestamp_max_side_reads_999_microseconds_lower():
    v = 1_600_000_000_123_456
    lit, low = L("timestamp", v), L("timestamp", v - 999)
    mn, mx = S(MIN, ["ts"], "timestamp"), S(MAX, ["ts"], "timestamp")
    assert rw(("=", C("ts"), lit)) == g(("and", ("<=", mn, lit), (">=", mx, low)), mn, mx)
    assert rw((">", C("ts"), lit)) == g((">", mx, low), mx)
    assert rw((">=", C("ts"), lit)) == g((">=", mx, low), mx)
    assert rw(("<", C("ts"), lit)) == g(("<", mn, lit), mn)
    assert rw(("!=", C("ts"), lit)) == g(("or", ("!=", mn, lit), ("!=", mx, low)), mn, mx)
    floor = -(1 << 63)
    assert rw((">", C("ts"), L("timestamp", floor + 5))) == g((">", mx, L("timestamp", floor)), mx)  # saturating
    assert rw((">", C("dt"), L("date", 3))) == g((">", S(MAX, ["dt"], "date"), L("date", 3)), S(MAX, ["dt"], "date"))


def test_lowers_to_one_program_with_sources():
    r = rw(("and", ("=", C("i"), FIVE), ("isnotnull", C("s"))))
    prog = P.build_program({"p": "integer"}, [("=", C("p"), L("integer", 1)), r])
    src = lambda s, t: t | s << 24  # noqa: E731
    assert prog.cols == [("p", 3), ("i", src(MIN, 3)), ("i", src(MAX, 3)), ("s", src(NC, 4)), ("", src(NR, 4))]
    nested = P.build_program({}, [rw(("<", C("n.x"), L("long", 0)))])
    assert nested.cols == [("n\x01x", src(MIN, 4))]
    md = {"schemaString": '{"type":"struct","fields":[{"name":"a","type":"long"},{"name":"p","type":"integer"},'
                          '{"name":"st","type":{"type":"struct","fields":[{"name":"b","type":"string"},'
                          '{"name":"arr","type":{"type":"array","elementType":"long","containsNull":true}}]}}]}',
          "partitionColumns": ["p"]}
    assert K.data_schema(md) == {("a",): "long", ("st", "b"): "string"}
    fs = [("and", ("=", C("p"), L("integer", 1)), (">", C("a"), L("long", 3))), ("like", C("st.b"), L("string", "x%"))]
    assert K.skipping_predicates(fs, md) == [K.rewrite((">", C("a"), L("long", 3)), K.data_schema(md), ["p"])]


# ---- soundness ------------------------------------------------------------------------------------------
TYPES = {"i": "integer", "d": "double", "s": "string", "dt": "date", "ts": "timestamp"}
SOUND_SCHEMA = {(c,): t for c, t in TYPES.items()}
NAN = float("nan")


def _value(rng, col):
    if rng.random() < 0.15:
        return None
    if col == "i":
        return rng.randrange(-50, 50)
    if col == "d":
        return rng.choice([NAN, float("inf"), -0.0, 0.0]) if rng.random() < 0.1 else round(rng.uniform(-20, 20), 1)
    if col == "s":
        return rng.choice(["", "a", "ab", "b" * 40, "b" * 33 + "c", "b" * 32, "zz", "é", "\U0010ffff" * 33]) + rng.choice(["", "x", "~"])
    if col == "dt":
        return rng.randrange(18000, 18040)
    return 1_600_000_000_000_000 + rng.randrange(0, 5000) * 250  # microseconds, a quarter of a millisecond apart


def _key(col, v):
    """A value as it compares: doubles by Spark's order (NaN largest, -0.0 = 0.0), strings as UTF-8 bytes."""
    if col == "d":
        return P.fp_order_key(P.double_bits(v))
    return v.encode("utf-8") if col == "s" else v


def _stats(rows):
    """What a writer records of the rows: min / max / nullCount per column, strings truncated to 32 characters
    (the max with the largest code point appended), timestamps to milliseconds; keyed as the evaluator compares."""
    st = {(NR, ()): len(rows)}
    for col in TYPES:
        vals = [r[col] for r in rows if r[col] is not None]
        st[(NC, (col,))] = len(rows) - len(vals)
        if not vals:
            continue
        lo, hi = min(vals, key=lambda v: _key(col, v)), max(vals, key=lambda v: _key(col, v))
        if col == "s":
            lo = lo[:32]
            if len(hi) > 32:  # a writer keeps the bound valid: where the appended character does not lift the
                cut = hi[:32] + "\U0010ffff"  # prefix above the value (it is all maximal characters), no truncation
                hi = cut if cut.encode("utf-8") >= hi.encode("utf-8") else hi
        if col == "ts":
            lo, hi = lo // 1000 * 1000, hi // 1000 * 1000
        st[(MIN, (col,))], st[(MAX, (col,))] = _key(col, lo), _key(col, hi)
    return st


def _lit_key(e):
    col = {"integer": "i", "double": "d", "string": "s", "date": "dt", "timestamp": "ts", "long": "i"}[e[1]]
    return None if e[2] is None else _key(col, e[2])


def ev(e, get):
    """Three-valued evaluation; `get` resolves a column or statistics node to a comparable value or None."""
    op = e[0]
    if op in ("col", "stats"):
        return get(e)
    if op == "lit":
        return _lit_key(e)
    if op in ("=", "!=", "<", "<=", ">", ">="):
        a, b = ev(e[1], get), ev(e[2], get)
        if a is None or b is None:
            return None
        return {"=": a == b, "!=": a != b, "<": a < b, "<=": a <= b, ">": a > b, ">=": a >= b}[op]
    if op in ("isnull", "isnotnull"):
        return (ev(e[1], get) is None) == (op == "isnull")
    if op == "in":
        a, vals = ev(e[1], get), [ev(x, get) for x in e[2]]
        return None if a is None else True if a in vals else False
    if op == "not":
        a = ev(e[1], get)
        return None if a is None else not a
    a, b = ev(e[1], get), ev(e[2], get)
    if op == "and":
        return False if (a is False or b is False) else (None if (a is None or b is None) else True)
    return True if (a is True or b is True) else (None if (a is None or b is None) else False)


def _predicate(rng, depth=0):
    pick = rng.random()
    if depth < 3 and pick < 0.35:
        return (rng.choice(["and", "or"]), _predicate(rng, depth + 1), _predicate(rng, depth + 1))
    if depth < 3 and pick < 0.5:
        return ("not", _predicate(rng, depth + 1))
    col = rng.choice(list(TYPES))

    def lit():
        v = None
        while v is None:
            v = _value(rng, col)
        return L(TYPES[col], v)
    kind = rng.random()
    if kind < 0.12:
        return (rng.choice(["isnull", "isnotnull"]), C(col))
    if kind < 0.24:
        return ("in", C(col), [lit() for _ in range(rng.randrange(1, 5))])
    if kind < 0.3 and col == "s":
        return ("startswith", C(col), lit())  # not rewritten: TRUE
    e = (rng.choice(["=", "!=", "<", "<=", ">", ">="]), C(col), lit())
    return (e[0], e[2], e[1]) if rng.random() < 0.2 else e


def test_soundness():
    rng = random.Random(77001)
    files = []
    for _ in range(2000):
        rows = [{c: _value(rng, c) for c in TYPES} for _ in range(rng.randrange(1, 6))]
        st = _stats(rows)
        if rng.random() < 0.1:  # a file that lacks some statistics
            for k in rng.sample(sorted(st, key=repr), k=min(3, len(st))):
                del st[k]
        files.append((rows, st))
    rewritten = skipped = 0
    for _ in range(500):
        pred = _predicate(rng)
        skip = K.rewrite(pred, SOUND_SCHEMA, [])
        if skip is None:
            continue
        rewritten += 1
        for rows, st in files:
            matches = False
            for r in rows:
                matches |= _row_matches(pred, lambda e, r=r: None if r[e[1]] is None else _key(e[1], r[e[1]]))
            keeps = ev(skip, lambda e: st.get((e[1], e[2]))) is True
            assert keeps or not matches, (pred, rows, st)
            skipped += not keeps
    assert rewritten > 300 and skipped > 20000  # the rewrite does skip


def _row_matches(pred, get):
    """The data predicate over one row, startswith included (bytewise prefix)."""
    def walk(e):
        if e[0] == "startswith":
            a, b = walk(e[1]), walk(e[2])
            return None if a is None or b is None else a.startswith(b)
        if e[0] in ("and", "or", "not"):
            vals = [walk(x) for x in e[1:]]
            if e[0] == "not":
                return None if vals[0] is None else not vals[0]
            a, b = vals
            if e[0] == "and":
                return False if (a is False or b is False) else (None if (a is None or b is None) else True)
            return True if (a is True or b is True) else (None if (a is None or b is None) else False)
        return ev(e, get)
    return walk(pred) is True


def test_backticked_name_is_one_segment_and_ambiguity_is_true():
    """A top-level column named `n.x` beside the nested leaf n -> x: a backticked name is one segment, an
    unquoted dotted one a nested path, and neither reads the other's statistics; a reference that fits two
    leaves (spellings that differ in case only) is TRUE."""
    schema = {("n", "x"): "long", ("n.x",): "long", ("Dup",): "long", ("dup",): "long", ("a", "b.c"): "long"}
    one = L("long", 1)

    def paths(e):
        r = K.rewrite(e, schema, [])
        out = set()

        def walk(x):
            if isinstance(x, tuple):
                if x and x[0] == "stats":
                    out.add(x[2])
                for y in x[1:]:
                    walk(y)
        walk(r)
        return out if r is not None else None
    assert paths(("=", C("`n.x`"), one)) == {("n.x",)}
    assert paths(("=", C("n.x"), one)) == {("n", "x")}
    assert paths(("=", C("`n`.`x`"), one)) == {("n", "x")} and paths(("=", C("N.`X`"), one)) == {("n", "x")}
    assert paths(("=", C("a.`b.c`"), one)) == {("a", "b.c")} and paths(("=", C("a.b.c"), one)) is None
    assert paths(("=", C("dup"), one)) is None and paths(("isnull", C("DUP")), ) is None
    for bad in ("`n.x", "n.", ".x", "n..x", "`n`x", "``"):
        assert paths(("=", C(bad), one)) is None, bad
    md = {"schemaString": '{"type":"struct","fields":[{"name":"n","type":{"type":"struct","fields":[{"name":"x","type":"long"}]}},'
                          '{"name":"n.x","type":"long"}]}', "partitionColumns": []}
    (r,) = K.skipping_predicates([("=", C("`n.x`"), one)], md)
    assert "('n', 'x')" not in repr(r) and "('n.x',)" in repr(r)


def test_conjuncts_beyond_the_program_limits_are_left_out():
    """Equality filters on 9 data columns beside a partition conjunct would need 19 predicate columns; dr_filter
    takes 16. The conjuncts that fit are kept in order, a later smaller one still gets in, and nothing raises."""
    cols = ["c%d" % k for k in range(10)]
    schema = {(c,): "long" for c in cols}
    part = [("=", C("p"), L("integer", 1))]
    skip = [K.rewrite(("=", C(c), L("long", 5)), schema, ["p"]) for c in cols[:9]] + [K.rewrite(("<", C("c9"), L("long", 5)), schema, ["p"])]
    pschema = {"p": "integer"}
    assert not K.within_limits(pschema, part + skip)
    assert len(P.build_program(pschema, part + skip[:9]).cols) == 19
    kept = K.fit_limits(pschema, part, skip)
    assert kept == skip[:7] + [skip[9]]            # 1 + 14 columns, then the one-column conjunct
    assert len(P.build_program(pschema, part + kept).cols) == 16 and K.within_limits(pschema, part + kept)
    assert K.fit_limits(pschema, part, skip[:3]) == skip[:3] and K.fit_limits(pschema, part, []) == []
    # the stack: a conjunct nested deeper than dr_filter's 32 values is left out, the ones around it stay
    deep = ("<", C("c0"), L("long", 0))
    for _ in range(40):
        deep = ("or", ("<", C("c0"), L("long", 0)), ("and", ("<", C("c1"), L("long", 0)), deep))
    rdeep = K.rewrite(deep, schema, ["p"])
    assert rdeep is not None and not K.within_limits(pschema, [rdeep])
    assert K.fit_limits(pschema, part, [skip[0], rdeep, skip[1]]) == [skip[0], skip[1]]
