"""Host side of the string pattern predicates (delta_amd/predicates.py): the program build_program
emits for StartsWith / EndsWith / Contains / Like, its operand rules, and the conjunct split that
hands them to dr_filter."""
import pytest

from delta_amd import predicates as P
from tests import filter_like_corpus as F

SCHEMA = {"s": "string", "b": "binary", "n": "integer"}
C, L = F.C, F.L


def test_opcodes_are_the_abi_values():
    assert [P.OP_CODE[k] for k in ("startswith", "endswith", "contains", "like")] == [15, 16, 17, 18]


@pytest.mark.parametrize("op", ["startswith", "endswith", "contains"])
def test_build_program_bytewise_ops(op):
    p = P.build_program(SCHEMA, [(op, C("S"), L("string", "eu-é"))])
    assert p.ops == [(P.OP_COL, 0), (P.OP_LIT, 0), (P.OP_CODE[op], 0)]
    assert p.cols == [("s", 0)] and p.lits == [(0, "eu-é".encode("utf-8"))]


def test_build_program_like_escape():
    """DR_OP_LIKE's arg is the escape character's code point: Spark's default backslash, or the
    fourth element."""
    p = P.build_program(SCHEMA, [("like", C("s"), L("string", "a\\%_"))])
    assert p.ops == [(P.OP_COL, 0), (P.OP_LIT, 0), (18, 92)] and p.lits == [(0, b"a\\%_")]
    assert P.build_program(SCHEMA, [("like", C("s"), L("string", "a#%_"), "#")]).ops[-1] == (18, ord("#"))
    assert P.build_program(SCHEMA, [("like", C("s"), L("string", "aé%"), "é")]).ops[-1] == (18, 0xE9)
    p = P.build_program(SCHEMA, [("not", ("like", C("s"), L("string", None))), ("=", C("n"), L("integer", 1))])
    assert p.ops == [(P.OP_COL, 0), (P.OP_LIT, 0), (18, 92), (P.OP_CODE["not"], 0), (P.OP_COL, 1), (P.OP_LIT, 1),
                     (P.OP_CODE["="], 0), (P.OP_CODE["and"], 0)]
    assert p.lits[0] == (0, None)
    # a NULL literal of any type is a NULL pattern
    assert P.build_program(SCHEMA, [("contains", C("s"), L("integer", None))]).lits == [(3, None)]


@pytest.mark.parametrize("op", ["startswith", "endswith", "contains", "like"])
def test_operand_rules(op):
    pat = L("string", "x")
    for bad, what in (((op, C("n"), pat), "string partition column"),          # a non-string column
                      ((op, C("b"), pat), "string partition column"),          # a binary column
                      ((op, L("string", "v"), pat), "string partition column"),  # no column at all
                      ((op, C("s"), C("s")), "string or NULL literal"),        # column against column
                      ((op, C("s"), L("integer", 5)), "string or NULL literal"),
                      ((op, C("s"), L("binary", b"x")), "string or NULL literal"),
                      ((op, C("s"), ("not", pat)), "string or NULL literal"),
                      ((op, C("s")), "takes a column and a literal")):
        with pytest.raises(P.PredicateError, match=what):
            P.build_program(SCHEMA, [bad])
    with pytest.raises(P.PredicateError, match="not a partition column"):
        P.build_program(SCHEMA, [(op, C("nope"), pat)])


def test_like_pattern_and_escape_rules():
    for p, e, msg in F.INVALID_PATTERNS:
        with pytest.raises(P.PredicateError) as err:
            P.build_program(SCHEMA, [("like", C("s"), L("string", p), e)])
        assert msg in str(err.value) and "the pattern '%s' is invalid" % p in str(err.value)
    for esc in ("", "ab", "\U0001F600", "\x00", "\ud800", 92, None):
        with pytest.raises(P.PredicateError, match="escape"):
            P.build_program(SCHEMA, [("like", C("s"), L("string", "a%"), esc)])
    with pytest.raises(P.PredicateError, match="takes a column and a literal"):
        P.build_program(SCHEMA, [("startswith", C("s"), L("string", "a"), "#")])  # only LIKE takes an escape
    # the escape test comes before the wildcard test
    P.build_program(SCHEMA, [("like", C("s"), L("string", "%%"), "%")])
    with pytest.raises(P.PredicateError, match="not allowed to end"):
        P.build_program(SCHEMA, [("like", C("s"), L("string", "%%%"), "%")])


def test_conjunct_split_lets_pattern_ops_through():
    parts = ["s", "n"]
    like = ("like", C("s"), L("string", "2024-03-%"), "#")  # the escape is no expression
    sw = ("startswith", C("`S`"), L("string", "eu-"))
    data = ("contains", C("payload"), L("string", "x"))
    mixed = ("or", ("endswith", C("s"), L("string", "z")), ("=", C("payload"), L("string", "y")))
    expr = ("and", ("and", like, data), ("and", sw, ("and", mixed, ("=", C("n"), L("integer", 3)))))
    meta, rest = P.split_metadata_and_data_predicates(expr, parts)
    assert meta == [like, sw, ("=", C("n"), L("integer", 3))] and rest == [data, mixed]
    assert P.is_partition_only(like, parts) and P.is_partition_only(("not", sw), parts)
    assert not P.is_partition_only(data, parts)
    prog = P.build_program({"s": "string", "n": "integer"}, meta)
    assert [o for o, _ in prog.ops if o >= 15] == [18, 15]


def test_every_corpus_predicate_builds():
    for preds in F.PREDICATES + F.ALWAYS_NULL + F.NEVER_TRUE:
        prog = P.build_program(F.PTYPES, preds)
        pred, keep = P.lower_program(prog)
        assert pred.nops == len(prog.ops)
