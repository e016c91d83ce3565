"""Data skipping: data filters rewritten into predicates over per-file statistics (`add.stats`,
PROTOCOL.md "Per-file Statistics"), evaluated by `dr_filter` together with the partition program.

The reference at this version has no stats skipping (its `stats/` package is only DeltaScan); the
rules are those of Delta's later releases (DataSkippingReader), restated here. A rewritten predicate
is TRUE -- or NULL-guarded into TRUE -- for every file that may hold a row the data filter selects,
so a file is dropped only when its statistics prove that no row matches. v is a non-NULL literal of
the column's type:

    c = v            min <= v AND max >= v
    c < v            min < v                      c <= v     min <= v
    c > v            max > v                      c >= v     max >= v
    c != v           min != v OR max != v
    c IN (v1..vk)    OR of the equalities, k <= 16
    c IS NULL        nullCount > 0
    c IS NOT NULL    nullCount < numRecords
    A AND B          both sides; a side that cannot be rewritten is dropped
    A OR B           both sides; TRUE if either cannot be rewritten
    NOT              pushed to the leaves first (De Morgan, flipped comparisons); otherwise TRUE
    anything else    TRUE (LIKE, functions, <=>, NULL literals, boolean, binary and partition columns)

Every leaf is ORed with IS NULL of each statistics column it reads, so a file without the statistic
is kept; the combination holds no NOT, so it stays monotone. TIMESTAMP statistics are truncated to
milliseconds: every max-side leaf of a timestamp column compares against v - 999 microseconds
(saturating). String statistics are prefixes (the max with a maximal character appended): both stay
valid bounds and need no adjustment.

Statistics columns are expression nodes ("stats", source, path, type): source one of N.DR_SRC_STATS_*,
path the tuple of the data column's field names, type its Spark type name; predicates.build_program
lowers them to columns whose type carries the source.
"""
from __future__ import annotations

import json
from typing import Dict, List, Optional, Sequence, Tuple

from . import _native as N
from .predicates import _INT_TYPES, _lit, _resolve, type_code, T_DECIMAL, T_TIMESTAMP, PredicateError

MIN, MAX, NULLCOUNT, NUMRECORDS = N.DR_SRC_STATS_MIN, N.DR_SRC_STATS_MAX, N.DR_SRC_STATS_NULLCOUNT, N.DR_SRC_STATS_NUMRECORDS
IN_MAX = 16
MAX_COLUMNS, MAX_STACK = 16, 32   # dr_filter's limits: PV_MAXC columns per program, PV_STACK values deep
MAX_OPS, MAX_LITERALS = 4096, 2048  # a bound of this module's own on what one call carries (no library limit)
TS_SLACK = 999          # microseconds a millisecond-truncated timestamp statistic may lack
MAX_SEGMENTS, MAX_PATH_BYTES = 8, 255
_I64_MIN = -(1 << 63)
_FLIP = {"<": ">", "<=": ">=", ">": "<", ">=": "<=", "=": "=", "!=": "!="}       # lit op col -> col op lit
_NEGATE = {"<": ">=", "<=": ">", ">": "<=", ">=": "<", "=": "!=", "!=": "="}    # NOT (col op lit)
_SKIPPABLE = ("byte", "short", "integer", "long", "date", "timestamp", "float", "double", "string")


def data_schema(metadata: Optional[dict]) -> Dict[Tuple[str, ...], str]:
    """Every leaf of metaData.schemaString that is no partition column: path (field names, struct
    fields nested) -> Spark type name. Arrays, maps and other non-primitive leaves are left out."""
    if not metadata:
        return {}
    parts = set(metadata.get("partitionColumns") or [])
    out: Dict[Tuple[str, ...], str] = {}

    def walk(fields, prefix):
        for f in fields:
            t, path = f["type"], prefix + (f["name"],)
            if isinstance(t, dict):
                if t.get("type") == "struct":
                    walk(t.get("fields") or [], path)
            elif isinstance(t, str) and not (not prefix and f["name"] in parts):
                out[path] = t
    walk(json.loads(metadata["schemaString"]).get("fields") or [], ())
    return out


def _skippable(typ: str, path: Tuple[str, ...]) -> bool:
    code = type_code(typ)
    if code is None or not (typ in _SKIPPABLE or code & 0xff == T_DECIMAL):
        return False
    return (len(path) <= MAX_SEGMENTS and all(path) and not any("\x01" in s or "\x00" in s for s in path)
            and len("\x01".join(path).encode("utf-8")) <= MAX_PATH_BYTES)


def _name_segments(name: str) -> Optional[List[str]]:
    """A column reference as path segments: `a.b` is the nested leaf a -> b, a backticked part is one
    segment whatever it holds (`` `n.x` `` is the top-level column named n.x, ``n.`x.y` `` two segments).
    None for a name that does not parse (an unclosed backtick, an empty segment)."""
    segs, cur, i, quoted = [], "", 0, False
    while i < len(name):
        ch = name[i]
        if ch == "`":
            if cur:
                return None
            j = name.find("`", i + 1)
            if j < 0 or (j + 1 < len(name) and name[j + 1] != "."):
                return None
            cur, quoted, i = name[i + 1:j], True, j + 1
            continue
        if ch == ".":
            if not cur and not quoted:
                return None
            segs.append(cur)
            cur, quoted = "", False
            if i + 1 == len(name):
                return None
        elif quoted:
            return None
        else:
            cur += ch
        i += 1
    if cur or quoted:
        segs.append(cur)
    return segs if segs and all(segs) else None


def _column(e, schema, partition_cols) -> Optional[Tuple[Tuple[str, ...], str]]:
    """(path, type) of a reference to a data column with statistics, else None. The name is split
    into segments (_name_segments) and each compares case-insensitively, as the session resolver does.
    A reference that fits more than one leaf -- two spellings that differ in case only -- is None:
    the statistics of the wrong column would drop files that hold matching rows."""
    if not isinstance(e, tuple) or e[0] != "col" or not isinstance(e[1], str) or _resolve(e[1], partition_cols) is not None:
        return None
    segs = _name_segments(e[1])
    if segs is None:
        return None
    want = tuple(s.lower() for s in segs)
    hits = [(path, typ) for path, typ in schema.items() if tuple(s.lower() for s in path) == want]
    if len(hits) != 1:
        return None
    path, typ = hits[0]
    return (path, typ) if _skippable(typ, path) else None


def _literal(e, typ: str):
    """The literal's value for a column of type `typ`, or None when it cannot stand in the rewrite:
    a NULL, a literal of another type (integer kinds go with each other), one that does not convert."""
    if not isinstance(e, tuple) or e[0] != "lit" or e[2] is None:
        return None
    same = e[1] == typ or (e[1] in _INT_TYPES and typ in _INT_TYPES)
    if not same:
        return None
    try:
        _lit(e[1], e[2])
    except (PredicateError, ValueError, TypeError):
        return None
    return e


def _guarded(expr, cols: Sequence) -> tuple:
    for c in cols:
        expr = ("or", expr, ("isnull", c))
    return expr


def _max_side(lit, typ: str):
    """The literal a max-side leaf compares with: v - 999 us for a timestamp column, saturating."""
    if type_code(typ) != T_TIMESTAMP:
        return lit
    return ("lit", "timestamp", max(_lit("timestamp", lit[2]) - TS_SLACK, _I64_MIN))


def _leaf(op: str, path, typ: str, lit) -> tuple:
    mn, mx = ("stats", MIN, path, typ), ("stats", MAX, path, typ)
    hi = _max_side(lit, typ)
    if op == "=":
        return _guarded(("and", ("<=", mn, lit), (">=", mx, hi)), (mn, mx))
    if op in ("<", "<="):
        return _guarded((op, mn, lit), (mn,))
    if op in (">", ">="):
        return _guarded((op, mx, hi), (mx,))
    return _guarded(("or", ("!=", mn, lit), ("!=", mx, hi)), (mn, mx))  # !=


def rewrite(expr, schema: Dict[Tuple[str, ...], str], partition_cols: Sequence[str] = (), negate: bool = False):
    """The skipping predicate of data filter `expr` (NOT `expr` with `negate`), or None for TRUE."""
    op = expr[0] if isinstance(expr, tuple) and expr else None
    if op == "not" and len(expr) == 2:
        return rewrite(expr[1], schema, partition_cols, not negate)
    if op in ("and", "or") and len(expr) == 3:
        a = rewrite(expr[1], schema, partition_cols, negate)
        b = rewrite(expr[2], schema, partition_cols, negate)
        if (op == "and") != negate:  # a conjunction: an unsupported side is dropped
            return b if a is None else a if b is None else ("and", a, b)
        return None if a is None or b is None else ("or", a, b)
    if op in _FLIP and len(expr) == 3:
        if isinstance(expr[1], tuple) and expr[1][0] == "lit":  # lit op col
            expr = (_FLIP[op], expr[2], expr[1])
            op = expr[0]
        col = _column(expr[1], schema, partition_cols)
        lit = _literal(expr[2], col[1]) if col else None
        if lit is None:
            return None
        return _leaf(_NEGATE[op] if negate else op, col[0], col[1], lit)
    if op == "in" and len(expr) == 3 and not negate:
        col = _column(expr[1], schema, partition_cols)
        lits = [_literal(l, col[1]) for l in expr[2]] if col else []
        if not lits or len(lits) > IN_MAX or any(l is None for l in lits):
            return None
        out = _leaf("=", col[0], col[1], lits[0])
        for l in lits[1:]:
            out = ("or", out, _leaf("=", col[0], col[1], l))
        return out
    if op in ("isnull", "isnotnull") and len(expr) == 2:
        # the counts exist for every column with statistics, whatever its type's bounds
        col = _column(expr[1], schema, partition_cols)
        if col is None:
            return None
        nc, nr = ("stats", NULLCOUNT, col[0], "long"), ("stats", NUMRECORDS, (), "long")
        if (op == "isnull") != negate:
            return _guarded((">", nc, ("lit", "long", 0)), (nc,))
        return _guarded(("<", nc, nr), (nc, nr))
    return None


def skipping_predicates(filters: Sequence, metadata: Optional[dict]) -> List[tuple]:
    """The skipping predicates of the data conjuncts of `filters` (those that reference a column
    that is no partition column); the ones that rewrite to TRUE are left out."""
    from .predicates import split_metadata_and_data_predicates
    parts = (metadata or {}).get("partitionColumns") or []
    schema = data_schema(metadata)
    out = []
    for f in filters:
        for conj in split_metadata_and_data_predicates(f, parts)[1]:
            r = rewrite(conj, schema, parts)
            if r is not None:
                out.append(r)
    return out


def _stack_depth(ops) -> int:
    """The deepest the value stack of the lowered program gets (an IN list holds its value and two
    slots, pred_plan.cpp lower_program)."""
    from .predicates import OP_COL, OP_LIT, OP_CODE, DATE_FN_CODE
    unary = {OP_CODE["isnull"], OP_CODE["isnotnull"], OP_CODE["not"]} | set(DATE_FN_CODE.values())
    depth = peak = 0
    for op, arg in ops:
        if op in (OP_COL, OP_LIT):
            depth += 1
        elif op == OP_CODE["in"]:
            depth -= arg
            peak = max(peak, depth + 2)
        elif op not in unary:
            depth -= 1
        peak = max(peak, depth)
    return peak


def within_limits(partition_schema: Dict[str, str], preds: Sequence) -> bool:
    """Does the AND of `preds` lower to a program dr_filter takes: at most 16 columns, a stack of at
    most 32 values, and this module's bounds on ops and literals?"""
    from .predicates import build_program
    prog = build_program(partition_schema, list(preds))
    return (len(prog.cols) <= MAX_COLUMNS and len(prog.ops) <= MAX_OPS and len(prog.lits) <= MAX_LITERALS
            and _stack_depth(prog.ops) <= MAX_STACK)


def fit_limits(partition_schema: Dict[str, str], base: Sequence, skipping: Sequence) -> List[tuple]:
    """The skipping conjuncts, in order, that still fit dr_filter's program limits beside `base` (the
    partition conjuncts) and the ones taken before. They are conjuncts over files that only ever drop
    more, so leaving one out is sound: asking for data skipping never turns a query that partition
    pruning answers into an error. A conjunct that does not fit is skipped, not the ones after it."""
    kept: List[tuple] = []
    for s in skipping:
        if within_limits(partition_schema, list(base) + kept + [s]):
            kept.append(s)
    return kept
