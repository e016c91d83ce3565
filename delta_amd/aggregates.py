"""Metadata-only aggregates: which dr_state_aggregate specs answer count / min / max expressions, and
when the per-file metadata *proves* the answer (Snapshot.aggregate_from_metadata). Host only: the
reduction itself runs on the device (State.aggregate); this module plans it and reads its result.

The reference at this version answers none of these from the log; the rules are those of Delta's later
releases (OptimizeMetadataOnlyDeltaQuery), restated:

    count(*)        sum of numRecords, when every file has numRecords
    count(c)        c a data column: sum of numRecords - sum of nullCount.c, when every file has both;
                    c a partition column: count(*) when no file's value is NULL, 0 when every one is
    min / max(c)    c a partition column: always exact (the typed value, as listFiles casts it)
                    c a data column of type byte, short, integer, long or date: the min of minValues.c /
                    max of maxValues.c, when every file either has the statistic or holds no non-NULL
                    value of c (nullCount.c == numRecords)
    anything else   not proven: timestamp statistics are truncated to milliseconds, string ones to a
                    prefix, float / double ones say nothing of NaN, decimal ones are written rounded

An answer is None when the metadata does not prove it -- and also when SQL's answer is NULL (min / max
over no non-NULL value). A data filter makes every data-column answer and every count None: data
skipping keeps files, it does not select rows.
"""
from __future__ import annotations

import struct
from typing import Dict, List, Optional, Sequence, Tuple

from . import _native as N
from .predicates import _resolve, type_code, partition_schema, PredicateError

EXACT_STATS = ("byte", "short", "integer", "long", "date")
_NUMRECORDS = ("sum", N.DR_SRC_STATS_NUMRECORDS, (), "long")


class Plan:
    """specs: the State.aggregate specs of one call (each once); items: one recipe per expression --
    (kind, spec indices ..., type) -- that `prove` reads the result through."""

    def __init__(self):
        self.specs: List[tuple] = []
        self.items: List[tuple] = []
        self.allnull: List[Tuple[int, tuple]] = []  # (spec index, data column path) whose missing statistics need the all-NULL check

    def use(self, spec) -> int:
        if spec not in self.specs:
            self.specs.append(spec)
        return self.specs.index(spec)


def plan(exprs: Sequence, metadata: Optional[dict], data_filter: bool = False) -> Plan:
    """The specs that answer `exprs` -- ("count",), ("count", col), ("min", col), ("max", col) -- over a
    table with `metadata`. `data_filter`: the selection was narrowed by a data conjunct."""
    from .skipping import data_schema, _column
    parts = list((metadata or {}).get("partitionColumns") or [])
    pschema = partition_schema(metadata)
    dschema = data_schema(metadata)
    P = Plan()
    for e in exprs:
        if not isinstance(e, tuple) or not e or e[0] not in ("count", "min", "max") or len(e) > 2 or (e[0] != "count" and len(e) != 2):
            raise PredicateError("aggregate_from_metadata takes ('count',), ('count', col), ('min', col), ('max', col), not %r" % (e,))
        if len(e) == 1:
            P.items.append(("unproven",) if data_filter else ("count_star", P.use(_NUMRECORDS)))
            continue
        fn, name = e
        if not isinstance(name, str):
            raise PredicateError("aggregate_from_metadata: a column is named by a string, not %r" % (name,))
        pcol = _resolve(name, parts)
        if pcol is not None:
            typ = pschema.get(pcol, "string")
            if type_code(typ) is None:
                P.items.append(("unproven",))
            elif fn == "count":
                P.items.append(("unproven",) if data_filter else
                               ("count_part", P.use(("count", N.DR_SRC_PARTITION, pcol, typ)), P.use(_NUMRECORDS)))
            else:
                P.items.append(("minmax_part", P.use((fn, N.DR_SRC_PARTITION, pcol, typ)), typ))
            continue
        col = _column(("col", name), dschema, parts)
        if col is None or data_filter:
            P.items.append(("unproven",))
            continue
        path, typ = col
        if fn == "count":
            P.items.append(("count_data", P.use(_NUMRECORDS), P.use(("sum", N.DR_SRC_STATS_NULLCOUNT, path, "long"))))
        elif typ in EXACT_STATS:
            k = P.use((fn, N.DR_SRC_STATS_MIN if fn == "min" else N.DR_SRC_STATS_MAX, path, typ))
            if (k, path) not in P.allnull:
                P.allnull.append((k, path))
            P.items.append(("minmax_data", k, typ))
        else:
            P.items.append(("unproven",))
    return P


def _sum64(res, a: int, g: int) -> Optional[int]:
    """Cell (a, g)'s 128-bit sum when it is a non-negative int64, else None."""
    lo, hi = int(res["value_lo"][a][g]), int(res["value_hi"][a][g])
    return lo if hi == 0 and lo >= 0 else None


def decode(typ: str, lo: int, hi: int, raw: Optional[bytes]):
    """A MIN / MAX cell as a Python value: integer kinds as int, date as days since the epoch, timestamp
    as microseconds, boolean as bool, float / double as float, decimal as decimal.Decimal, string as
    str, binary as bytes."""
    if typ == "string":
        return None if raw is None else raw.decode("utf-8", "surrogatepass")
    if typ == "binary":
        return raw
    if typ == "boolean":
        return bool(lo)
    if typ == "float":
        return struct.unpack("<f", struct.pack("<I", lo & 0xffffffff))[0]
    if typ == "double":
        return struct.unpack("<d", struct.pack("<q", lo))[0]
    if typ.startswith("decimal"):
        import decimal
        scale = type_code(typ) >> 16
        unscaled = (hi << 64) | (lo & ((1 << 64) - 1))
        return decimal.Decimal(unscaled).scaleb(-scale, decimal.Context(prec=60))
    return lo


def prove(P: Plan, res: Dict[str, "object"], allnull: Optional[Dict[int, Sequence[int]]] = None) -> List[List]:
    """Per group, the answer of every planned expression from a State.aggregate result `res` of
    P.specs, or None where the rules in this module's docstring do not prove it. `allnull[k][g]`: how
    many files of group g lack spec k's statistic and are proven to hold no non-NULL value of its
    column (missing: 0)."""
    out = []
    for g in range(len(res["group_rows"])):
        files = int(res["group_rows"][g])
        row = []
        for it in P.items:
            kind, ans = it[0], None
            if kind == "count_star":
                if int(res["nonnull"][it[1]][g]) == files:
                    ans = _sum64(res, it[1], g)
            elif kind == "count_part":
                nn = int(res["nonnull"][it[1]][g])
                if nn == 0:
                    ans = 0
                elif nn == files and int(res["nonnull"][it[2]][g]) == files:
                    ans = _sum64(res, it[2], g)
            elif kind == "count_data":
                if int(res["nonnull"][it[1]][g]) == files and int(res["nonnull"][it[2]][g]) == files:
                    n, z = _sum64(res, it[1], g), _sum64(res, it[2], g)
                    if n is not None and z is not None and z <= n:
                        ans = n - z
            elif kind in ("minmax_part", "minmax_data"):
                k, typ = it[1], it[2]
                nn = int(res["nonnull"][k][g])
                proven = kind == "minmax_part" or nn + int((allnull or {}).get(k, [0] * (g + 1))[g]) == files
                if nn and proven:
                    ans = decode(typ, int(res["value_lo"][k][g]), int(res["value_hi"][k][g]), res["strings"][k][g])
            row.append(ans)
        out.append(row)
    return out
