"""Expected results of dr_state_aggregate as a plain-Python fold over exported records (the files of
tests/filter_stats_corpus.py): F.typed for statistics, a cast of partitionValues["p"] for the partition
column. The order is Python's own -- ints, bytes -- and for float / double the rule of SQLOrderingUtil
written out below. Nothing here calls the device."""
import struct

from delta_amd import _native as N
from tests import filter_stats_corpus as F

M64 = (1 << 64) - 1


def s64(u):
    u &= M64
    return u - (1 << 64) if u >= 1 << 63 else u


def fp_order(bits, typ):
    """The order of a float / double from its bits: NaN = NaN, NaN above +Infinity, -0.0 = 0.0."""
    v = struct.unpack("<f", struct.pack("<I", bits & 0xffffffff))[0] if typ == "float" else struct.unpack("<d", struct.pack("<Q", bits & M64))[0]
    return (1, 0.0) if v != v else (0, v + 0.0)  # (Python compares -0.0 == 0.0)


def cell(typ, t):
    """(order key, value_lo, value_hi, bytes) of a non-NULL F.typed value t."""
    if typ in ("float", "double"):
        return fp_order(t[0], typ), s64(t[0]), 0, None
    if typ.startswith("decimal"):
        return t[1], s64(t[1]), t[1] >> 64, None
    if typ == "string":
        return t[1], 0, 0, t[1]
    return t[0], t[0], t[0] >> 63, None


_TYPED = {}  # (source, path, type, stats string) -> input: the reference is computed once and shared


def stats_input(src, path, typ):
    """agg_spec tail and the per-file input of a statistics column."""
    def get(f):
        key = (src, tuple(path), typ, f["stats"])
        if key not in _TYPED:
            t = F.typed(f["stats"], src, path, typ)
            _TYPED[key] = None if t is None else cell(typ, t)
        return _TYPED[key]
    return (src, tuple(path), typ), get


def partition_input():
    return (N.DR_SRC_PARTITION, "p", "integer"), lambda f: cell("integer", (int(f["partitionValues"]["p"]),) * 2)


def builtin_input(which):
    field = {"size": "size", "mtime": "modificationTime"}[which]
    return (which,), lambda f: cell("long", (f[field],) * 2)


def fold(fn, get, live, rows, off):
    """Per group (nonnull, value_lo, value_hi, arg_row, bytes) of `fn` over selection `rows` (None: all)
    cut by `off` (None: one group)."""
    rows = list(range(len(live))) if rows is None else list(rows)
    off = [0, len(rows)] if off is None else list(off)
    out = []
    for g in range(len(off) - 1):
        pos = range(off[g], off[g + 1])
        vals = [(q, get(live[rows[q]])) for q in pos]
        vals = [(q, v) for q, v in vals if v is not None]
        if fn == "count" or (fn == "sum" and not vals):
            out.append((len(vals), 0, 0, -1, None))
        elif fn == "sum":
            total = sum(v[0] for _, v in vals) % (1 << 128)
            out.append((len(vals), s64(total), s64(total >> 64), -1, None))
        elif not vals:
            out.append((0, 0, 0, -1, None))
        else:
            best = (min if fn == "min" else max)(v[0] for _, v in vals)
            q, v = next((q, v) for q, v in vals if v[0] == best)  # the first position attaining it
            out.append((len(vals), v[1], v[2], rows[q], v[3]))
    return out


def compare(res, a, want, what):
    """Spec a of a State.aggregate result against fold()'s groups."""
    got = [(int(res["nonnull"][a][g]), int(res["value_lo"][a][g]), int(res["value_hi"][a][g]), int(res["arg_row"][a][g]),
            res["strings"][a][g]) for g in range(len(want))]
    assert got == want, (what, [(g, x, y) for g, (x, y) in enumerate(zip(got, want)) if x != y][:4])
