"""Reference for dr_state_probe_keys (include/deltareplay.h): a brute-force evaluator written from the
header's "Meaning" paragraph -- every file against every distinct key, in Python integers and
struct-decoded floats, no bisection -- and a table of 1 500 live files whose statistics are steered to
the places the kernel can go wrong: ranges that are one key, end one below or start one above a key, lie
strictly between two keys, end at the first and last entry of the splitter table and of its segments,
cover everything, are empty (lo > hi), sit at the integer extremes, lack a bound, or have no statistics.
Nothing here calls the device. The conventions (_F, _ST, the commit layout) are filter_stats_corpus's."""
import datetime as dt
import json
import os
import struct

from delta_amd import _native as N
from delta_amd.testing import synth as S
from tests import filter_stats_corpus as F

MIN, MAX = N.DR_SRC_STATS_MIN, N.DR_SRC_STATS_MAX
I64_MIN, I64_MAX, I32_MIN, I32_MAX = -2 ** 63, 2 ** 63 - 1, -2 ** 31, 2 ** 31 - 1
TYPES = {"id": "long", "i": "integer", "sh": "short", "b": "byte", "dt": "date", "ts": "timestamp", "f": "float", "d": "double"}
SCHEMA = F._ST([F._F(c, t) for c, t in TYPES.items()] + [F._F("s", "string"), F._F("p", "integer"), F._F("q", "double")])
METADATA = {"id": "key-probe", "format": {"provider": "parquet", "options": {}},
            "schemaString": json.dumps(SCHEMA, separators=(",", ":")), "partitionColumns": ["p", "q"],
            "configuration": {}, "createdTime": 1600000000000}
N_ADDS, N_CKPT, N_TAIL, REMOVED = 1503, 700, 40, (701, 800, 1400)
N_LIVE = N_ADDS - len(REMOVED)
KEY_STEP = 10   # the long keys of the tests are KEY_STEP * j: room for ranges strictly between two of them


def long_keys(count):
    return [KEY_STEP * j for j in range(count)]


# the key slots whose neighbourhood the `id` ranges are steered to: the first keys, the edges of a wave, and
# the first / last entries of the splitter table (N.PROBE_TAB entries) and of its segments at the key
# counts where the segment length is 1, 2 and 3
EDGES = sorted(set([0, 1, 2, 3, 62, 63, 64, 65] + [e + d for e in (N.PROBE_TAB, 2 * N.PROBE_TAB) for d in (-3, -2, -1, 0, 1, 2)]))


def _id_ranges():
    out = [None, "absent", "{}", (None, 5), (5, None), (I64_MIN, I64_MIN), (I64_MAX, I64_MAX), (I64_MIN, I64_MAX),
           (I64_MIN, -1), (1, I64_MAX), (50, 40), (I64_MAX, I64_MIN), (-10 ** 9, 10 ** 9), (-500, -1)]
    top = KEY_STEP * 3 * N.PROBE_TAB
    for e in EDGES:
        k = KEY_STEP * e
        out += [(k, k), (k - 9, k - 1), (k + 1, k + 9), (k - 5, k), (k, k + 5), (0, k), (k, top), (k - 1, k + KEY_STEP), (k + 1, k - 1)]
    return out


ID_RANGES = _id_ranges()


def _iso_day(days):
    return (dt.date(1970, 1, 1) + dt.timedelta(days=days)).isoformat()


def _iso_ms(ms):
    t = dt.datetime(1970, 1, 1) + dt.timedelta(milliseconds=ms)
    return t.strftime("%Y-%m-%dT%H:%M:%S.") + "%03dZ" % (ms % 1000)


_FP_SPECIAL = [("NaN", "NaN"), (1.5, "NaN"), ("-Infinity", "Infinity"), ("-Infinity", "-Infinity"), ("Infinity", "Infinity"),
               (-0.0, -0.0), (0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), ("NaN", 1.0), (2.5, 2.5), (-1.25, -0.0), ("Infinity", "NaN")]
_INT_SPECIAL = [(I32_MIN, I32_MIN), (I32_MAX, I32_MAX), (I32_MIN, I32_MAX), (5, 3), (0, 0), (-1, 1)]


def stats_of(i):
    """The stats string of add i (None: no stats member)."""
    r = ID_RANGES[i] if i < len(ID_RANGES) else ((i * 7919) % 90000 - 2000, (i * 7919) % 90000 - 2000 + (i % 13) * (i % 29))
    if r is None or r == "absent":
        return None
    if r == "{}":
        return "{}"
    mn, mx = {}, {}
    if r[0] is not None:
        mn["id"] = r[0]
    if r[1] is not None:
        mx["id"] = r[1]
    a, b = _INT_SPECIAL[i % 97] if i % 97 < len(_INT_SPECIAL) else ((i * 37) % 2000 - 1000, (i * 37) % 2000 - 1000 + i % 50)
    mn["i"], mx["i"] = a, b
    mn["sh"], mx["sh"] = (i * 7) % 600 - 300, (i * 7) % 600 - 300 + i % 9
    mn["b"], mx["b"] = i % 200 - 100, min(127, i % 200 - 100 + i % 5)
    mn["dt"], mx["dt"] = _iso_day(18000 + i % 400), _iso_day(18000 + i % 400 + i % 3)
    mn["ts"], mx["ts"] = _iso_ms(1600000000000 + 1000 * (i % 500)), _iso_ms(1600000000000 + 1000 * (i % 500) + 250 * (i % 7))
    fa, fb = _FP_SPECIAL[i % 101] if i % 101 < len(_FP_SPECIAL) else ((i % 64) / 4.0 - 8, (i % 64) / 4.0 - 8 + (i % 5) * 0.25)
    mn["f"], mx["f"] = fa, fb
    da, db = _FP_SPECIAL[i % 103] if i % 103 < len(_FP_SPECIAL) else ((i % 640) / 8.0 - 40, (i % 640) / 8.0 - 40 + (i % 9) * 0.125)
    mn["d"], mx["d"] = da, db
    if i % 17 == 3:
        del mn["i"], mx["sh"], mn["f"], mx["d"], mn["dt"], mx["ts"], mn["b"]
    mn["s"], mx["s"] = "a%d" % i, "b%d" % i
    return json.dumps({"numRecords": 10 + i % 5, "minValues": mn, "maxValues": mx}, separators=(",", ":"))


_Q = ["NaN", "-0.0", "0.0", "Infinity", "-Infinity", "1.5", "-2.25", None]


def _add(i):
    a = {"path": "k-%05d.parquet" % i, "partitionValues": {"p": None if i % 11 == 0 else str(i % 7 - 2), "q": _Q[i % len(_Q)]},
         "size": 10 + i, "modificationTime": 1600000000000 + i, "dataChange": True}
    s = stats_of(i)
    if s is not None:
        a["stats"] = s
    return a


def live_files():
    return [_add(i) for i in range(N_ADDS) if i not in REMOVED]


def build(table_dir, checkpoint):
    """The _delta_log path: v0 (protocol, metadata, 700 adds; with `checkpoint` also a checkpoint of v0), v1,
    and v2 -- the last 40 adds and the removes -- which a test applies on top of the v1 state."""
    log = os.path.join(table_dir, "_delta_log")
    os.makedirs(log, exist_ok=True)
    line = lambda a: json.dumps(a, separators=(",", ":"))  # noqa: E731
    cuts = [(0, N_CKPT), (N_CKPT, N_ADDS - N_TAIL), (N_ADDS - N_TAIL, N_ADDS)]
    for v, (lo, hi) in enumerate(cuts):
        with open(os.path.join(log, "%020d.json" % v), "w", encoding="utf-8") as f:
            if v == 0:
                f.write(line({"protocol": F.PROTOCOL}) + "\n" + line({"metaData": METADATA}) + "\n")
            if v == 2:
                for r in REMOVED:
                    f.write(line({"remove": {"path": "k-%05d.parquet" % r, "deletionTimestamp": 1600000001000, "dataChange": True}}) + "\n")
            for i in range(lo, hi):
                f.write(line({"add": _add(i)}) + "\n")
    if checkpoint:
        adds = [_add(i) for i in range(N_CKPT)]
        S.write_checkpoint_records(os.path.join(log, "%020d.checkpoint.parquet" % 0), F.PROTOCOL, METADATA, adds, row_group_size=250)
        with open(os.path.join(log, "_last_checkpoint"), "w") as f:
            f.write('{"version":0,"size":%d}\n' % (len(adds) + 2))
    return log


# ---- the evaluator --------------------------------------------------------------------------------------
def signed64(u):
    return u - (1 << 64) if u >= 1 << 63 else u


def order(typ, word):
    """An int64 word in dr_state_stats_column's encoding as a Python value that compares as the header says:
    integers as they are (plain ints: the evaluator compares every file with every key, and ints compare
    several times faster than tuples); FLOAT / DOUBLE decoded with struct, every NaN one value above
    +Infinity, and -0.0 == 0.0 as Python's floats compare anyway. One call of evaluate() has one type."""
    if typ == "float":
        x = struct.unpack("<f", struct.pack("<I", word & 0xffffffff))[0]
    elif typ == "double":
        x = struct.unpack("<d", struct.pack("<q", word))[0]
    else:
        return word
    return (1, 0.0) if x != x else (0, x)


def stat_word(add, source, column):
    """The bound as dr_state_stats_column reports it (an int64 word), None for NULL: filter_stats_corpus's
    typed() over the add's stats string."""
    t = F.typed(add.get("stats"), source, (column,), TYPES[column])
    return None if t is None else t[0]


def evaluate(typ, bounds, lo_stats, hi_stats, keys, key_null=None, rows=None):
    """The dr_probe_result of the header's Meaning. bounds[r] = (lo word or None, hi word or None) of live
    position r; lo_stats / hi_stats: that bound is a statistics source; keys: int64 words. Returns
    (selected, hits, unknown, key_files) as lists. Files x keys comparisons: 8 194 keys against the 1 500 files
    take about 0.4 s, and all calls of tests/test_gpu_probe_keys.py together about 4 s of one CPU core."""
    sel_rows = list(range(len(bounds))) if rows is None else [int(r) for r in rows]
    live_keys = [(order(typ, k), i) for i, k in enumerate(keys) if not (key_null is not None and key_null[i])]
    # distinct under the order: (0, -0.0) and (0, 0.0) hash and compare equal, and so do all (1, 0.0)
    distinct = list(dict.fromkeys(o for o, _ in live_keys))
    cover = dict.fromkeys(distinct, 0)
    memo = {}
    selected, hits, unknown = [], [], 0
    for r in sel_rows:
        lo, hi = bounds[r]
        if (lo is None and lo_stats) or (hi is None and hi_stats):
            selected.append(r)
            hits.append(-1)
            unknown += 1
            continue
        if lo is None or hi is None:
            continue
        if r not in memo:
            a, b = order(typ, lo), order(typ, hi)
            memo[r] = [k for k in distinct if a <= k and k <= b]
        inside = memo[r]
        for k in inside:
            cover[k] += 1
        if inside:
            selected.append(r)
            hits.append(len(inside))
    key_files = [0] * len(keys)
    for o, i in live_keys:
        key_files[i] = cover[o]
    return selected, hits, unknown, key_files
