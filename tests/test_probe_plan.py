"""dr_state_probe_keys' host side without a device: check_probe_args / check_probe_rows of
delta_amd/csrc/pred_plan.cpp and the order map probe_order_key of delta_amd/csrc/filter_plan.h (the
function k_probe.hip calls) as a stand-alone program under ASan + UBSan -- every refusal with its status
and the index it names, the order map against Python's floats -- the binding's constants, and
Snapshot.files_for_keys' fallback where the bounds cannot decide, over a faked state."""
import math
import os
import random
import re
import struct
import subprocess

import numpy as np
import pytest

from delta_amd import _native as N
from tests import key_probe_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = [os.path.join(ROOT, "tests", "native", "probe_plan_host.cpp"), os.path.join(ROOT, "delta_amd", "csrc", "pred_plan.cpp")]
INVALID_ARG, UNSUPPORTED = 1, 12
STRING, BYTE, SHORT, INT, LONG, DATE, BOOLEAN, FLOAT, DOUBLE, TIMESTAMP, BINARY = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10
DEC = 11 | 12 << 8 | 2 << 16
src = lambda s, t: t | s << 24  # noqa: E731


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("probeplan") / "probe_plan_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", out] + SRCS)
    return out


def run(exe, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe], input=("\n".join(lines) + "\n").encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    assert r.returncode == 0, r.stderr.decode("utf-8", "replace")[-3000:]
    out = [(int(l.split("|", 1)[0]), l.split("|", 1)[1]) for l in r.stdout.decode("utf-8").splitlines()]
    assert len(out) == len(lines)
    return out


def _hex(name):
    return "0" if name is None else (name.encode("utf-8").hex() or "-")


def args(lo=(src(1, LONG), "id"), hi=(src(2, LONG), "id"), hasrows=0, nrows=0, haskeys=1, nkeys=1, flags=0):
    return "A %d %d %d %s %d %s %d %d %d" % (hasrows, nrows, lo[0], _hex(lo[1]), hi[0], _hex(hi[1]), haskeys, nkeys, flags)


def test_binding_names_the_kernels_constants():
    with open(os.path.join(ROOT, "delta_amd", "csrc", "kernels.h")) as f:
        text = f.read()
    for name in ("PROBE_BLOCK", "PROBE_GRID", "PROBE_TAB"):
        m = re.search(r"constexpr uint32_t %s = (\d+);" % name, text)
        assert m and int(m.group(1)) == getattr(N, name), name
    assert N.PROBE_TAB * 8 * 4 <= 160 * 1024  # four workgroups' tables within a CU's LDS
    assert set(("dr_state_probe_keys", "dr_probe_release")) <= set(N.OPTIONAL_SYMBOLS) <= set(N.SYMBOLS)
    assert N.OPTIONS["probe_search"] == 10


def test_refusals_with_status_and_text(exe):
    P = "dr_state_probe_keys: "
    cases = [
        (args(flags=4), INVALID_ARG, P + "flags = 4, not 0"),
        (args(hasrows=1, nrows=-2), INVALID_ARG, P + "nrows = -2 is negative"),
        (args(hasrows=1, nrows=2 ** 32), INVALID_ARG, P + "nrows = 4294967296 is above 4294967295"),
        (args(nkeys=-1), INVALID_ARG, P + "nkeys = -1 is outside 0..2147483647"),
        (args(nkeys=2 ** 31), INVALID_ARG, P + "nkeys = 2147483648 is outside 0..2147483647"),
        (args(haskeys=0, nkeys=3), INVALID_ARG, P + "keys == NULL with nkeys = 3"),
        (args(lo=(src(1, LONG), None)), INVALID_ARG, P + "lo needs a name"),
        (args(hi=(src(2, LONG), None)), INVALID_ARG, P + "hi needs a name"),
        (args(lo=(12, "p")), INVALID_ARG, P + "lo has no valid column type (code 12)"),
        (args(hi=(-1, "p")), INVALID_ARG, P + "hi has no valid column type (code -1)"),
        (args(lo=(src(1, LONG), "id"), hi=(src(2, INT), "id")), INVALID_ARG, P + "lo is of type 4 and hi of type 3; both bounds take one base type"),
        (args(lo=(LONG, "p"), hi=(TIMESTAMP, "p")), INVALID_ARG, P + "lo is of type 4 and hi of type 9; both bounds take one base type"),
        # what a predicate column of that source is refused for, "lo" / "hi" in the column's place
        (args(lo=(src(5, LONG), "id")), INVALID_ARG, "predicate column lo: unknown source 5 (DR_SRC_PARTITION .. DR_SRC_STATS_NUMRECORDS)"),
        (args(hi=(src(3, INT), "id")), INVALID_ARG, "predicate column hi: nullCount is a LONG, not type 3"),
        (args(hi=(src(4, LONG), "ab")), INVALID_ARG, 'predicate column hi: numRecords takes the name "", not a path of 2 bytes'),
        (args(lo=(src(1, LONG), "a\x01\x01b")), INVALID_ARG, "predicate column lo: segment 1 of the statistics path is empty"),
        (args(hi=(src(2, LONG), "\x01".join(["a"] * 9))), INVALID_ARG, "predicate column hi: a statistics path has at most 8 segments, not 9"),
        (args(lo=(src(1, LONG), "y" * 256)), INVALID_ARG, "predicate column lo: a statistics path has at most 255 bytes, not 256"),
        # the first offender is the one named: flags before keys, lo before hi
        (args(flags=1, nkeys=-1), INVALID_ARG, P + "flags = 1, not 0"),
        (args(lo=(12, "p"), hi=(13, "p")), INVALID_ARG, P + "lo has no valid column type (code 12)"),
    ]
    for typ in (STRING, BINARY, DEC, BOOLEAN):
        for s in (0, 1, 2):
            cases.append((args(lo=(src(s, typ), "x"), hi=(src(s, typ), "x")), UNSUPPORTED,
                          P + "lo is of type %d; STRING, BINARY, DECIMAL and BOOLEAN bounds are not probed" % (typ & 0xff)))
        cases.append((args(hi=(src(2, typ), "x")), UNSUPPORTED, P + "hi is of type %d; STRING, BINARY, DECIMAL and BOOLEAN bounds are not probed" % (typ & 0xff)))
    got = run(exe, [c[0] for c in cases])
    for (line, status, text), (rc, msg) in zip(cases, got):
        assert (rc, msg) == (status, text), line


def test_accepted_arguments(exe):
    lines = [args(lo=(src(1, t), "c"), hi=(src(2, t), "c")) for t in (BYTE, SHORT, INT, LONG, DATE, TIMESTAMP, FLOAT, DOUBLE)]
    lines += [args(lo=(t, "p"), hi=(t, "p")) for t in (BYTE, SHORT, INT, LONG, DATE, TIMESTAMP, FLOAT, DOUBLE)]
    lines += [args(lo=(LONG, "p"), hi=(src(2, LONG), "id")),                      # a partition bound beside a statistic
              args(lo=(src(3, LONG), "id"), hi=(src(4, LONG), "")),              # nullCount .. numRecords: both LONG
              args(haskeys=0, nkeys=0), args(nkeys=2 ** 31 - 1), args(hasrows=0, nrows=-7),   # nrows is ignored without rows
              args(hasrows=1, nrows=0), args(hasrows=1, nrows=2 ** 32 - 1), args(hasrows=0, nrows=2 ** 40), args(lo=(src(1, LONG), "a\x01b"), hi=(src(2, LONG), "a\x01b"))]
    assert run(exe, lines) == [(0, "")] * len(lines)


def test_rows_refusals_name_the_first_offender(exe):
    got = run(exe, ["R 10 3 0 9 10", "R 10 4 0 -1 99 5", "R 10 3 0 9 9", "R 10 0", "R 0 1 0"])
    P = "dr_state_probe_keys: "
    assert got == [(INVALID_ARG, P + "rows[2] = 10 is outside [0, 10)"), (INVALID_ARG, P + "rows[1] = -1 is outside [0, 10)"),
                   (0, ""), (0, ""), (INVALID_ARG, P + "rows[0] = 0 is outside [0, 0)")]


def _f32(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def _f64(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def _sql_cmp(a, b):
    """SQLOrderingUtil.compareDoubles / compareFloats: -0.0 = 0.0, NaN = NaN, NaN above everything."""
    if a != a or b != b:
        return (a != a) - (b != b)
    return (a > b) - (a < b)


@pytest.mark.parametrize("base", [FLOAT, DOUBLE])
def test_order_map_against_python_floats(exe, base):
    rng = random.Random(11)
    wide = base == DOUBLE
    nbits, dec = (64, _f64) if wide else (32, _f32)
    sign, inf = 1 << (nbits - 1), (0x7ff << 52) if wide else (0xff << 23)
    bits = [0, sign, 1, sign | 1, inf, sign | inf, inf - 1, sign | (inf - 1),             # +-0, subnormals, +-inf, the extremes
            inf | 1, sign | inf | 1, inf | (inf >> 1), (1 << nbits) - 1, inf | 12345, sign | inf | (1 << 20),   # NaN payloads
            (1 << (52 if wide else 23)), sign | (1 << (52 if wide else 23)), (1 << (52 if wide else 23)) - 1]
    bits += [rng.getrandbits(nbits) for _ in range(300)]
    words = [b - (1 << 64) if b >= 1 << 63 else b for b in bits]   # the int64 word (a float's bits zero-extended)
    keys = [int(m) for _, m in run(exe, ["K %d %d" % (base, w) for w in words])]
    vals = [dec(b) for b in bits]
    assert all(-(1 << 63) <= k < (1 << 63) for k in keys)
    for i in range(len(bits)):
        for j in range(len(bits)):
            c = _sql_cmp(vals[i], vals[j])
            assert ((keys[i] > keys[j]) - (keys[i] < keys[j])) == c, (hex(bits[i]), hex(bits[j]))
    nan = [k for k, v in zip(keys, vals) if v != v]
    assert len(set(nan)) == 1 and nan[0] > keys[4]                         # every NaN is one value above +Infinity
    assert keys[0] == keys[1] == 0                                         # -0.0 collapses onto 0.0
    # monotone over a sorted sample
    order = sorted((v for v in vals if v == v))
    ks = [int(m) for _, m in run(exe, ["K %d %d" % (base, R.signed64(struct.unpack("<Q", struct.pack("<d", v))[0]) if wide else
                                                   struct.unpack("<I", struct.pack("<f", v))[0]) for v in order])]
    assert ks == sorted(ks) and all((a == b) == (x == y) for a, b, x, y in zip(ks, ks[1:], order, order[1:]))
    if not wide:   # a FLOAT key's high 32 bits are not read
        assert run(exe, ["K 7 %d" % ((5 << 32) | 0x3fc00000), "K 7 %d" % 0x3fc00000])[0][1] == run(exe, ["K 7 %d" % 0x3fc00000])[0][1]


def test_order_map_leaves_the_integer_kinds_alone(exe):
    words = [0, -1, 1, -2 ** 63, 2 ** 63 - 1, 2 ** 31, -2 ** 31 - 1, 123456789012]
    for base in (BYTE, SHORT, INT, LONG, DATE, TIMESTAMP):
        assert [int(m) for _, m in run(exe, ["K %d %d" % (base, w) for w in words])] == words


# ---- Snapshot.files_for_keys where the bounds cannot decide: every file of the filter selection, no key_files ----
class _FakeState:
    """Stands in for delta_log.State: dr_filter and the exports, no device. A probe is an error."""
    def __init__(self, files, metadata):
        self.files = files
        self.counts = {"num_files": len(files), "size_in_bytes": 0, "num_removes": 0, "num_metadata": 1, "num_protocol": 1,
                       "num_set_transactions": 0}
        self.nonfile = [{"protocol": {"minReaderVersion": 1, "minWriterVersion": 2}}, {"metaData": metadata}]
        self.probes = []

    def export(self, which):
        return list(self.files)

    def export_rows_records(self, which, rows):
        return [self.files[r] for r in rows]

    def filter(self, program):
        return [i for i, f in enumerate(self.files) if f["partitionValues"]["p"] == "1"]

    def probe_keys(self, lo, hi, keys, key_null=None, rows=None):
        self.probes.append((lo, hi, [int(k) for k in keys], [int(z) for z in key_null], rows))
        sel = list(range(len(self.files))) if rows is None else list(rows)
        return {"selected": np.asarray(sel[:2], dtype=np.int64), "hits": np.ones(len(sel[:2]), dtype=np.int64),
                "key_files": np.arange(len(keys), dtype=np.int64), "unknown": 0}


def _snapshot():
    from delta_amd.delta_log import Snapshot
    F_, ST_ = R.F._F, R.F._ST
    schema = ST_([F_("id", "long"), F_("s", "string"), F_("ok", "boolean"), F_("amt", "decimal(10,2)"), F_("ts", "timestamp"),
                  F_("d", "double"), F_("blob", "binary"), F_("ID2", "long"), F_("id2", "long"), F_("p", "integer"), F_("ps", "string")])
    md = dict(R.METADATA, schemaString=__import__("json").dumps(schema), partitionColumns=["p", "ps"])
    files = [{"path": "f%d" % i, "partitionValues": {"p": str(i % 3), "ps": "x"}} for i in range(9)]
    st = _FakeState(files, md)
    return Snapshot(None, 0, st, 0), st


def test_files_for_keys_falls_back_without_a_wrong_skip():
    snap, st = _snapshot()
    flt = [("=", ("col", "p"), ("lit", "integer", 1))]
    for column, keys in (("s", ["a"]), ("ok", [True]), ("amt", [1]), ("blob", [b"x"]), ("ps", ["x"]),   # types the probe does not take
                         ("ts", [5]),                    # a timestamp statistic is truncated to milliseconds
                         ("d", [1.0, float("nan")]),     # float / double statistics ignore NaN rows
                         ("id2", [1]), ("nope", [1])):   # two leaves that differ in case only; no such column
        files, key_files = snap.files_for_keys(column, keys)
        assert key_files is None and files == st.files, column
        files, key_files = snap.files_for_keys(column, keys, filters=flt)
        assert key_files is None and files == [f for f in st.files if f["partitionValues"]["p"] == "1"], column
    assert st.probes == []


def test_files_for_keys_encodes_keys_and_passes_the_filter_rows():
    snap, st = _snapshot()
    files, key_files = snap.files_for_keys("ID", [7, None, -3, 2 ** 70], filters=[("=", ("col", "p"), ("lit", "integer", 1))])
    lo, hi, keys, nulls, rows = st.probes[-1]
    assert lo == (N.DR_SRC_STATS_MIN, ("id",), "long") and hi == (N.DR_SRC_STATS_MAX, ("id",), "long")
    assert keys == [7, 0, -3, 0] and nulls == [0, 1, 0, 1] and rows == [1, 4, 7]
    assert files == [st.files[1], st.files[4]] and list(key_files) == [0, 1, 2, 3]
    snap.files_for_keys("`P`", [1, 2])                       # a partition column: the same column twice
    lo, hi, keys, nulls, rows = st.probes[-1]
    assert lo == hi == (N.DR_SRC_PARTITION, "p", "integer") and keys == [1, 2] and rows is None
    snap.files_for_keys("d", [-0.0, math.inf, 2.5])
    assert st.probes[-1][2] == [-2 ** 63, 0x7ff0000000000000, 0x4004000000000000]
