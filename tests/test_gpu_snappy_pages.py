"""SNAPPY checkpoint pages the project's compressor never writes, on the device (k_snappy.hip). One table
(config 3 at scale 0.001, seed 3, plain pages: its add.path page holds 15 fragments of 64 KiB) is built once
and the oracle reads it once; each case copies the log and replaces page bodies (tests/lz4_corpus.rewrite) by
bodies built here from the page's own bytes with the steered compressor of tests/snappy_corpus.py. What a kind
is named for is asserted on the elements of the body that is sent. Every case runs under DR_SNAP_DEBUG=1 and
reads the engine's report of how many pages went to the serial decoder:

 (a) legal forms inside the writers' fragment rules decode on the parallel path (bad 0);
 (b) legal pages the documented rules send to k_snap_serial are reported as exactly those pages, and replay
     to the same state, twice from one staged log;
 (c) one malformed body per refusal (tests/test_snappy_host.MALFORMED, each refused by the host decoder under
     the sanitizers first) ends in DR_E_PARQUET, and a good table replays afterwards;
 (d) a crafted tag-3 SNAPPY chunk among GZIP, ZSTD and LZ4 chunks.

Pages of sizes the base table does not have come from tables of their own, whose twin as pyarrow wrote it gives
the state: add.stats padded to exactly 4 * 65536 and to 65537 bytes, and remove.extendedFileMetadata of 8 to
40 retained removes in DATA_PAGE_V2 pages (1 to 5 bytes behind the levels), whose flags export(1) hands back.
A page of 1 byte can hold no copy, so it is one literal, which the planner copies: k_snap_exec cannot be
reached with it."""
import os
import re
import shutil

import pytest

from oracle import delta_oracle as O
from tests import snappy_corpus as S
from tests.test_gpu_parity import _assert_same
from tests.test_snappy_host import MALFORMED, malformed_bodies

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = S.FRAGMENT


def _kernel_constant(name):
    src = open(os.path.join(ROOT, "delta_amd", "csrc", "k_snappy.hip")).read()
    return int(re.search(r"#define %s (\d+)" % name, src).group(1))


EMAX, CH, WG = _kernel_constant("DR_EXEC_EMAX"), _kernel_constant("DR_SNAP_CH"), _kernel_constant("DR_SNAP_WG_CHUNKS")
LONG_LEN, LONG = _kernel_constant("DR_EXEC_LONG_LEN"), 256
assert re.search(r"constexpr uint32_t EXEC_LONG = 256;", open(os.path.join(ROOT, "delta_amd", "csrc", "k_snappy.hip")).read())


@pytest.fixture(scope="module")
def engine():
    from delta_amd.delta_log import Engine
    return Engine.get(0)


def _replay(engine, lp, cutoff):
    staged = engine.stage_log(lp)
    try:
        return staged.replay(cutoff), staged.plan()
    finally:
        staged.release()


def _report(err):
    """(pages, bad, {code: pages}, exec phases seen, [(n_in, n_out) of the bad pages, up to three per code]) of
    the DR_SNAP_DEBUG lines."""
    tot = [(int(a), int(b)) for a, b in re.findall(r"snappy: pages (\d+), pages with serially resolved regions \d+, bad (\d+)", err)]
    codes = {}
    for c, n in re.findall(r"snappy bad code (\d+): (\d+) pages", err):
        codes[int(c)] = codes.get(int(c), 0) + int(n)
    which = sorted((int(a), int(b)) for a, b in re.findall(r"snappy bad page \d+ code \d+: n_in (\d+) n_out (\d+)", err))
    return sum(a for a, _ in tot), sum(b for _, b in tot), codes, "exec phases" in err, which


@pytest.fixture(scope="module")
def base(tmp_path_factory, engine):
    """(log path, checkpoint file name, checkpoint as a table, cutoff, oracle snapshot, export(0), export(1),
    plan) of the untouched table."""
    import pyarrow.parquet as pq
    from delta_amd.testing import synth as Sy
    d = str(tmp_path_factory.mktemp("snappy_base"))
    exp = Sy.build_table(d, Sy.config_spec(3, 0.001), seed=3, use_dictionary=False)
    lp = os.path.join(d, "_delta_log")
    ck = [f for f in os.listdir(lp) if f.endswith(".checkpoint.parquet")]
    assert len(ck) == 1
    cutoff = exp.min_file_retention_timestamp
    snap = O.state_reconstruction(O.get_log_segment(lp), cutoff)
    st, plan = _replay(engine, lp, cutoff)
    try:
        _assert_same(st, snap)
        live, dead = st.export(0), st.export(1)
    finally:
        st.release()
    return lp, ck[0], pq.read_table(os.path.join(lp, ck[0])), cutoff, snap, live, dead, plan


def _page(ck, leaf, k=0):
    """(the page's bytes, decoded with the reference; its body)"""
    at, c, u = S.snappy_pages(ck, leaf)[k]
    body = open(ck, "rb").read()[at:at + c]
    data = S.reference(body, u)
    assert data is not None and len(data) == u
    return data, body


def _staged_copy(base, d, bodies):
    lp = os.path.join(str(d), "_delta_log")
    shutil.copytree(base[0], lp)
    ck = os.path.join(lp, base[1])
    S.rewrite(ck, ck, {key: (1, body) for key, body in bodies.items()})
    return lp


def _check(engine, base, lp, capfd, monkeypatch, want=None):
    """Replays `lp`: the oracle's state, the untouched table's exports. Returns (report, plan). want: the
    state to compare with instead (export(0), export(1)) for a table with other contents."""
    monkeypatch.setenv("DR_SNAP_DEBUG", "1")
    capfd.readouterr()
    st, plan = _replay(engine, lp, base[3])
    try:
        if want is None:
            _assert_same(st, base[4])
        live, dead = want or (base[5], base[6])
        assert st.export(0) == live and st.export(1) == dead
    finally:
        st.release()
    return _report(capfd.readouterr().err), plan


def _fragments(data):
    return [data[k:k + F] for k in range(0, len(data), F)]


def _per_fragment(data, special):
    """Elements of `data`: fragment k from special[k](fragment) where given, else the plain compressor."""
    out = []
    for k, frag in enumerate(_fragments(data)):
        out += special[k](frag) if k in special else S.compress(frag)
    return out


def _copies(el):
    return [e for e in el if e[0] == "copy"]


def _lits(el):
    return [e for e in el if e[0] == "lit"]


def _steer(elements, boundaries):
    """`elements` with literal length fields widened so that, for the k-th position B of `boundaries` (input
    positions behind the preamble), a tag-3 copy's 5-byte header starts at B - (5 - k % 5): it ends exactly at
    B (phase 0) or straddles it with 4, 3, 2 or 1 bytes in front (phases 1 to 4)."""
    el = list(elements)
    starts, pos = [], 0                       # input positions before any widening
    for e in el:
        starts.append(pos)
        pos += len(S.encode_element(e))
    shift, lo = 0, 0                          # bytes added so far: all of them in front of el[lo:]
    for k, B in enumerate(boundaries):
        T = B - (5 - k % 5)
        j = max(i for i in range(lo, len(el)) if el[i][0] == "copy" and el[i][3] == 4 and starts[i] + shift <= T)
        need = T - (starts[j] + shift)
        shift += need
        i = j - 1
        while need and i >= lo:
            if el[i][0] == "lit":
                nb = max(el[i][2], S.min_nb(len(el[i][1])))
                add = min(need, 4 - nb)
                if add > 0:
                    el[i] = ("lit", el[i][1], nb + add)
                    need -= add
            i -= 1
        assert need == 0
        lo = j + 1
    return el


def _range_elements(body, block):
    """(elements, input bytes) k_snap_exec counts for output block `block`. This restates the kernel's steps 0
    and 1 (k_snappy.hip, k_snap_exec: the chunk range [block_chunk[b], block_chunk[b + 1] + 1) and the start
    bits kept in it): the element starts in the speculation chunks from the one holding the block's first
    element to the one holding the next block's first element. If the kernel counts otherwise one day, the
    EXEC_EMAX cases below no longer sit on the limit: change both together."""
    lay = S.layout(body)[0]
    first, op = {}, 0
    for ip, hdr, e in lay:
        if op % F == 0:
            first[op // F] = ip
        op += len(e[1]) if e[0] == "lit" else e[2]
    lo = first[block] // CH * CH
    hi = (first[block + 1] // CH + 1) * CH if block + 1 in first else 1 << 40
    return sum(lo <= ip < hi for ip, _, _ in lay), min(hi, lay[-1][0] + 1) - lo


# ---- (a) inside the fragment rules: the parallel path ---------------------------------------------------
def _a_tag3(data):
    el = S.compress(data, kinds=(4,))
    enc = S.encode(el)
    n_in = len(enc) - S.preamble_of(enc)[1]
    el = _steer(el, list(range(WG * CH, n_in - 4096, WG * CH)))
    lay = S.layout(S.encode(el))[0]
    assert {e[3] for e in _copies(el)} == {4} and len(_copies(el)) > 50000
    heads = [ip for ip, hdr, e in lay if e[0] == "copy"]
    # 5-byte headers at every phase of a chunk end, and of a workgroup's end: ending on it (0), 1..4 bytes behind it
    for unit in (CH, WG * CH):
        phases = {(ip + 5) % unit for ip in heads if (ip + 5) % unit < 5}
        assert phases == {0, 1, 2, 3, 4}, (unit, phases)
    assert len([ip for ip in heads if ip // (WG * CH) != (ip + 4) // (WG * CH)]) >= 10
    return el


def _a_tag2(data):
    el = S.compress(data, kinds=(2,))
    assert {e[3] for e in _copies(el)} == {2}
    assert {e[2] for e in _copies(el) if e[1] < 2048} >= set(range(4, 12))
    return el


def _a_lit_nb(nb):
    def build(data):
        el = S.compress(data, lit_nb=nb)
        assert all(e[2] == max(nb, S.min_nb(len(e[1]))) for e in _lits(el))
        assert sum(len(e[1]) == 1 and e[2] == nb for e in _lits(el)) > 100
        # the length field across chunk ends, cut at each of its bytes
        cuts = {CH - ip % CH for ip, hdr, e in S.layout(S.encode(el))[0] if e[0] == "lit" and hdr == 1 + nb and ip % CH + hdr > CH}
        assert cuts == set(range(1, nb + 1)), cuts
        return el
    return build


def _a_literal_lengths(data):
    sizes = (60, 61, 64, 65, 256, 257, 65536)

    def one(n):
        return lambda f: S.compress(f[:1000]) + S.literal(f[1000:1000 + n]) + S.compress(f[1000 + n:]) if n < F else S.literal(f)
    el = _per_fragment(data, {k + 1: one(n) for k, n in enumerate(sizes)})
    sp = S.spans(el)
    for k, n in enumerate(sizes):
        assert any(e[0] == "lit" and ln == n and op // F == k + 1 for op, ln, e in sp), n
    assert any(e[0] == "lit" and ln == F and op == 7 * F for op, ln, e in sp)     # a whole fragment, between compressed ones
    return el


def _a_copy_lengths(data):
    def short(n):
        return lambda f: S.compress(f[:30000]) + S.compress(f[30000:34000], kinds=(2, 4), min_copy=n, max_copy=n) + S.compress(f[34000:])
    el = _per_fragment(data, {1: short(1), 2: short(2), 3: short(3), 4: lambda f: S.compress(f, kinds=(4,), min_copy=1, max_copy=3, key=3)})
    n = {k: sum(e[2] == k for e in _copies(el)) for k in (1, 2, 3)}
    assert min(n.values()) > 100 and any(e[2] < 4 and e[3] == 4 for e in _copies(el)), n
    return el


def _a_far_offsets(data):
    """The largest offset a position allows: a copy of the fragment's first bytes, at every place they recur."""
    def build(f):
        out, at, i = [], 0, f.find(f[:1], 1)
        while i > 0:
            n = 1
            while n < 64 and i + n < len(f) and f[n] == f[i + n]:
                n += 1
            out += S.compress(f[at:i]) + [("copy", i, n, 2)]
            at = i + n
            i = f.find(f[:1], max(at, i + 2000))
        return out + S.compress(f[at:])
    el = _per_fragment(data, {k: build for k in range(len(data) // F)})
    top = [(op, e) for op, _, e in S.spans(el) if e[0] == "copy" and e[1] == op % F]
    assert len(top) > 100 and max(e[1] for _, e in top) > 60000
    return el


def _a_emax(extra):
    def build(data):
        n1 = EMAX * 1024 - 2 + extra     # one-byte literals; with the long one behind them and the next block's first
        def block0(f):                   # element the chunk range holds EMAX * 1024 (+ extra) elements
            return [("lit", f[k:k + 1], 0) for k in range(n1)] + S.literal(f[n1:])
        el = _per_fragment(data, {0: block0, 1: lambda f: S.literal(f[:300]) + S.compress(f[300:])})
        body = S.encode(el)
        count, span = _range_elements(body, 0)
        assert count == EMAX * 1024 + extra and span + 24 < 2 * F, (count, span)
        return el
    return build


def _a_long_literals(data):
    el = _per_fragment(data, {2: lambda f: S.compress(f, kinds=(4,), min_lit=LONG_LEN + 1)})
    n = sum(e[0] == "lit" and ln > LONG_LEN and op // F == 2 for op, ln, e in S.spans(el))
    assert n > LONG + 50 and {e[3] for op, _, e in S.spans(el) if e[0] == "copy" and op // F == 2} == {4}, n
    return el


A_KINDS = {
    "every copy tag 3, headers across chunk and workgroup ends": (_a_tag3, {}),
    "every copy tag 2": (_a_tag2, {}),
    "literals in 1 length byte": (_a_lit_nb(1), {}),
    "literals in 2 length bytes": (_a_lit_nb(2), {}),
    "literals in 3 length bytes": (_a_lit_nb(3), {}),
    "literals in 4 length bytes": (_a_lit_nb(4), {}),
    "literals of 60, 61, 64, 65, 256, 257 and 65536": (_a_literal_lengths, {}),
    "copies of 1, 2 and 3": (_a_copy_lengths, {}),
    "offset equal to the position in the fragment": (_a_far_offsets, {}),
    "a block of EXEC_EMAX * 1024 elements": (_a_emax(0), {}),
    "more long literals than the queue holds": (_a_long_literals, {}),
    "5-byte preamble": (lambda data: S.compress(data), {"preamble": 5}),
}


@pytest.mark.parametrize("kind", sorted(A_KINDS))
def test_legal_forms_inside_the_fragment_rules_decode_in_parallel(engine, base, tmp_path, capfd, monkeypatch, kind):
    build, kw = A_KINDS[kind]
    data, old = _page(os.path.join(base[0], base[1]), "add.path")
    assert len(data) > 14 * F
    el = build(data)
    body = S.encode(el, **kw)
    assert S.keeps_fragments(el) and S.reference(body, len(data)) == data and S.pyarrow_decode(body, len(data)) == data
    # an element ends exactly on every fragment end, and the body has the writers' 3-byte preamble unless the kind pads it
    assert S.preamble_of(body)[1] == kw.get("preamble", 3)
    lp = _staged_copy(base, tmp_path, {("add.path", 0): body})
    (pages, bad, codes, phases, _), plan = _check(engine, base, lp, capfd, monkeypatch)
    assert pages > 1 and bad == 0 and not codes and phases, (pages, bad, codes)
    # the page is decoded, not copied by the planner's literals-only shortcut
    grew = (len(body) - S.preamble_of(body)[1]) - (len(old) - S.preamble_of(old)[1])
    assert plan["snappy_in_bytes"] == base[7]["snappy_in_bytes"] + grew
    assert plan["snappy_out_bytes"] == base[7]["snappy_out_bytes"]


def _periodic_table(table):
    """The checkpoint with add.stats replaced: every row's stats has 251 bytes (a record of 255 with its length
    prefix, which divides 65535) and holds runs of "q", "ab" and "xyz", each longer than a wave."""
    import pyarrow as pa
    col = table.schema.get_field_index("add")
    add = table.column(col).combine_chunks()
    valid = add.is_valid().to_pylist()
    row = '{"numRecords":%07d,"tags":"' + "q" * 70 + "ab" * 35 + "xyz" * 26 + "-" + '"}'
    assert len(row % 0) == 251
    stats = pa.array([row % i if v else None for i, v in enumerate(valid)], pa.string())
    k = add.type.get_field_index("stats")
    children = [stats if j == k else add.field(j) for j in range(add.type.num_fields)]
    new = pa.StructArray.from_arrays(children, fields=list(add.type), mask=pa.array([not v for v in valid]))
    return table.set_column(col, table.schema.field(col), new)


def test_short_periods_and_offset_65535(engine, base, tmp_path, capfd, monkeypatch):
    """A table of its own (add.stats holds runs of one, two and three bytes and repeats every 255 bytes): its
    twin as pyarrow wrote it gives the state; the crafted page holds overlapping copies of 64 bytes at offsets
    1, 2 and 3 and copies at offset 65535, the largest tag 2 holds."""
    import pyarrow.parquet as pq
    lp0 = os.path.join(str(tmp_path), "twin", "_delta_log")
    shutil.copytree(base[0], lp0)
    pq.write_table(_periodic_table(base[2]), os.path.join(lp0, base[1]), compression="snappy", use_dictionary=False,
                   version="1.0", write_statistics=False)
    st, _ = _replay(engine, lp0, base[3])
    try:
        want = (st.export(0), st.export(1))
    finally:
        st.release()
    assert sum("q" * 70 + "ab" * 35 in (a.get("stats") or "") for a in want[0]) > 1000
    twin = (lp0,) + base[1:]
    data, _ = _page(os.path.join(lp0, base[1]), "add.stats")
    assert len(data) > 4 * F
    el = _per_fragment(data, {0: lambda f: S.compress(f, kinds=(2,), offsets=(1, 2, 3)),
                              1: lambda f: S.compress(f, kinds=(4,), offsets=(1, 2, 3)),
                              2: lambda f: S.compress(f[:65535], kinds=(2,), offsets=(255,)) + [("copy", 65535, 1, 2)],
                              3: lambda f: S.compress(f[:65500], kinds=(2,), offsets=(255,)) + S.literal(f[65500:65535]) + [("copy", 65535, 1, 4)]})
    for off in (1, 2, 3):
        assert {e[3] for e in _copies(el) if e[1] == off and e[2] == 64} == {2, 4}, off
    assert [e[3] for e in _copies(el) if e[1] == 65535] == [2, 4]
    body = S.encode(el)
    assert S.keeps_fragments(el) and S.reference(body, len(data)) == data and S.pyarrow_decode(body, len(data)) == data
    lp = _staged_copy(twin, tmp_path / "crafted", {("add.stats", 0): body})
    (pages, bad, codes, phases, _), _ = _check(engine, twin, lp, capfd, monkeypatch, want=want)
    assert pages > 1 and bad == 0 and phases, (pages, bad, codes)


def _add_leaf(table, name, values):
    """The checkpoint with leaf `name` of add set to values(valid) (appended when add has no such leaf)."""
    import pyarrow as pa
    col = table.schema.get_field_index("add")
    add = table.column(col).combine_chunks()
    valid = add.is_valid().to_pylist()
    arr = values(valid)
    k = add.type.get_field_index(name)
    children = [arr if j == k else add.field(j) for j in range(add.type.num_fields)] + ([arr] if k < 0 else [])
    fields = list(add.type) + ([pa.field(name, arr.type)] if k < 0 else [])
    new = pa.StructArray.from_arrays(children, fields=fields, mask=pa.array([not v for v in valid]))
    return table.set_column(col, pa.field("add", new.type), new)


def _twin(engine, base, d, table, capfd, monkeypatch, **kw):
    """A copy of the log whose checkpoint is `table` as pyarrow writes it: (base tuple of the twin, its exports,
    the pages its replay and exports report)."""
    import pyarrow.parquet as pq
    lp0 = os.path.join(str(d), "_delta_log")
    shutil.copytree(base[0], lp0)
    pq.write_table(table, os.path.join(lp0, base[1]), compression="snappy", use_dictionary=False, version="1.0",
                   write_statistics=False, **kw)
    monkeypatch.setenv("DR_SNAP_DEBUG", "1")
    capfd.readouterr()
    st, _ = _replay(engine, lp0, base[3])
    try:
        want = (st.export(0), st.export(1))
    finally:
        st.release()
    pages, bad, _, _, _ = _report(capfd.readouterr().err)
    assert bad == 0
    return (lp0,) + base[1:], want, pages


def _sized_stats(base, d, target, row='{"numRecords":%07d}'):
    """The checkpoint table whose add.stats page (plain, levels included) has exactly `target` bytes: short
    stats, one row padded by what is missing."""
    import pyarrow as pa
    import pyarrow.parquet as pq

    def table(pad):
        first = []

        def values(valid):
            out = []
            for i, v in enumerate(valid):
                mine = v and not first
                if mine:
                    first.append(i)
                out.append(None if not v else (row % i if "%" in row else row) + " " * (pad if mine else 0))
            return pa.array(out, pa.string())
        return _add_leaf(base[2], "stats", values)
    probe = os.path.join(str(d), "probe.parquet")
    pq.write_table(table(0), probe, compression="snappy", use_dictionary=False, version="1.0", write_statistics=False)
    (_, _, u), = S.snappy_pages(probe, "add.stats")
    assert u <= target
    return table(target - u)


def test_a_page_of_an_exact_multiple_of_65536(engine, base, tmp_path, capfd, monkeypatch):
    """add.stats of exactly 4 * 65536 bytes: the last block is a whole one, and an element ends on the page's end
    as on every fragment's. Copies under tag 3 in the last block."""
    twin, want, pages0 = _twin(engine, base, tmp_path / "twin", _sized_stats(base, tmp_path, 4 * F), capfd, monkeypatch)
    data, _ = _page(os.path.join(twin[0], twin[1]), "add.stats")
    assert len(data) == 4 * F
    el = _per_fragment(data, {3: lambda f: S.compress(f, kinds=(4,))})
    body = S.encode(el)
    assert S.keeps_fragments(el) and len(_copies(el)) > 1000 and S.reference(body, len(data)) == data
    lp = _staged_copy(twin, tmp_path / "crafted", {("add.stats", 0): body})
    (pages, bad, codes, phases, _), _ = _check(engine, twin, lp, capfd, monkeypatch, want=want)
    assert pages == pages0 > 1 and bad == 0 and not codes and phases, (pages, pages0, bad, codes)


def test_the_smallest_page_outside_the_rules(engine, base, tmp_path, capfd, monkeypatch):
    """add.stats of 65537 bytes, two blocks: its last element is a literal of 4 bytes across the fragment end.
    Every page reported is that one (once per decode of the leaf), and the state is the twin's."""
    twin, want, pages0 = _twin(engine, base, tmp_path / "twin", _sized_stats(base, tmp_path, F + 1, row="{}"), capfd, monkeypatch)
    data, _ = _page(os.path.join(twin[0], twin[1]), "add.stats")
    assert len(data) == F + 1
    el = S.compress(data[:F - 3]) + S.literal(data[F - 3:])
    body = S.encode(el)
    assert [(op, n, e[0]) for op, n, e in S.spans(el) if op // F != (op + n - 1) // F] == [(F - 3, 4, "lit")]
    assert len(_copies(el)) > 100 and S.reference(body, len(data)) == data and S.pyarrow_decode(body, len(data)) == data
    lp = _staged_copy(twin, tmp_path / "crafted", {("add.stats", 0): body})
    pages, bad, codes, phases, which = _twice(engine, twin, lp, capfd, monkeypatch, want=want)
    assert pages == pages0 and bad >= 1 and set(which) == {(len(body) - 3, F + 1)} and len(which) == bad and codes == {32: bad} \
        and phases, (pages, pages0, bad, codes, which)


def _with_removes(table, cutoff, flags):
    """The checkpoint with one retained remove per flag behind its rows: remove.extendedFileMetadata holds the
    flags, which export(1) hands back."""
    import pyarrow as pa
    n = len(flags)
    rtype = table.schema.field("remove").type
    rows = [{"path": "removed/part-%05d" % i, "deletionTimestamp": cutoff + 1000000 + i, "dataChange": False,
             "extendedFileMetadata": bool(f), "partitionValues": [("p1", str(i))], "size": 1000 + i, "tags": None}
            for i, f in enumerate(flags)]
    cols = [pa.array(rows, rtype) if f.name == "remove" else pa.nulls(n, f.type) for f in table.schema]
    return pa.concat_tables([table, pa.Table.from_arrays(cols, schema=table.schema)])


TINY = {
    # kind: (the page's bytes -- eight flags a byte, the first in bit 0 -- and the body's elements)
    "1 byte, one literal": (b"\xa5", [("lit", b"\xa5", 0)]),
    "1 byte, one literal in 4 length bytes": (b"\xa5", [("lit", b"\xa5", 4)]),
    "2 bytes, offset 1": (b"\xa5\xa5", [("lit", b"\xa5", 0), ("copy", 1, 1, 2)]),
    "3 bytes, offset 1": (b"\xa5" * 3, [("lit", b"\xa5", 0), ("copy", 1, 2, 2)]),
    "3 bytes, offset 2": (b"\xa5\x3c\xa5", [("lit", b"\xa5\x3c", 0), ("copy", 2, 1, 4)]),
    "4 bytes, offset 1": (b"\x3c" * 4, [("lit", b"\x3c", 1), ("copy", 1, 3, 4)]),
    "4 bytes, offset 2": (b"\xa5\x3c\xa5\x3c", [("lit", b"\xa5\x3c", 0), ("copy", 2, 2, 2)]),
    "5 bytes, offset 1": (b"\xa5" * 5, [("lit", b"\xa5", 0), ("copy", 1, 4, 1)]),
    "5 bytes, offset 2": (b"\xa5\x3c\xa5\x3c\xa5", [("lit", b"\xa5\x3c", 2), ("copy", 2, 3, 2)]),
    "5 bytes, offset 3": (b"\xa5\x3c\x0f\xa5\x3c", [("lit", b"\xa5\x3c\x0f", 0), ("copy", 3, 2, 2)]),
}


@pytest.mark.parametrize("kind", sorted(TINY))
def test_one_block_pages_of_one_to_five_bytes(engine, base, tmp_path, capfd, monkeypatch, kind):
    """remove.extendedFileMetadata of 8 n retained removes in DATA_PAGE_V2 pages: n bytes of mixed bits behind
    the levels, which pyarrow leaves uncompressed. Here compressed, with a copy wherever n allows one, through
    k_snap_exec's byte stores of a page's last block. export(1) hands the flags back: they must be the ones
    written, bit for bit, and the state the oracle's of this table. A page of 1 byte has no room for a copy: the
    literal, whatever its length field, is the planner's to copy."""
    page, el = TINY[kind]
    n = len(page)
    flags = [bool(page[i // 8] >> (i % 8) & 1) for i in range(8 * n)]
    assert 0 < sum(flags) < len(flags)
    monkeypatch.setenv("DR_SNAP_DEBUG", "1")
    twin, want, pages0 = _twin(engine, base, tmp_path / "twin", _with_removes(base[2], base[3], flags), capfd, monkeypatch,
                               data_page_version="2.0")
    ck = os.path.join(twin[0], twin[1])
    leaf = "remove.extendedFileMetadata"
    assert S.snappy_pages(ck, leaf) == []      # stored, not compressed
    body = S.encode(el)
    assert S.reference(body, n) == page and S.pyarrow_decode(body, n) == page and S.preamble_of(body) == (n, 1)
    assert (n == 1) == (not _copies(el))
    lp = os.path.join(str(tmp_path), "crafted", "_delta_log")
    shutil.copytree(twin[0], lp)
    S.rewrite(ck, os.path.join(lp, twin[1]), {(leaf, 0): (1, body)}, stored=(leaf,))
    (at, c, u), = S.snappy_pages(os.path.join(lp, twin[1]), leaf)
    assert (c, u) == (len(body), n)
    snap = O.state_reconstruction(O.get_log_segment(lp), base[3])
    capfd.readouterr()
    st, _ = _replay(engine, lp, base[3])
    try:
        _assert_same(st, snap)
        live, dead = st.export(0), st.export(1)
    finally:
        st.release()
    pages, bad, codes, phases, _ = _report(capfd.readouterr().err)
    got = {a["path"]: a["extendedFileMetadata"] for a in dead if a["path"].startswith("removed/part-")}
    assert [got["removed/part-%05d" % i] for i in range(8 * n)] == flags
    assert (live, dead) == want
    # one more page through the SNAPPY kernels than in the twin, unless it is the planner's copy
    assert pages == pages0 + (n > 1) and bad == 0 and not codes and phases, (pages, pages0, bad, codes)


def test_a_page_of_eight_bytes(engine, base, tmp_path, capfd, monkeypatch):
    """The smallest page of the table (remove.path: 8 bytes, one block, a 1-byte preamble), which pyarrow
    stores as a literal and the planner copies: here with copies of 2 bytes and of 1, through k_snap_exec's
    byte stores of a page's last block."""
    data, old = _page(os.path.join(base[0], base[1]), "remove.path")
    assert len(data) == 8 and data[2:4] == data[1:2] * 2 and data[7] == data[3] and S.elements_of(old)[0][0] == "lit"
    el = [("lit", data[:2], 0), ("copy", 1, 2, 2), ("lit", data[4:7], 1), ("copy", 4, 1, 4)]
    body = S.encode(el)
    assert S.reference(body, 8) == data and S.pyarrow_decode(body, 8) == data and S.preamble_of(body)[1] == 1
    lp = _staged_copy(base, tmp_path, {("remove.path", 0): body})
    (pages, bad, codes, phases, _), plan = _check(engine, base, lp, capfd, monkeypatch)
    assert bad == 0 and phases and plan["snappy_out_bytes"] == base[7]["snappy_out_bytes"] + 8


# ---- (b) legal pages the documented rules send to k_snap_serial ----------------------------------------
def _find_back(data, at, n, before):
    """(offset, length) of the longest copy of at most n bytes for data[at:] from a source that starts before
    `before`."""
    for m in range(n, 0, -1):
        i = data.rfind(data[at:at + m], 0, before + m - 1)
        if i >= 0:
            return at - i, m
    raise AssertionError


def _b_reach_before(data):
    off, m = _find_back(data, F, 8, F - 70)
    el = S.compress(data[:F]) + [("copy", off, m, 2)] + S.compress(data[F + m:2 * F]) + S.compress(data[2 * F:])
    bad = [(op, e) for op, n, e in S.spans(el) if e[0] == "copy" and e[1] > op % F]
    assert bad == [(F, ("copy", off, m, 2))] and off < 65536
    return el


def _b_copy_straddles(data):
    off, m = _find_back(data, F - 2, 4, F - 70)
    assert m >= 3
    el = S.compress(data[:F - 2]) + [("copy", off, m, 2)] + S.compress(data[F - 2 + m:2 * F]) + S.compress(data[2 * F:])
    assert [(op, e[0]) for op, n, e in S.spans(el) if op // F != (op + n - 1) // F] == [(F - 2, "copy")]
    return el


def _b_literal_straddles(data):
    el = S.compress(data[:F - 3]) + S.literal(data[F - 3:F + 3]) + S.compress(data[F + 3:2 * F]) + S.compress(data[2 * F:])
    assert [(op, e[0]) for op, n, e in S.spans(el) if op // F != (op + n - 1) // F] == [(F - 3, "lit")]
    assert all(e[0] == "lit" or e[1] <= op % F for op, _, e in S.spans(el))
    return el


def _b_offset_65536(data):
    at = 2 * F + 100
    off, m = _find_back(data, at, 8, at - 65536)
    assert off >= 65536
    el = S.compress(data[:2 * F]) + S.compress(data[2 * F:at]) + [("copy", off, m, 4)] + S.compress(data[at + m:3 * F]) + S.compress(data[3 * F:])
    assert [e for e in _copies(el) if e[1] >= 65536] == [("copy", off, m, 4)]
    return el


def _b_one_byte_copies(data):
    def block(f):
        n = 2 * F // 5 + 1              # tag-3 copies of one byte: five bytes of input each, more than 128 KiB
        head = len(f) - n
        last, out = {}, S.literal(f[:head])
        for i in range(head):
            last[f[i]] = i
        for i in range(head, len(f)):
            out.append(("copy", i - last[f[i]], 1, 4) if f[i] in last else ("lit", f[i:i + 1], 0))
            last[f[i]] = i
        return out
    el = _per_fragment(data, {1: block})
    body = S.encode(el)
    count, span = _range_elements(body, 1)
    assert count <= EMAX * 1024 and span > 2 * F and S.keeps_fragments(el), (count, span)
    return el


B_KINDS = {
    # kind: (builder, the code k_snap_exec gives the page)
    "a copy reaching before its fragment": (_b_reach_before, 32),
    "a copy straddling a fragment end": (_b_copy_straddles, 32),
    "a literal straddling a fragment end": (_b_literal_straddles, 32),
    "a tag-3 copy at offset 65536 or more": (_b_offset_65536, 32),
    "a block of EXEC_EMAX * 1024 + 1 elements": (_a_emax(1), 16),
    "a block of one-byte copies in more than 128 KiB": (_b_one_byte_copies, 16),
}


def _twice(engine, base, lp, capfd, monkeypatch, want=None):
    """Two replays of one staged log, released in between: the same state and the same report. want: the
    exports to compare with, for a table whose contents are not the base's (then the oracle is not asked)."""
    monkeypatch.setenv("DR_SNAP_DEBUG", "1")
    capfd.readouterr()
    staged = engine.stage_log(lp)
    reports = []
    try:
        for _ in range(2):
            st = staged.replay(base[3])
            try:
                if want is None:
                    _assert_same(st, base[4])
                live, dead = want or (base[5], base[6])
                assert st.export(0) == live and st.export(1) == dead
            finally:
                st.release()
            reports.append(_report(capfd.readouterr().err))
    finally:
        staged.release()
    assert reports[0] == reports[1], reports
    return reports[0]


@pytest.mark.parametrize("kind", sorted(B_KINDS))
def test_legal_pages_outside_the_rules_take_the_serial_decoder(engine, base, tmp_path, capfd, monkeypatch, kind):
    """The crafted page is the only one reported, with the code of the rule it breaks; its neighbours -- every
    other page of the file is untouched -- decode in parallel, and the state is the oracle's on both replays."""
    build, code = B_KINDS[kind]
    data, _ = _page(os.path.join(base[0], base[1]), "add.path")
    el = build(data)
    body = S.encode(el)
    assert S.reference(body, len(data)) == data and S.pyarrow_decode(body, len(data)) == data
    lp = _staged_copy(base, tmp_path, {("add.path", 0): body})
    pages, bad, codes, phases, which = _twice(engine, base, lp, capfd, monkeypatch)
    assert pages > 1 and bad == 1 and codes == {code: 1} and phases, (pages, bad, codes)
    assert which == [(len(body) - 3, len(data))]


def test_two_pages_of_two_blocks_outside_the_rules(engine, base, tmp_path, capfd, monkeypatch):
    """The smallest pages of the table that can break a fragment rule (add.size and add.modificationTime: two
    blocks each), both crafted, beside an add.path page that keeps the rules. Every page reported is one of
    the two (the engine decodes add.size for two of its consumers, so that page is reported twice)."""
    bodies, crafted = {}, set()
    for leaf in ("add.size", "add.modificationTime"):
        data, _ = _page(os.path.join(base[0], base[1]), leaf)
        assert F < len(data) < 2 * F
        el = S.compress(data[:F - 3]) + S.literal(data[F - 3:F + 3]) + S.compress(data[F + 3:])
        assert not S.keeps_fragments(el)
        bodies[(leaf, 0)] = S.encode(el)
        assert S.reference(bodies[(leaf, 0)], len(data)) == data
        crafted.add((len(bodies[(leaf, 0)]) - 3, len(data)))
    lp = _staged_copy(base, tmp_path, bodies)
    pages, bad, codes, phases, which = _twice(engine, base, lp, capfd, monkeypatch)
    assert set(which) == crafted and len(crafted) == 2 and 2 <= bad == len(which) < pages and codes == {32: bad} and phases, \
        (pages, bad, codes, which)


# ---- (c) malformed bodies ---------------------------------------------------------------------------------
def test_malformed_pages_are_refused(engine, base, tmp_path, capfd, monkeypatch):
    """One page per refusal, each in a table of its own: the add.path page, replaced by a body made for its
    size. Each ends in DR_E_PARQUET, never in a state; the good table replays afterwards on the same engine."""
    from delta_amd.delta_log import DeltaError
    data, _ = _page(os.path.join(base[0], base[1]), "add.path")
    bodies = malformed_bodies(len(data))
    assert sorted(bodies) == MALFORMED and len(bodies) == 16
    # those bodies' bytes are no Parquet values, which the page decoders refuse as well; this one holds the page's own
    # bytes in full, so that only the SNAPPY decoder can refuse it: a decoder that took the literal of 2^32 bytes
    # behind them for an empty one would hand on a good page
    own = S.encode(S.compress(data)) + bytes([63 << 2]) + b"\xff" * 4
    assert S.wrapping_literal(own) and S.reference(own[:-5], len(data)) == data
    bodies = dict(bodies, **{"literal length 0xffffffff behind the page's own bytes": own})
    accepted = []
    for k, kind in enumerate(sorted(bodies)):
        assert S.reference(bodies[kind], len(data)) is None
        lp = _staged_copy(base, tmp_path / ("bad%d" % k), {("add.path", 0): bodies[kind]})
        try:
            st, _ = _replay(engine, lp, base[3])
            st.release()
            accepted.append(kind)
        except DeltaError as e:
            assert e.code == "DR_E_PARQUET", (kind, str(e))
    assert not accepted, accepted
    (pages, bad, codes, phases, _), _ = _check(engine, base, base[0], capfd, monkeypatch)
    assert bad == 0 and phases


# ---- (d) mixed codecs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("other", ["zstd", "lz4"])
def test_a_crafted_snappy_chunk_among_other_codecs(engine, base, tmp_path, capfd, monkeypatch, other):
    """The file holds chunks of all four codecs; of the leaves the replay plans, add.path is the crafted SNAPPY
    page, remove.deletionTimestamp GZIP and add.size ZSTD or LZ4 (the removes' pages are too small for either
    to count: a stored block is the planner's copy)."""
    import pyarrow.parquet as pq
    md = pq.ParquetFile(os.path.join(base[0], base[1])).metadata
    names = [md.row_group(0).column(i).path_in_schema for i in range(md.num_columns)]
    codec = {"add.path": "snappy", "add.size": other, "remove.path": "lz4", "remove.deletionTimestamp": "gzip"}
    lp = os.path.join(str(tmp_path), "_delta_log")
    shutil.copytree(base[0], lp)
    ck = os.path.join(lp, base[1])
    pq.write_table(base[2], ck, compression={n: codec.get(n, ("zstd", "snappy", "gzip", "lz4")[len(n) % 4]) for n in names},
                   use_dictionary=False, version="1.0", write_statistics=False)
    assert set(S.codecs_of(ck).values()) == {1, 2, 6, 7}
    data, _ = _page(ck, "add.path")
    el = S.compress(data, kinds=(4,), lit_nb=2)
    assert {e[3] for e in _copies(el)} == {4}
    S.rewrite(ck, ck, {("add.path", 0): (1, S.encode(el))})
    (pages, bad, codes, phases, _), plan = _check(engine, base, lp, capfd, monkeypatch)
    assert bad == 0 and phases and plan["snappy_in_bytes"] > 0 and plan["gzip_pages"] > 0 and plan[other + "_pages"] > 0
