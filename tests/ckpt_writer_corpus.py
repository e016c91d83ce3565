"""Shared by the checkpoint writer's page tests (host and GPU): `_delta_log`s of JSON commits written from
explicit action dicts (the dicts are the truth), the checkpoint rows those actions must give
(expected_rows: the test's own replay, nothing from the device), and the page bodies that steer
k_snap_compress (delta_amd/csrc/k_encode.hip) through the strings the writer copies verbatim.

A steered page is the add.stats page of a table of protocol, metaData and ONE add: the page is then the
writer's level bytes and the value's 4-byte length (page_prefix(): 11 bytes) followed by the string, so a
body kind lays out the whole page and hands back what lies behind the prefix. Every kind is a function
(seed, size, skip) -> bytes: `size` is the page's length, `skip` the prefix's, and the result has
size - skip bytes of JSON-safe text (64-symbol ASCII unless the kind says otherwise). Positions below are
page positions; the compressor cuts the page into 8 KiB fragments (one workgroup each) and every fragment
into 64-byte slices (one thread each).

model_elements() restates the compressor's documented algorithm (earliest position per hash bucket, greedy
per slice, matches cut at the slice end) on the host. It is there to check the corpus: that a kind really
holds the forms it is named for (tests/test_ckpt_writer_corpus.py). No GPU test expects its output."""
import json
import os
import re

import numpy as np

from tests import snappy_corpus as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHABET = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_", np.uint8)


def _source():
    return open(os.path.join(ROOT, "delta_amd", "csrc", "k_encode.hip")).read()


def kernel_constant(name):
    """A constexpr of k_encode.hip."""
    return int(re.search(r"constexpr \w+ %s = (\d+);" % name, _source()).group(1))


def hash_multiplier():
    return int(re.search(r"sc_hash\(uint32_t x\) \{ return \(x \* (0x[0-9a-f]+)u\) >> \(32 - SC_TBITS\); \}", _source()).group(1), 16)


FRAG, SLICE, SLOT, TBITS = (kernel_constant("SC_FRAG"), kernel_constant("SC_FRAG") // kernel_constant("SC_T"),
                            kernel_constant("SC_SLOT"), kernel_constant("SC_TBITS"))
MULT = hash_multiplier()
assert SLICE == 64 and FRAG == 8192


def sc_hash(x):
    """The bucket of the little-endian 4-byte group(s) x (an int or a uint32 array)."""
    if isinstance(x, np.ndarray):
        return (x.astype(np.uint64) * MULT & 0xffffffff) >> (32 - TBITS)
    return (x * MULT & 0xffffffff) >> (32 - TBITS)


def _groups(data):
    """The 4-byte group at every position of `data` (len - 3 of them), little-endian."""
    b = np.frombuffer(bytes(data), np.uint8).astype(np.uint32)
    return b[:-3] | b[1:-2] << 8 | b[2:-1] << 16 | b[3:] << 24 if len(b) >= 4 else np.zeros(0, np.uint32)


# ---- the compressor's algorithm, restated ------------------------------------------------------------
def model_elements(data):
    """The elements k_snap_compress's comment promises for `data` (snappy_corpus element tuples)."""
    out = []
    for f0 in range(0, len(data), FRAG):
        frag = data[f0:f0 + FRAG]
        n = len(frag)
        g = _groups(frag)
        table = {}
        for i, h in enumerate(sc_hash(g).tolist() if len(g) else []):
            table.setdefault(h, i)
        g = g.tolist()
        for s0 in range(0, n, SLICE):
            s1 = min(n, s0 + SLICE)
            ip = lit = s0
            while ip + 4 <= s1:
                cand = table[sc_hash(g[ip])]
                if cand < ip and g[cand] == g[ip]:
                    m = 4
                    while m < s1 - ip and frag[cand + m] == frag[ip + m]:
                        m += 1
                    if ip > lit:
                        out += S.literal(frag[lit:ip])
                    out.append(("copy", ip - cand, m, 1 if 4 <= m <= 11 and ip - cand < 2048 else 2))
                    ip += m
                    lit = ip
                else:
                    ip += 1
            if s1 > lit:
                out += S.literal(frag[lit:s1])
    return out


# ---- body kinds ----------------------------------------------------------------------------------------
def _fresh(rng, n):
    return ALPHABET[rng.integers(0, 64, n)].tobytes()


def _collision_free(rng, n, taken=()):
    """n symbols whose 4-byte groups (cyclically) fall into distinct buckets, none of them in `taken`."""
    while True:
        v = ALPHABET[rng.permutation(64)[:n]].tobytes()
        h = sc_hash(_groups(v + v[:3])).tolist()
        if len(set(h)) == len(h) and not set(h) & set(taken):
            return v


def random_body(seed, size, skip):
    """Incompressible."""
    return _fresh(np.random.default_rng(seed), size - skip)


def slice_literals(L):
    """Every 64-byte slice is L fresh bytes followed by 64 - L bytes repeated from the fragment's first slice
    (in the page's first fragment: from its second, the first holds the writer's prefix). A slice of the
    kernel's is then a literal of L and a copy of 64 - L -- while a copy fits: 64 - L < 4 leaves no room
    for one, and the slice is a literal of 64, in a tag of 60 << 2 and a length byte."""
    def kind(seed, size, skip):
        rng = np.random.default_rng(seed)
        page = bytearray(size)
        for f0 in range(0, size, FRAG):
            m0 = f0 + SLICE if f0 == 0 else f0
            page[f0:m0 + SLICE] = _fresh(rng, m0 + SLICE - f0)
            model = bytes(page[m0:m0 + SLICE])
            for s0 in range(m0 + SLICE, min(size, f0 + FRAG), SLICE):
                page[s0:s0 + SLICE] = _fresh(rng, L) + model[L:]
        return bytes(page[skip:size])
    return kind


def periodic64(seed, size, skip):
    """Every slice is one copy of earlier bytes: a fragment repeats its first slice (64 symbols whose groups
    share no bucket); the page's first fragment, whose first slice begins with the writer's prefix, repeats
    the 64 - skip bytes behind the prefix instead, so that its second slice is a copy of the first's own."""
    rng = np.random.default_rng(seed)
    page = bytearray(size)
    for f0 in range(0, size, FRAG):
        lo = skip if f0 == 0 else f0
        v = _collision_free(rng, SLICE - (lo - f0))
        n = min(size, f0 + FRAG) - lo
        page[lo:lo + n] = (v * (n // len(v) + 1))[:n]
    return bytes(page[skip:size])


RUN = 700   # bytes per run: no multiple of the slice


def runs(seed, size, skip):
    """Runs of RUN bytes, each of symbols no other run of the fragment uses: one byte repeated, then a
    period of 2, then of 3, and again. The second slice-step into a run finds its first group 1, 2 or 3
    bytes back: an overlapping copy."""
    rng = np.random.default_rng(seed)
    out = bytearray()
    k, base = 0, int(rng.integers(0, 64))
    while len(out) < size - skip:
        sym = ALPHABET[(np.arange(3) + 3 * k + base) % 64].tobytes()
        period = sym[:1 + k % 3]
        out += (period * RUN)[:RUN]
        k += 1
    return bytes(out[:size - skip])


# copy_lengths: (source position, target position, length) per fragment, as fragment positions. The source is
# bytes 64..512 of the fragment; a target repeats `length` source bytes and then differs.
COPY_PLAN = ([(64, 512 + 64 * k, n) for k, n in enumerate((4, 11, 12, 64))] + [(64, 768 + 1, 63)] +      # offsets 448..705
             [(65 + 64 * k, 2112 + 64 * k, n) for k, n in enumerate((4, 11, 12))] +                     # offset 2047
             [(64 + 64 * k, 2112 + 64 * k, n) for k, n in ((3, 4), (4, 11), (5, 12))] +                 # offset 2048
             [(70, 8100, 4), (100, 8128, 64)])                                                          # offsets 8030, 8028


def copy_lengths(seed, size, skip):
    """Matches of exactly 4, 11, 12, 63 and 64 bytes at offsets below 2048, of 4, 11 and 12 at 2047 and at
    2048, and of 4 and 64 above 8000 (COPY_PLAN), in every whole fragment. The seed is advanced until the
    restated algorithm finds every planned match (no source loses its bucket, no chance match runs into a target)."""
    assert size >= FRAG
    while True:
        rng = np.random.default_rng(seed)
        page = bytearray(b"\0" * skip + _fresh(rng, size - skip))
        for f0 in range(0, size - FRAG + 1, FRAG):
            for s, t, n in COPY_PLAN:
                page[f0 + t:f0 + t + n] = page[f0 + s:f0 + s + n]
                if (t + n) % SLICE:      # the byte behind the match differs from the source's
                    nxt = page[f0 + s + n]
                    page[f0 + t + n] = int(ALPHABET[(int(np.where(ALPHABET == nxt)[0][0]) + 1) % 64])
        if skip == ONE_ADD_SKIP:
            page[:skip] = page_prefix([0, 0, 2], 2, size - skip)
        found = {(op // FRAG, op % FRAG, e[1], e[2]) for op, _, e in S.spans(model_elements(bytes(page))) if e[0] == "copy"}
        ok = all((f, t, t - s, n) in found for f in range(size // FRAG) for s, t, n in COPY_PLAN)
        if ok:
            return bytes(page[skip:size])
        seed += 1000


_WORDS = ["Zürich", "naïve", "日本語", "ключ", "größe", "λόγος", "données", "ąęść", "数", "Ünïcödé"]


def utf8(seed, size, skip):
    """Multi-byte text: words of two- and three-byte characters, so every slice holds bytes >= 0x80."""
    rng = np.random.default_rng(seed)
    out = bytearray()
    while len(out) < size - skip:
        w = _WORDS[int(rng.integers(0, len(_WORDS)))].encode()
        if len(out) + len(w) > size - skip:
            break
        out += w
    while len(out) < size - skip - 1:
        out += "é".encode()
    out += b"." * (size - skip - len(out))
    return bytes(out)


COLLIDE_GROUPS = 40
COLLIDE_AT = 1024    # page position of the first group; one group every 16 bytes


def colliding_groups(count=COLLIDE_GROUPS):
    """`count` distinct 4-symbol groups of one sc_hash bucket (the fullest among the groups tried)."""
    a = ALPHABET.astype(np.uint32)
    g = (a[:, None, None, None] | a[None, :, None, None] << 8 | a[None, None, :, None] << 16 |
         a[None, None, None, :16] << 24).ravel()
    h = sc_hash(g)
    bucket = int(np.bincount(h.astype(np.int64)).argmax())
    mine = g[h == bucket][:count]
    assert len(mine) == count
    return [int(x).to_bytes(4, "little") for x in mine]


def collide(seed, size, skip):
    """COLLIDE_GROUPS distinct groups of one bucket, one every 16 bytes from COLLIDE_AT on, random text between
    them, and behind the last one a true repeat of it (4 bytes; what follows differs). The earliest-position
    table keeps the first group's position for the bucket, so the repeat's candidate is the wrong group."""
    assert size >= COLLIDE_AT + 16 * (COLLIDE_GROUPS + 2)
    rng = np.random.default_rng(seed)
    page = bytearray(b"\0" * skip + _fresh(rng, size - skip))
    groups = colliding_groups()
    for f0 in range(0, size - FRAG + 1, FRAG):
        for k, grp in enumerate(groups + groups[-1:]):
            page[f0 + COLLIDE_AT + 16 * k:f0 + COLLIDE_AT + 16 * k + 4] = grp
        last = f0 + COLLIDE_AT + 16 * (len(groups) - 1)
        page[last + 4], page[last + 20] = ord("A"), ord("B")
    return bytes(page[skip:size])


def collide_repeat(f0=0):
    """(position of the last group, position of its repeat) in the fragment at f0."""
    last = f0 + COLLIDE_AT + 16 * (COLLIDE_GROUPS - 1)
    return last, last + 16


KINDS = {"random": random_body, "periodic64": periodic64, "runs": runs, "copy_lengths": copy_lengths, "utf8": utf8,
         "collide": collide}
KINDS.update({"slice_literals(%d)" % L: slice_literals(L) for L in (1, 59, 60, 61, 63)})

# Page sizes for one add.stats page. SMALLEST is the page of one row with null stats (levels only). A tail of
# 60 or 61 bytes is the only place a literal of exactly 60 or 61 can stand (a full slice that holds a copy
# has at most 60 literal bytes): 252 and 253 reach the one-byte / two-byte literal tag boundary.
SMALLEST = "smallest"
TAILS = [192, 193, 195, 196, 197, 252, 253]            # len % 64 in {0, 1, 3, 4, 5, 60, 61}
FRAGMENTS = [8191, 8192, 8193, 8195, 16384]
BLOCKS = [65535, 65536, 65537, 2 * 65536 + 100]
SIZES = TAILS + FRAGMENTS + BLOCKS


# ---- logs -------------------------------------------------------------------------------------------------
PROTOCOL = {"minReaderVersion": 1, "minWriterVersion": 2}


def metadata(partition_columns=(), configuration=None, table_id="ckpt-writer"):
    schema = {"type": "struct", "fields": [{"name": c, "type": "string", "nullable": True, "metadata": {}}
                                           for c in list(partition_columns) + ["v"]]}
    return {"id": table_id, "name": None, "description": None, "format": {"provider": "parquet", "options": {}},
            "schemaString": json.dumps(schema), "partitionColumns": list(partition_columns),
            "configuration": dict(configuration or {}), "createdTime": 1}


def write_log(table, commits):
    """Writes table/_delta_log with one JSON commit per list of `commits` ([{"add": {...}}, ...], written as
    given: a missing key stays missing, a None is a JSON null). Returns (log path, the actions in log order)."""
    lp = os.path.join(str(table), "_delta_log")
    os.makedirs(lp)
    for v, actions in enumerate(commits):
        with open(os.path.join(lp, "%020d.json" % v), "w", encoding="utf-8") as f:
            for a in actions:
                f.write(json.dumps(a, ensure_ascii=False, separators=(",", ":")) + "\n")
    return lp, [a for actions in commits for a in actions]


def head(partition_columns=(), txns=()):
    return [{"protocol": PROTOCOL}, {"metaData": metadata(partition_columns)}] + [{"txn": t} for t in txns]


def add(path, **kw):
    a = {"path": path, "partitionValues": {}, "size": 1, "modificationTime": 1, "dataChange": True}
    a.update(kw)
    return {"add": a}


def remove(path, **kw):
    r = {"path": path, "deletionTimestamp": 10, "dataChange": True}
    r.update(kw)
    return {"remove": r}


def one_add_log(table, stats, **kw):
    """protocol, metaData and one add whose stats is `stats` (None: no stats key)."""
    extra = {} if stats is None else {"stats": stats}
    return write_log(table, [head() + [add("steered.parquet", **extra, **kw)]])


def _varint(n):
    return S.varint(n)


def page_prefix(levels, width, value_len=None):
    """The bytes a PLAIN v1 page of a flat optional leaf begins with: the definition levels as one bit-packed run
    (u32 length, varint header, groups of 8 levels in `width` bits, least significant first), then the first
    value's length."""
    groups = (len(levels) + 7) // 8
    packed = bytearray()
    for g in range(groups):
        bits = 0
        for k, lv in enumerate(levels[8 * g:8 * g + 8]):
            bits |= lv << width * k
        packed += bits.to_bytes(width, "little")
    sec = _varint(groups << 1 | 1) + bytes(packed)
    return len(sec).to_bytes(4, "little") + sec + (b"" if value_len is None else value_len.to_bytes(4, "little"))


ONE_ADD_SKIP = len(page_prefix([0, 0, 2], 2, 0))     # 11: protocol and metaData rows (level 0), the add's stats (2)


def one_add_page(string):
    """The add.stats page of one_add_log(): string None gives the smallest page the writer can produce."""
    if string is None:
        return page_prefix([0, 0, 1], 2)
    return page_prefix([0, 0, 2], 2, len(string)) + string


def steered(kind, size, seed=1):
    """(stats string, the page it must give) of body kind `kind` for a page of `size` bytes."""
    if size == SMALLEST:
        return None, one_add_page(None)
    s = KINDS[kind](seed, size, ONE_ADD_SKIP)
    assert len(s) == size - ONE_ADD_SKIP
    return s.decode("utf-8"), one_add_page(s)


# ---- expected rows ------------------------------------------------------------------------------------------
def _items(m):
    return None if m is None else list(m.items())


def expected_rows(actions, cutoff, stats=True, parsed=None):
    """The checkpoint's rows as pyarrow reads them (maps as lists of pairs), in the writer's order: protocol,
    metaData, txns, live adds, tombstones retained past `cutoff` -- replayed here from the action dicts (paths
    must be plain relative names, which no canonicalisation touches). parsed: the string partition columns of
    partitionValues_parsed, or None."""
    prot = md = None
    txns, adds, rms = {}, {}, {}
    for a in actions:
        (kind, v), = a.items()
        if kind == "protocol":
            prot = v
        elif kind == "metaData":
            md = v
        elif kind == "txn":
            txns[v["appId"]] = v
        elif kind == "add":
            assert re.fullmatch(r"[A-Za-z0-9._=-]+", v["path"]), v["path"]
            rms.pop(v["path"], None)
            adds.pop(v["path"], None)
            adds[v["path"]] = v
        elif kind == "remove":
            adds.pop(v["path"], None)
            rms.pop(v["path"], None)
            rms[v["path"]] = v
    rows = []

    def row(kind, v):
        r = dict.fromkeys(("txn", "add", "remove", "metaData", "protocol"))
        r[kind] = v
        rows.append(r)
    if prot is not None:
        row("protocol", {"minReaderVersion": prot.get("minReaderVersion", 0), "minWriterVersion": prot.get("minWriterVersion", 0)})
    if md is not None:
        fmt = md.get("format") or {}
        row("metaData", {"id": md.get("id"), "name": md.get("name"), "description": md.get("description"),
                         "format": {"provider": fmt.get("provider"), "options": _items(fmt.get("options") or {})},
                         "schemaString": md.get("schemaString"), "partitionColumns": md.get("partitionColumns"),
                         "configuration": _items(md.get("configuration") or {}), "createdTime": md.get("createdTime")})
    for t in txns.values():
        row("txn", {"appId": t.get("appId"), "version": t.get("version", 0), "lastUpdated": t.get("lastUpdated")})
    for a in adds.values():
        r = {"path": a["path"], "partitionValues": _items(a.get("partitionValues")), "size": a.get("size") or 0,
             "modificationTime": a.get("modificationTime") or 0, "dataChange": False, "tags": _items(a.get("tags"))}
        if stats:
            r["stats"] = a.get("stats")
        if parsed:
            r["partitionValues_parsed"] = {c: (a.get("partitionValues") or {}).get(c) for c in parsed}
        row("add", r)
    for x in rms.values():
        if (x.get("deletionTimestamp") or 0) > cutoff:
            row("remove", {"path": x["path"], "deletionTimestamp": x.get("deletionTimestamp"), "dataChange": False,
                           "extendedFileMetadata": bool(x.get("extendedFileMetadata") or False),
                           "partitionValues": _items(x.get("partitionValues")), "size": x.get("size") or 0,
                           "tags": _items(x.get("tags"))})
    return rows


def kind_of(row):
    (k,) = [k for k, v in row.items() if v is not None]
    return k


def assert_rows(got, want):
    """Same rows: the head rows in order, the sections in the writer's order (head, adds, removes), each
    file-action side as a multiset keyed by path."""
    assert [kind_of(r) for r in got] == [kind_of(r) for r in want]
    for side in ("add", "remove"):
        g = sorted((r[side] for r in got if r[side] is not None), key=lambda x: x["path"])
        w = sorted((r[side] for r in want if r[side] is not None), key=lambda x: x["path"])
        assert [x["path"] for x in g] == [x["path"] for x in w]
        for x, y in zip(g, w):
            assert x == y, (x, y)
    g = [r for r in got if r["add"] is None and r["remove"] is None]
    w = [r for r in want if r["add"] is None and r["remove"] is None]
    assert g == w, (g, w)


# ---- the tables of the level tests ------------------------------------------------------------------------
I64 = [0, -1, 2 ** 31, 2 ** 32 + 1, 2 ** 63 - 1, -2 ** 63]
CUTOFF = -2 ** 63     # retains every tombstone but one whose deletionTimestamp is the smallest int64


def _map_cases(i):
    """The map of row i: null, empty, 1 entry, 9 entries, null values first / last / everywhere, empty key,
    empty value."""
    cases = [None, {}, {"k": "v%d" % i}, {"k%d" % j: "v%d-%d" % (i, j) for j in range(9)},
             {"a": None, "b": "x", "c": "y"}, {"a": "x", "b": "y", "c": None}, {"a": None, "b": None}, {"": "empty key"},
             {"empty value": ""}, {"": ""}]
    return cases[i % len(cases)]


def level_table(n_adds=300, n_removes=40, txns=1):
    """The commits of a table of 2 + txns head rows, n_adds live adds and n_removes tombstones: maps of every
    shape on both sides (one row of each side with 300 entries), int64 values of I64, stats absent, empty and
    set, removes with and without extendedFileMetadata and deletionTimestamp."""
    c0 = head(txns=[{"appId": "app-%d" % k, "version": 7 + k, "lastUpdated": 1000 + k} for k in range(txns)])
    big = {"key-%03d" % j: (None if j % 7 == 3 else "value-%03d" % j) for j in range(300)}
    for i in range(n_adds + n_removes):
        a = {"path": "f-%05d.parquet" % i, "partitionValues": _map_cases(i), "size": I64[i % 6],
             "modificationTime": I64[(i // 6) % 6], "dataChange": True}
        if i % 5 != 0:
            a["tags"] = _map_cases(i // 3 + 1)
        if i % 3:
            a["stats"] = "" if i % 3 == 1 else '{"numRecords":%d}' % i
        if i == 17:
            a["partitionValues"] = big
        if i == 255:
            a["tags"] = big
        c0.append({"add": a})
    c1 = []
    for i in range(n_adds, n_adds + n_removes):
        r = {"path": "f-%05d.parquet" % i, "dataChange": True}
        if i % 11:           # else: no deletionTimestamp, which reads as 0 and is written as null
            r["deletionTimestamp"] = I64[i % 5]
        if i % 2:
            r.update(extendedFileMetadata=bool(i % 4 == 1), partitionValues=_map_cases(i // 2), size=I64[(i // 2) % 6])
            if i % 8 != 1:
                r["tags"] = _map_cases(i // 2 + 3)
            if i == n_adds + 5:
                r["partitionValues"] = big
            if i == n_adds + 7:
                r["tags"] = big
        c1.append({"remove": r})
    if c1:      # at the cutoff, not past it: never a row
        c1.append(remove("never-a-row.parquet", deletionTimestamp=CUTOFF))
    return [c0, c1] if c1 else [c0]
