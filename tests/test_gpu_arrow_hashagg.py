"""Hash GROUP BY on the GPU (csrc/kernels/colgroup.hip): the kernels alone
through ops/colgroup.py on hand-built batch tables against the numpy twin —
by key, never slot by slot: which slot a key gets depends on which CAS wins
— and whole scans with by=HashBy against pyarrow and the host twin under the
comparison rule of tests/agggen.py."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))

PREFILL = -77
ROWS = (1000, 64, 41)                   # full words, an exact word, a tail
I64_MIN = -(1 << 63)


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nvme_strom_amd as S
    S.configure(gpu_emulation=0)
    return S


# ------------------------------------------------------------ kernels alone
class _Tab:
    """Hand-built record batches on the device: per column a (nbatches, 5)
    strom_filter_batch table over the same batches, the code buffers' table,
    and the host arrays."""

    def __init__(self, rows=ROWS, seed=0):
        self.rows = list(rows)
        self.rng = np.random.default_rng(seed)
        words = [(r + 63) // 64 for r in self.rows]
        self.word_base = np.concatenate([[0], np.cumsum(words)[:-1]]).astype(np.int64)
        self.nwords = int(sum(words))
        self.keep = []
        self.kbuf = torch.full((self.nwords * 64,), PREFILL, dtype=torch.int32, device="cuda")
        ct = np.zeros((len(self.rows), 5), np.int64)
        for b, n in enumerate(self.rows):
            ct[b] = (self.kbuf.data_ptr() + int(self.word_base[b]) * 256, 0, n, self.word_base[b], 0)
        self.ctab = torch.from_numpy(ct).cuda()

    def column(self, make, null_p=0.0, all_null=False):
        """(host [(values, valid or None)], device table); ``make`` is a
        function of the row count or one array over all rows."""
        host, tab = [], np.zeros((len(self.rows), 5), np.int64)
        at = 0
        for b, n in enumerate(self.rows):
            v = make(n) if callable(make) else np.asarray(make)[at:at + n]
            at += n
            ok, vptr = None, 0
            if null_p or all_null:
                ok = np.zeros(n, bool) if all_null else self.rng.random(n) >= null_p
                bits = np.zeros(((n + 63) // 64) * 64, np.uint8)
                bits[:n] = ok
                dv = torch.from_numpy(np.packbits(bits, bitorder="little").copy()).cuda()
                self.keep.append(dv)
                vptr = dv.data_ptr()
            d = torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).copy()).cuda()
            self.keep.append(d)
            tab[b] = (d.data_ptr(), vptr, n, self.word_base[b], 0)
            host.append((np.asarray(v), ok))
        t = torch.from_numpy(tab).cuda()
        self.keep.append(t)
        return host, t

    def bitmap(self, p, garbage=True):
        """(host bool per batch, source words): bits beyond a batch's rows
        are set at random — the kernels must ignore them."""
        words = np.zeros(self.nwords, np.uint64)
        host = []
        for b, n in enumerate(self.rows):
            nw = (n + 63) // 64
            bits = self.rng.random(nw * 64) < p
            host.append(bits[:n].copy())
            if not garbage:
                bits[n:] = False
            words[self.word_base[b]:self.word_base[b] + nw] = \
                np.packbits(bits, bitorder="little").view(np.uint64)
        return host, words

    def unpack(self, words):
        """Bitmap words -> bool per batch (the rows that exist)."""
        out = []
        for wb, n in zip(self.word_base, self.rows):
            nw = (n + 63) // 64
            bits = np.unpackbits(words[int(wb):int(wb) + nw].view(np.uint8), bitorder="little")
            out.append(bits[:n].astype(bool))
        return out

    def codes(self):
        out = self.kbuf.cpu().numpy()
        return [out[int(wb) * 64:int(wb) * 64 + n] for wb, n in zip(self.word_base, self.rows)]


def _codes_launch(G, t, tab, kcode, key, sel_h, src_words, in_place, stream=None):
    """strom_group_codes over ``tab``; checks the destination bitmap and the
    codes, returns (rows that kept a code per batch, {key pattern: code})."""
    khost, ktab = key
    src = torch.from_numpy(src_words.view(np.int64).copy()).cuda()
    dst = src if in_place else torch.full_like(src, 0x1234)
    tab.kbuf.fill_(PREFILL)
    torch.cuda.synchronize()
    G.group_codes(t, kcode, ktab, tab.nwords, src, dst, tab.ctab, stream=stream)
    torch.cuda.synchronize()
    got = tab.unpack(dst.cpu().numpy().view(np.uint64))
    # no bit beyond a batch's rows survives, whatever the source held there
    clean = np.zeros(tab.nwords, np.uint64)
    for wb, g in zip(tab.word_base, got):
        bits = np.zeros(((len(g) + 63) // 64) * 64, np.uint8)
        bits[:len(g)] = g
        clean[int(wb):int(wb) + len(bits) // 64] = np.packbits(bits, bitorder="little").view(np.uint64)
    assert np.array_equal(dst.cpu().numpy().view(np.uint64), clean)
    if not in_place:
        assert np.array_equal(src.cpu().numpy().view(np.uint64), src_words)
    slots = t.slots()
    C = t.capacity
    code_of = {}
    for (kv, kok), sel, kept, codes in zip(khost, sel_h, got, tab.codes()):
        assert not (kept & ~sel).any()
        assert (codes[~sel] == PREFILL).all()          # only selected rows are written
        assert (codes[sel & ~kept] == 0).all()         # no slot found: code 0, bit cleared
        pat = G.wide_keys(kv).view(np.uint64)
        ok = np.ones(len(kv), bool) if kok is None else kok
        assert (codes[kept & ~ok] == C).all()
        assert (kept | ~sel | ok).all()                # a null key never overflows
        for p, c in zip(pat[kept & ok].tolist(), codes[kept & ok].tolist()):
            assert code_of.setdefault(p, c) == c       # one code per key
            if p == 1 << 63:
                assert c == C + 1
            else:
                assert 0 <= c < C and int(slots[c]) == p
    assert len(set(code_of.values())) == len(code_of)  # distinct keys, distinct codes
    return got, code_of


def _equal_groups(G, got, want):
    assert got.keys.dtype == want.keys.dtype and np.array_equal(got.keys, want.keys)
    for e in range(len(want.entries)):
        g, w = got.arrays(e), want.arrays(e)
        for name in w:
            assert np.array_equal(g[name], w[name], equal_nan=w[name].dtype.kind == "f"), \
                (e, name, g[name], w[name])


def _twin(G, ents, kept, key, data, unsigned):
    want = G.empty_groups(ents, unsigned)
    for b in range(len(kept)):
        want = G.merge(want, G.host_group_agg(ents, kept[b], key[0][b][0], key[0][b][1],
                                              [(h[b][0], h[b][1]) for h, _ in data]))
    return want


def _run(G, tab, kdtype, key, ents, data, sel, groups, in_place=True, combine=None,
         overflow=False):
    """codes + every entry's accumulate + compaction against the twin; the
    header counters; returns (header, device Groups, {key: code})."""
    sel_h, src_words = sel
    unsigned = np.dtype(kdtype).kind == "u"
    t = G.DeviceGroups(ents, groups, "cuda", unsigned)
    kept, code_of = _codes_launch(G, t, tab, G.KEY_CODE[kdtype], key, sel_h, src_words, in_place)
    bm = torch.from_numpy(np.concatenate(
        [np.packbits(np.pad(k, (0, -len(k) % 64)), bitorder="little") for k in kept]
    ).view(np.int64).copy()).cuda()
    for e, (_, vt) in enumerate(data):
        G.group_agg(t, e, bm, tab.nwords, vt, tab.ctab, combine=combine)
    hdr, got = G.compact(t)
    torch.cuda.synchronize()
    dropped = sum(int((s & ~k).sum()) for s, k in zip(sel_h, kept))
    assert int(hdr[G.H_CAPACITY]) == G.capacity(groups) == t.capacity
    assert int(hdr[G.H_OVERFLOW]) == dropped and (dropped > 0) == overflow
    assert int(hdr[G.H_NKEYS]) == len(code_of)
    assert bool(hdr[G.H_HAS_EMPTY]) == ((1 << 63) in code_of)
    assert (hdr[4:] == 0).all()
    want = _twin(G, ents, kept, key, data, unsigned)
    assert len(want.keys) == len(code_of)
    _equal_groups(G, got, want)
    return hdr, got, code_of


def _special(dt):
    info = np.iinfo(dt)
    s = [0, info.min, info.max] + ([-1] if info.min < 0 else [])
    if dt.itemsize == 8:
        s.append((1 << 63) if info.min == 0 else I64_MIN)      # the free slot's pattern
    return np.array(s, dt)


def _int_f8(r):
    # small integers as floats: their sums are exact in any order
    return lambda n: np.where(r.random(n) < 0.1, np.nan, r.integers(-1000, 1000, n).astype(np.float64))


def _entries(A, tab, r):
    """count(*), int64 all four, f64 all four with NaN, f32, a count-only
    column: (entries, [(host, table)])."""
    ents = [A.Entry(A.COUNT | A.ALL), A.Entry(15, "i8"), A.Entry(15, "f8"), A.Entry(15, "f4"),
            A.Entry(A.COUNT, None, "validity only"), A.Entry(A.COUNT | A.SUM, "u8")]
    data = [tab.column(lambda n: np.zeros(n, np.int8)),
            tab.column(lambda n: r.integers(-2**63, 2**63 - 1, n, dtype=np.int64), null_p=0.2),
            tab.column(_int_f8(r), null_p=0.1),
            tab.column(lambda n: _int_f8(r)(n).astype(np.float32)),
            tab.column(lambda n: np.zeros(n, np.int32), null_p=0.5),
            tab.column(lambda n: r.integers(0, 2**64 - 1, n, dtype=np.uint64))]
    return ents, data


@pytest.mark.parametrize("kdtype", ["i1", "i2", "i4", "i8", "u1", "u2", "u4", "u8"])
@pytest.mark.parametrize("in_place", [True, False])
def test_every_key_type(S, kdtype, in_place):
    """Keys 0, -1, the type's min and max and (64-bit) the free slot's
    pattern among random ones, nulls in the key; a uint64 column mixes
    values below and above 2^63; garbage in the bitmap's tail bits."""
    from nvme_strom_amd.ops import colagg as A
    from nvme_strom_amd.ops import colgroup as G
    tab = _Tab(seed=3)
    r = tab.rng
    dt = np.dtype(kdtype)
    info = np.iinfo(dt)
    pool = np.concatenate([_special(dt), r.integers(info.min, info.max, 40, dtype=dt, endpoint=True)])
    if kdtype == "u8":
        assert (pool < 2**63).any() and (pool > 2**63).any() and (pool == 2**63).any()
    key = tab.column(lambda n: r.choice(pool, n), null_p=0.1)
    ents, data = _entries(A, tab, r)
    hdr, got, code_of = _run(G, tab, kdtype, key, ents, data, tab.bitmap(0.8), 64, in_place)
    for s in _special(dt).tolist():
        assert s in got.keys.tolist()
    # f64 NaN in some groups only
    sums = got.arrays(2)["sum"]
    assert np.isnan(sums).any() and not np.isnan(sums).all()
    assert got.arrays(0)["count"][-1] > 0             # the null keys' group


def test_chain_and_wrap(S):
    """200 keys on one home slot of a 512-slot table; keys homed on the
    last two slots of a 64-slot table, whose chains wrap."""
    from joingen import keys_with_home
    from nvme_strom_amd.ops import colagg as A
    from nvme_strom_amd.ops import colgroup as G
    for keys, groups in ((keys_with_home(300, 512, 200), 256),
                         (np.concatenate([keys_with_home(63, 64, 9),
                                          keys_with_home(62, 64, 3, 10**7)]), 32)):
        tab = _Tab(seed=5)
        r = tab.rng
        key = tab.column(np.resize(r.permutation(keys), sum(ROWS)))    # each key 5 times or more
        ents, data = _entries(A, tab, r)
        hdr, got, code_of = _run(G, tab, "i8", key, ents, data, tab.bitmap(0.95), groups)
        assert len(code_of) == len(keys)
        cap = G.capacity(groups)
        home = (G.hash64(keys) & np.uint64(cap - 1)).astype(np.int64)
        disp = (np.array([code_of[int(k)] for k in keys]) - home) % cap
        assert sorted(disp.tolist())[-1] >= len(keys) - 4   # one chain (two that meet: wrap)


def test_exactly_full_and_over_full(S):
    from nvme_strom_amd.ops import colagg as A
    from nvme_strom_amd.ops import colgroup as G
    tab = _Tab(seed=7)
    r = tab.rng
    keys = r.permutation(np.arange(-20, 20)).astype(np.int64) * 10**9
    ents, data = _entries(A, tab, r)
    # exactly full: groups distinct keys
    key = tab.column(lambda n: r.choice(keys[:32], n))
    hdr, got, code_of = _run(G, tab, "i8", key, ents, data, tab.bitmap(1.0), 32)
    assert int(hdr[G.H_NKEYS]) == 32 and int(hdr[G.H_OVERFLOW]) == 0
    # over-full: 40 distinct keys into groups=8 (16 slots); the accumulators
    # hold exactly the rows that kept a code (_run's twin runs over those)
    key = tab.column(lambda n: r.choice(keys, n), null_p=0.05)
    for in_place in (True, False):
        hdr, got, code_of = _run(G, tab, "i8", key, ents, data, tab.bitmap(0.9), 8, in_place,
                                 overflow=True)
        assert int(hdr[G.H_NKEYS]) == 16 and int(hdr[G.H_OVERFLOW]) > 0
        assert got.arrays(0)["count"][-1] > 0         # null keys need no slot


@pytest.mark.parametrize("combine", [0, 1])
def test_one_key_and_two_alternating(S, combine):
    """One key on all 65,536 selected rows (the run path: one set of atomics
    per wave); two keys alternating row by row (mixed words, every lane on
    two addresses)."""
    from nvme_strom_amd.ops import colagg as A
    from nvme_strom_amd.ops import colgroup as G
    n = 65_536
    for keys in (np.full(n, 123456789012, np.int64),
                 np.where(np.arange(n) % 2 == 0, -5, 10**15).astype(np.int64)):
        tab = _Tab(rows=(40_000, 25_536), seed=9)
        r = tab.rng
        key = tab.column(keys)
        ents, data = _entries(A, tab, r)
        hdr, got, code_of = _run(G, tab, "i8", key, ents, data, tab.bitmap(1.0), 4,
                                 combine=combine)
        assert got.arrays(0)["count"].tolist() == ([n, 0] if keys[0] == keys[1] else
                                                   [n // 2, n // 2, 0])


def test_all_distinct(S):
    """20,000 rows, all distinct, groups=20,000."""
    from nvme_strom_amd.ops import colagg as A
    from nvme_strom_amd.ops import colgroup as G
    tab = _Tab(rows=(12_000, 7_959, 41), seed=11)
    r = tab.rng
    keys = np.unique(r.integers(-2**63, 2**63 - 1, 30_000, dtype=np.int64))[:20_000]
    key = tab.column(r.permutation(keys))
    ents, data = _entries(A, tab, r)
    hdr, got, code_of = _run(G, tab, "i8", key, ents, data, tab.bitmap(1.0), 20_000)
    assert int(hdr[G.H_NKEYS]) == 20_000 and got.arrays(0)["count"][:-1].tolist() == [1] * 20_000


def test_null_columns_and_empty_selection(S):
    """An all-null key column yields only the null group (code C); an
    all-null value column counts nothing; an empty selection no group."""
    from nvme_strom_amd.ops import colagg as A
    from nvme_strom_amd.ops import colgroup as G
    tab = _Tab(seed=13)
    r = tab.rng
    ents = [A.Entry(A.COUNT | A.ALL), A.Entry(15, "f8"), A.Entry(15, "i4")]
    data = [tab.column(lambda n: np.zeros(n, np.int8)),
            tab.column(_int_f8(r), all_null=True),
            tab.column(lambda n: r.integers(-2**31, 2**31 - 1, n).astype(np.int32))]
    key = tab.column(lambda n: r.integers(0, 9, n), all_null=True)
    sel = tab.bitmap(0.7)
    hdr, got, code_of = _run(G, tab, "i8", key, ents, data, sel, 16)
    assert code_of == {} and len(got.keys) == 0 and int(hdr[G.H_NKEYS]) == 0
    nsel = sum(int(s.sum()) for s in sel[0])
    assert got.arrays(0)["count"].tolist() == [nsel]
    assert got.arrays(1)["count"].tolist() == [0] and got.arrays(2)["count"].tolist() == [nsel]
    for c in tab.codes():
        assert set(c.tolist()) <= {PREFILL, G.capacity(16)}
    key = tab.column(lambda n: r.integers(0, 9, n))
    hdr, got, _ = _run(G, tab, "i8", key, ents, data, sel, 16)
    assert got.arrays(1)["count"].tolist() == [0] * 10 and len(got.keys) == 9
    hdr, got, code_of = _run(G, tab, "i8", key, ents, data, tab.bitmap(0.0), 16, in_place=False)
    assert code_of == {} and len(got.keys) == 0 and got.arrays(0)["count"].tolist() == [0]
    # a fresh table: every key word free, the header capacity and zeros
    fresh = G.DeviceGroups(ents, 16, "cuda")
    assert fresh.slots().tolist() == [1 << 63] * 32
    assert fresh.header().tolist() == [32] + [0] * 7


def test_two_launches_on_one_table(S):
    """Overlapping key sets from two streams into one table, then one
    compaction: the scan's slot streams."""
    from nvme_strom_amd.ops import colagg as A
    from nvme_strom_amd.ops import colgroup as G
    ents = [A.Entry(A.COUNT | A.ALL), A.Entry(15, "i8"), A.Entry(15, "f8")]
    t = G.DeviceGroups(ents, 4096, "cuda")
    torch.cuda.synchronize()
    parts, streams = [], [torch.cuda.Stream(), torch.cuda.Stream()]
    for i, st in enumerate(streams):
        tab = _Tab(rows=(30_000, 2_041), seed=20 + i)
        r = tab.rng
        key = tab.column(lambda n: r.integers(1000 * i, 1000 * i + 3000, n), null_p=0.05)
        data = [tab.column(lambda n: np.zeros(n, np.int8)),
                tab.column(lambda n: r.integers(-2**40, 2**40, n), null_p=0.1),
                tab.column(_int_f8(r))]
        sel_h, words = tab.bitmap(0.9)
        bm = torch.from_numpy(words.view(np.int64).copy()).cuda()
        parts.append((tab, key, data, sel_h, bm))
    torch.cuda.synchronize()
    for (tab, key, data, sel_h, bm), st in zip(parts, streams):
        with torch.cuda.stream(st):
            G.group_codes(t, G.KEY_CODE["i8"], key[1], tab.nwords, bm, bm, tab.ctab, stream=st)
            for e, (_, vt) in enumerate(data):
                G.group_agg(t, e, bm, tab.nwords, vt, tab.ctab, stream=st)
    torch.cuda.synchronize()
    hdr, got = G.compact(t)
    want = G.empty_groups(ents)
    for tab, key, data, sel_h, bm in parts:
        want = G.merge(want, _twin(G, ents, sel_h, key, data, False))
    # keys 0..2999 and 1000..3999, nearly all of them selected: 2,000 shared
    assert int(hdr[G.H_OVERFLOW]) == 0 and 3900 < int(hdr[G.H_NKEYS]) == len(want.keys) <= 4000
    _equal_groups(G, got, want)


def test_wrapper_refuses(S):
    from nvme_strom_amd.ops import colagg as A
    from nvme_strom_amd.ops import colgroup as G
    with pytest.raises(ValueError):
        G.DeviceGroups([A.Entry(A.COUNT | A.ALL)], 0, "cuda")
    with pytest.raises(ValueError):
        G.DeviceGroups([A.Entry(A.COUNT | A.ALL)], (1 << 24) + 1, "cuda")
    tab = _Tab(seed=1)
    key = tab.column(lambda n: np.zeros(n))
    t = G.DeviceGroups([A.Entry(A.COUNT | A.ALL)], 8, "cuda")
    bm = torch.zeros(tab.nwords, dtype=torch.int64, device="cuda")
    with pytest.raises(NotImplementedError):
        G.group_codes(t, A.VALUE_CODE["f8"], key[1], tab.nwords, bm, bm, tab.ctab)


# ------------------------------------------------------------ whole scans
@pytest.mark.parametrize("col,refcol", [("i64", "i64"), ("u32", "u32"), ("i8", "i8"),
                                        ("ts", "ts_ticks"), ("d32", "d32_ticks")])
@pytest.mark.parametrize("codec", [None, "lz4", "zstd"])
def test_hash_aggregate_query_matrix(S, tmp_path, codec, col, refcol):
    """The CPU file's matrix (qualifier lists x key columns) through the
    kernels, against pyarrow and against the host twin."""
    from agggen import same_results
    from arrowgen import write
    from hashagggen import AGGS, BATCH_ROWS, check, qual_lists, sorted_keys, tables
    from nvme_strom_amd.models.arrow_scan import ArrowScan, HashBy
    tbl, _ = tables()
    path = str(tmp_path / f"h_{codec}.arrow")
    write(path, tbl, codec, batch_rows=BATCH_ROWS)
    sc = ArrowScan(path, "cuda", chunk_sz=64 << 10, slot_bytes=1 << 20)
    try:
        for label, quals, ref in qual_lists():
            by = HashBy(col, groups=1 << 13)
            out = sc.aggregate(quals, AGGS, by=by)
            assert out.rows == tbl.num_rows and out.groups >= 1 and out.by == col
            check(out, label, ref, refcol)
            sorted_keys(out, unsigned=col == "u32")
            same_results(out, sc.host_aggregate(quals, AGGS, by=by))
        # a bare integer key is still refused, by name
        with pytest.raises(NotImplementedError, match="i64"):
            sc.aggregate([], [("count", None)], by="i64")
        for col in ("f64", "s", "dict", "dec", "b"):
            with pytest.raises(NotImplementedError, match=col):
                sc.aggregate([], [("count", None)], by=HashBy(col))
    finally:
        sc.close()


def test_merge_overflow_and_reuse(S, tmp_path):
    """Merged batches= ranges equal the whole scan (and a GPU result merges
    with a host one); too many keys raise at the sync and the scan object
    works afterwards."""
    from agggen import same_results
    from arrowgen import write
    from hashagggen import AGGS, BATCH_ROWS, check, distinct, qual_lists, tables
    from nvme_strom_amd.models.arrow_scan import ArrowScan, HashBy
    from nvme_strom_amd.ops.colpred import P
    tbl, _ = tables()
    path = str(tmp_path / "m.arrow")
    write(path, tbl, None, batch_rows=BATCH_ROWS)
    sc = ArrowScan(path, "cuda", chunk_sz=64 << 10, slot_bytes=1 << 20)
    try:
        quals = [P("f64") > 0.4]
        full = sc.aggregate(quals, AGGS, by=HashBy("i64", 8000))
        parts = [sc.aggregate(quals, AGGS, by=HashBy("i64", g), batches=r)
                 for r, g in (((0, 2), 2000), ((2, 2), 1))]
        parts.append(sc.host_aggregate(quals, AGGS, by=HashBy("i64", 4000), batches=(2, 6)))
        got = parts[0].merge(parts[1]).merge(parts[2])
        assert got.rows == full.rows
        same_results(got, full)
        check(got, "one", qual_lists()[1][2], "i64")
        with pytest.raises(ValueError):
            sc.aggregate(quals, AGGS, by=HashBy("i8")).merge(sc.aggregate(quals, AGGS, by="i8"))
        aggs = [("count", None), ("sum", "f64")]
        n = distinct(tbl, "i64")
        out = sc.aggregate([], aggs, by=HashBy("i64", groups=n))
        assert len([k for k in out.keys if k is not None]) == n
        with pytest.raises(RuntimeError, match=rf"i64.*groups={n - 1}\b.*\b{n} distinct"):
            sc.aggregate([], aggs, by=HashBy("i64", groups=n - 1))
        # a table too small for the keys to fit at all: rows overflow
        with pytest.raises(RuntimeError, match=r"i64.*groups=100\b"):
            sc.aggregate([], aggs, by=HashBy("i64", groups=100))
        same_results(sc.aggregate([], aggs, by=HashBy("i64", groups=n)), out)
    finally:
        sc.close()


def test_more_groups_than_slots(S, tmp_path):
    """200,000 rows in batches of 4,093 with an int64 key of 50,000 distinct
    values plus nulls: more scan groups than ring slots, so the table lives
    across reused slots."""
    from agggen import same_results
    from arrowgen import write
    from hashagggen import BIG_AGGS, big_table, check_by_runs
    from nvme_strom_amd.models.arrow_scan import ArrowScan, HashBy
    from nvme_strom_amd.ops.colpred import P
    tbl = big_table()
    path = str(tmp_path / "big.arrow")
    write(path, tbl, None, batch_rows=4093)
    tight = ArrowScan(path, "cuda", chunk_sz=64 << 10, slot_bytes=1 << 20)
    tight.MAX_SLOTS = 2                    # the ring at its minimum: every slot reused
    try:
        by = HashBy("k", groups=50_000)
        g = tight.aggregate([], BIG_AGGS, by=by)
        assert g.groups > len(tight._slots) and len(g.keys) == 50_001 and g.keys[-1] is None
        check_by_runs(g, tbl, "k", BIG_AGGS)
        same_results(g, tight.host_aggregate([], BIG_AGGS, by=by))
        # every kind of query in turn on the one object: they share the slots'
        # kept tensors, events, counts and key buffer, and the emit stream
        quals = [P("c") > 0]
        rows = tight.scan_where(quals, project="a")
        flat = tight.aggregate(quals, BIG_AGGS)
        hashed = tight.aggregate(quals, BIG_AGGS, by=by)
        again = tight.scan_where(quals, project="a")
        assert rows.groups > len(tight._slots) and 0 < rows.selected < tbl.num_rows
        ref = tight.host_scan_where(quals, project="a")
        for out in (rows, again):
            assert np.array_equal(out.indices.cpu().numpy(), ref.indices)
            assert np.array_equal(out.values.cpu().numpy(), ref.values)
        same_results(flat, tight.host_aggregate(quals, BIG_AGGS))
        same_results(hashed, tight.host_aggregate(quals, BIG_AGGS, by=by))
    finally:
        tight.close()


@pytest.mark.parametrize("how", ["semi", "anti"])
def test_join_then_hash(S, tmp_path, how):
    """join=Join(fk, dim, how) with by=HashBy("u32"): the hash step runs on
    the bitmap the probe left; against pyarrow's join + group_by."""
    import pyarrow.compute as pc
    from agggen import same_results
    from arrowgen import write
    from hashagggen import BATCH_ROWS, check, tables
    from joingen import dimension, joined
    from nvme_strom_amd.models.arrow_scan import ArrowScan, HashBy, Join, JoinTable
    from nvme_strom_amd.ops.colpred import P
    tbl, _ = tables()
    path = str(tmp_path / "j.arrow")
    write(path, tbl, None, batch_rows=BATCH_ROWS)
    keys, cats, regs = dimension(tbl.column("i64").combine_chunks())
    aggs = [("count", None), ("sum", "i64"), ("min", "f64"), ("max", "f64"), ("sum", "f64"),
            ("count", "i8")]
    j = joined(tbl, "i64", keys, {}, "left " + how)
    sc = ArrowScan(path, "cuda", chunk_sz=64 << 10, slot_bytes=1 << 20)
    dim = JoinTable(keys, device="cuda")
    try:
        for label, quals, ref in (("all", [], None),
                                  ("f64", [P("f64") > 0.4],
                                   lambda t: pc.greater(t.column("f64").combine_chunks(), 0.4))):
            by = HashBy("u32", groups=1 << 13)
            out = sc.aggregate(quals, aggs, by=by, join=Join("i64", dim, how))
            assert out.selected > 100
            check(out, label, ref, "u32", aggs, tbl=j, tag="join-" + how)
            same_results(out, sc.host_aggregate(quals, aggs, by=by, join=Join("i64", dim, how)))
    finally:
        dim.close()
        sc.close()
