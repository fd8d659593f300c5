"""Hash GROUP BY on several key columns on the GPU (strom_group_codes_multi in
csrc/kernels/colgroup.hip): the kernel alone through ops/colgroup.py on
hand-built batch tables against the numpy twin — by packed key, never slot
by slot — and whole scans with by=HashBy([...]) against pyarrow and the host
twin under the comparison rule of tests/agggen.py."""
import dataclasses
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))

from test_gpu_arrow_hashagg import ROWS, _entries, _equal_groups, _Tab  # noqa: E402

EMPTY = 1 << 63


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nvme_strom_amd as S
    S.configure(gpu_emulation=0)
    return S


# ------------------------------------------------------------ kernel alone
def _pool(r, c, extra=5):
    """A few values of component ``c``, the ends of its declared range and 0
    among them: many rows share a component."""
    lo, hi = (-(1 << (c.bits - 1)), (1 << (c.bits - 1)) - 1) if c.signed else (0, (1 << c.bits) - 1)
    dt = np.dtype(c.storage)
    return np.concatenate([np.array([lo, hi, 0], dt), r.integers(lo, hi, extra, endpoint=True, dtype=dt)])


def _drop_valid(col, b):
    """Batch ``b`` of a column loses its validity buffer (pointer 0: every
    row valid), the other batches keep theirs."""
    host, t = col
    host[b] = (host[b][0], None)
    t[b, 1] = 0
    return col


def _launch(G, t, tab, comps, sel_h, src_words, in_place, before=None, stream=None):
    """strom_group_codes_multi over ``tab`` with ``t.spec``; checks the
    destination bitmap and the codes against the twin's packing, returns
    (rows that kept a code per batch, {packed key: code}, rows per component
    that did not fit)."""
    spec = t.spec
    ktab = torch.stack([c[1] for c in comps]).contiguous()
    src = torch.from_numpy(src_words.view(np.int64).copy()).cuda()
    dst = src if in_place else torch.full_like(src, 0x1234)
    if before is None:
        tab.kbuf.fill_(-77)
    before = tab.codes()
    before = [b.copy() for b in before]
    torch.cuda.synchronize()
    G.group_codes_multi(t, ktab, tab.nwords, src, dst, tab.ctab, stream=stream)
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
    misfit = np.zeros(len(spec), np.int64)
    for b, (sel, kept, codes, was) in enumerate(zip(sel_h, got, tab.codes(), before)):
        packed, bad = spec.pack_why([c[0][b][0] for c in comps], [c[0][b][1] for c in comps])
        assert not (kept & ~sel).any()
        assert np.array_equal(codes[~sel], was[~sel])  # only selected rows are written
        assert not (kept & (bad >= 0)).any()           # what does not fit is cleared
        assert (codes[sel & ~kept] == 0).all()         # no code: 0, bit cleared
        misfit += np.bincount(bad[sel & (bad >= 0)].astype(np.int64), minlength=len(spec))
        for p, c in zip(packed[kept].tolist(), codes[kept].tolist()):
            assert code_of.setdefault(p, c) == c       # one code per packed key
            if p == EMPTY:
                assert c == C + 1
            else:
                assert 0 <= c < C and int(slots[c]) == p   # never the null code C
    assert len(set(code_of.values())) == len(code_of)  # distinct keys, distinct codes
    return got, code_of, misfit


def _run(G, tab, spec, comps, ents, data, sel, groups, in_place=True, overflow=False, before=None):
    """codes + every entry's accumulate + compaction against the twin; the
    header counters; returns (header, device Groups, {packed key: code})."""
    sel_h, src_words = sel
    t = G.DeviceGroups(ents, groups, "cuda", spec=spec)
    # the twin's packing of the rows as they are before the launch (in place
    # over the code buffer the launch overwrites a component)
    packs = [spec.pack_why([c[0][b][0] for c in comps], [c[0][b][1] for c in comps])
             for b in range(len(tab.rows))]
    kept, code_of, misfit = _launch(G, t, tab, comps, sel_h, src_words, in_place, before)
    bm = torch.from_numpy(np.concatenate(
        [np.packbits(np.pad(k, (0, -len(k) % 64)), bitorder="little") for k in kept]
    ).view(np.int64).copy()).cuda()
    for e, (_, vt) in enumerate(data):
        G.group_agg(t, e, bm, tab.nwords, vt, tab.ctab)
    hdr, got = G.compact(t)
    torch.cuda.synchronize()
    dropped = sum(int((s & (bad < 0) & ~k).sum()) for s, k, (_, bad) in zip(sel_h, kept, packs))
    assert int(hdr[G.H_CAPACITY]) == G.capacity(groups) == t.capacity
    assert int(hdr[G.H_OVERFLOW]) == dropped and (dropped > 0) == overflow
    assert int(hdr[G.H_NKEYS]) == len(code_of)
    assert bool(hdr[G.H_HAS_EMPTY]) == (EMPTY in code_of)
    assert hdr[G.H_RANGE:G.H_RANGE + len(spec)].tolist() == misfit.tolist()
    assert (hdr[G.H_RANGE + len(spec):] == 0).all()
    want = G.empty_groups(ents, spec=spec)
    for b in range(len(kept)):
        part, _ = G.host_group_agg_multi(ents, kept[b], spec, [c[0][b][0] for c in comps],
                                         [c[0][b][1] for c in comps],
                                         [(h[b][0], h[b][1]) for h, _ in data])
        want = G.merge(want, part)
    assert len(want.keys) == len(code_of) and got.spec == spec
    assert want.arrays(0)["count"][-1] == 0           # the null code's slot stays empty
    _equal_groups(G, got, want)
    return hdr, got, code_of


SHAPES = {
    "i8": [("a", "i8", None, False)],                       # v = 0 packs to the free slot's pattern
    "u8?": [("a", "u8", 63, True)],
    "i4-u4": [("a", "i4", None, False), ("b", "u4", None, False)],      # 64 bits, (0, 0) = free
    "i1?-u2-i2?": [("a", "i1", None, True), ("b", "u2", None, False), ("c", "i2", None, True)],
    "u1-i2?-u4?-i1?": [("a", "u1", 3, False), ("b", "i2", None, True), ("c", "u4", None, True),
                       ("d", "i1", 6, True)],
}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("in_place", [True, False])
def test_every_storage_type(S, shape, in_place):
    """1-4 components over the eight storage types, nulls in the nullable
    ones — but batch 1 of the first nullable component has no validity
    buffer, and the other nullable ones have none in batch 2; garbage in the
    bitmap's tail bits."""
    from nvme_strom_amd.ops import colagg as A
    from nvme_strom_amd.ops import colgroup as G
    spec = G.KeySpec(SHAPES[shape])
    tab = _Tab(seed=31)
    r = tab.rng
    comps = []
    for i, c in enumerate(spec.comps):
        vals = r.choice(_pool(r, c), sum(ROWS))
        vals[:8] = 0                                  # rows of all zeros: (0, 0) packs to 1 << 63
        col = tab.column(vals, null_p=0.15 if c.nullable else 0.0)
        if c.nullable:
            first = not any(k.nullable for k in spec.comps[:i])
            _drop_valid(col, 1 if first else 2)
        comps.append(col)
    ents, data = _entries(A, tab, r)
    hdr, got, code_of = _run(G, tab, spec, comps, ents, data, tab.bitmap(0.8), 4096, in_place)
    assert len(code_of) >= 4 and int(hdr[G.H_OVERFLOW]) == 0
    if shape in ("i8", "i4-u4"):
        assert EMPTY in code_of and bool(hdr[G.H_HAS_EMPTY])
    vals, oks = spec.unpack(got.keys)
    for c, ok in zip(spec.comps, oks):
        assert (not ok.all()) == c.nullable           # nulls where there can be any
    assert (np.diff(got.keys.astype(object)) > 0).all()


def test_all_null_component(S):
    from nvme_strom_amd.ops import colagg as A
    from nvme_strom_amd.ops import colgroup as G
    spec = G.KeySpec([("a", "i2", None, True), ("b", "u1", None, False)])
    tab = _Tab(seed=33)
    r = tab.rng
    comps = [tab.column(lambda n: r.integers(-5, 5, n).astype(np.int16), all_null=True),
             tab.column(lambda n: r.integers(0, 7, n).astype(np.uint8))]
    ents, data = _entries(A, tab, r)
    hdr, got, code_of = _run(G, tab, spec, comps, ents, data, tab.bitmap(0.9), 16)
    vals, oks = spec.unpack(got.keys)
    assert not oks[0].any() and vals[1].tolist() == list(range(7))
    for c in tab.codes():
        assert G.capacity(16) not in set(c.tolist())  # the null code is never written


def _split64(packed):
    """(int32, uint32) columns whose packing under (i4, u4) is ``packed``."""
    p = np.asarray(packed).astype(np.int64).view(np.uint64)
    return ((p >> np.uint64(32)).astype(np.int64) - (1 << 31)).astype(np.int32), \
        (p & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def test_chain_wrap_full_and_over_full(S):
    """Packed words chosen by their home slot: 200 on one slot of a 512-slot
    table; chains that wrap a 64-slot table; then exactly groups keys, and 40
    keys into 16 slots."""
    from joingen import keys_with_home
    from nvme_strom_amd.ops import colagg as A
    from nvme_strom_amd.ops import colgroup as G
    spec = G.KeySpec(SHAPES["i4-u4"])
    for keys, groups in ((keys_with_home(300, 512, 200), 256),
                         (np.concatenate([keys_with_home(63, 64, 9),
                                          keys_with_home(62, 64, 3, 10**7)]), 32)):
        tab = _Tab(seed=35)
        r = tab.rng
        a, b = _split64(np.resize(r.permutation(keys), sum(ROWS)))
        comps = [tab.column(a), tab.column(b)]
        ents, data = _entries(A, tab, r)
        hdr, got, code_of = _run(G, tab, spec, comps, ents, data, tab.bitmap(0.95), groups)
        assert sorted(code_of) == sorted(keys.tolist())
        cap = G.capacity(groups)
        home = (G.hash64(keys) & np.uint64(cap - 1)).astype(np.int64)
        disp = (np.array([code_of[int(k)] for k in keys]) - home) % cap
        assert sorted(disp.tolist())[-1] >= len(keys) - 4
    tab = _Tab(seed=37)
    r = tab.rng
    ents, data = _entries(A, tab, r)
    pa_, pb_ = r.integers(-2**31, 2**31, 40).astype(np.int32), np.arange(40, dtype=np.uint32) * 10**8
    pick = r.integers(0, 32, sum(ROWS))
    pick[:32] = np.arange(32)
    comps = [tab.column(pa_[pick]), tab.column(pb_[pick])]
    hdr, got, code_of = _run(G, tab, spec, comps, ents, data, tab.bitmap(1.0), 32)
    assert int(hdr[G.H_NKEYS]) == 32 and int(hdr[G.H_OVERFLOW]) == 0
    pick = r.integers(0, 40, sum(ROWS))
    comps = [tab.column(pa_[pick]), tab.column(pb_[pick])]
    for in_place in (True, False):
        hdr, got, code_of = _run(G, tab, spec, comps, ents, data, tab.bitmap(0.9), 8, in_place,
                                 overflow=True)
        assert int(hdr[G.H_NKEYS]) == 16 and int(hdr[G.H_OVERFLOW]) > 0


def test_out_of_range_in_tail_words(S):
    """Component 1 of 3 declared 10 bits wide: values outside it in the tail
    word of batch 0 (rows 960-999) and in batch 2's only, partial word; a null
    in component 2, which is not nullable, counts there."""
    from nvme_strom_amd.ops import colagg as A
    from nvme_strom_amd.ops import colgroup as G
    spec = G.KeySpec([("a", "u1", None, False), ("b", "i4", 10, True), ("c", "u2", None, False)])
    for in_place in (True, False):
        tab = _Tab(seed=39)
        r = tab.rng
        b = r.integers(-512, 512, sum(ROWS)).astype(np.int32)
        out = np.array([961, 975, 999, 1000 + 64 + 3, 1000 + 64 + 40])
        b[out] = [512, -513, 2**31 - 1, -2**31, 70000]
        comps = [tab.column(lambda n: r.integers(0, 3, n).astype(np.uint8)),
                 tab.column(b, null_p=0.1),
                 tab.column(lambda n: r.integers(0, 4, n).astype(np.uint16))]
        for bi, row in ((0, 961), (0, 975), (0, 999), (2, 3), (2, 40)):
            comps[1][0][bi][1][row] = True            # those rows are not null
        # the validity went up with the column: rebuild it with those rows valid
        comps[1] = _revalid(tab, comps[1])
        sel_h, words = tab.bitmap(1.0)
        ents, data = _entries(A, tab, r)
        hdr, got, code_of = _run(G, tab, spec, comps, ents, data, (sel_h, words), 4096, in_place)
        assert hdr[G.H_RANGE:].tolist() == [0, 5, 0, 0]
    # a null where the spec has no null bit
    tab = _Tab(seed=41)
    r = tab.rng
    comps = [tab.column(lambda n: r.integers(0, 3, n).astype(np.uint8)),
             tab.column(lambda n: r.integers(-5, 5, n).astype(np.int32)),
             tab.column(lambda n: r.integers(0, 4, n).astype(np.uint16), null_p=0.05)]
    ents, data = _entries(A, tab, r)
    sel = tab.bitmap(1.0)
    hdr, got, code_of = _run(G, tab, G.KeySpec([("a", "u1", None, False), ("b", "i4", 10, False),
                                                ("c", "u2", None, False)]),
                             comps, ents, data, sel, 4096)
    nulls = sum(int((~h[1]).sum()) for h in comps[2][0])
    assert nulls > 10 and hdr[G.H_RANGE:].tolist() == [0, 0, nulls, 0]


def _revalid(tab, col):
    """The column's device table with validity buffers rebuilt from the
    host's (edited) bool arrays."""
    host, t = col
    tnp = t.cpu().numpy().copy()
    for b, (v, ok) in enumerate(host):
        bits = np.zeros(((len(ok) + 63) // 64) * 64, np.uint8)
        bits[:len(ok)] = ok
        dv = torch.from_numpy(np.packbits(bits, bitorder="little").copy()).cuda()
        tab.keep.append(dv)
        tnp[b, 1] = dv.data_ptr()
    t2 = torch.from_numpy(tnp).cuda()
    tab.keep.append(t2)
    return host, t2


@pytest.mark.parametrize("in_place", [True, False])
def test_component_in_the_code_buffer(S, in_place):
    """What the scan does with a join attribute: component 0's values are the
    int32 buffers the codes are written to (the probe left the attribute's
    codes there).  Every lane reads its row before it stores its code."""
    from nvme_strom_amd.ops import colagg as A
    from nvme_strom_amd.ops import colgroup as G
    spec = G.KeySpec([("attr", "u4", 3, False), ("b", "i2", None, True)])
    tab = _Tab(seed=43)
    r = tab.rng
    attr = r.integers(0, 7, tab.nwords * 64).astype(np.int32)
    tab.kbuf.copy_(torch.from_numpy(attr))
    host = [(attr[int(wb) * 64:int(wb) * 64 + n].astype(np.uint32), None)
            for wb, n in zip(tab.word_base, tab.rows)]
    comps = [(host, tab.ctab), tab.column(lambda n: r.integers(-3, 3, n).astype(np.int16), null_p=0.1)]
    ents, data = _entries(A, tab, r)
    hdr, got, code_of = _run(G, tab, spec, comps, ents, data, tab.bitmap(0.85), 256, in_place,
                             before=True)
    vals, oks = spec.unpack(got.keys)
    assert sorted(set(vals[0].tolist())) == list(range(7)) and len(code_of) > 40


def test_two_streams_on_one_table(S):
    """Overlapping tuple sets from two streams into one table, then one
    compaction: the scan's slot streams."""
    from nvme_strom_amd.ops import colagg as A
    from nvme_strom_amd.ops import colgroup as G
    spec = G.KeySpec([("a", "i4", 20, True), ("b", "u2", None, False)])
    ents = [A.Entry(A.COUNT | A.ALL), A.Entry(15, "i8")]
    t = G.DeviceGroups(ents, 8192, "cuda", spec=spec)
    torch.cuda.synchronize()
    parts, streams = [], [torch.cuda.Stream(), torch.cuda.Stream()]
    for i in range(2):
        tab = _Tab(rows=(30_000, 2_041), seed=50 + i)
        r = tab.rng
        comps = [tab.column(lambda n: r.integers(100 * i, 100 * i + 300, n).astype(np.int32),
                            null_p=0.05),
                 tab.column(lambda n: r.integers(0, 10, n).astype(np.uint16))]
        data = [tab.column(lambda n: np.zeros(n, np.int8)),
                tab.column(lambda n: r.integers(-2**40, 2**40, n), null_p=0.1)]
        sel_h, words = tab.bitmap(0.9)
        bm = torch.from_numpy(words.view(np.int64).copy()).cuda()
        ktab = torch.stack([c[1] for c in comps]).contiguous()
        parts.append((tab, comps, data, sel_h, bm, ktab))
    torch.cuda.synchronize()
    for (tab, comps, data, sel_h, bm, ktab), st in zip(parts, streams):
        with torch.cuda.stream(st):
            G.group_codes_multi(t, ktab, tab.nwords, bm, bm, tab.ctab, stream=st)
            for e, (_, vt) in enumerate(data):
                G.group_agg(t, e, bm, tab.nwords, vt, tab.ctab, stream=st)
    torch.cuda.synchronize()
    hdr, got = G.compact(t)
    want = G.empty_groups(ents, spec=spec)
    for tab, comps, data, sel_h, bm, ktab in parts:
        for b in range(len(tab.rows)):
            part, bad = G.host_group_agg_multi(ents, sel_h[b], spec, [c[0][b][0] for c in comps],
                                               [c[0][b][1] for c in comps],
                                               [(h[b][0], h[b][1]) for h, _ in data])
            assert not bad.any()
            want = G.merge(want, part)
    # a in 0..299 and 100..399 plus null, b in 0..9: 2,010 shared tuples
    assert int(hdr[G.H_OVERFLOW]) == 0 and 3900 < int(hdr[G.H_NKEYS]) == len(want.keys) <= 4010
    assert (hdr[G.H_RANGE:] == 0).all()
    _equal_groups(G, got, want)


def test_wrapper_refuses(S):
    from nvme_strom_amd.ops import colagg as A
    from nvme_strom_amd.ops import colgroup as G
    tab = _Tab(seed=1)
    key = tab.column(lambda n: np.zeros(n, np.int32))
    bm = torch.zeros(tab.nwords, dtype=torch.int64, device="cuda")
    plain = G.DeviceGroups([A.Entry(A.COUNT | A.ALL)], 8, "cuda")
    with pytest.raises(ValueError, match="KeySpec"):
        G.group_codes_multi(plain, key[1][None], tab.nwords, bm, bm, tab.ctab)
    t = G.DeviceGroups([A.Entry(A.COUNT | A.ALL)], 8, "cuda",
                       spec=G.KeySpec([("a", "i4", None, False), ("b", "i4", 8, False)]))
    with pytest.raises(ValueError, match="keys"):
        G.group_codes_multi(t, key[1][None], tab.nwords, bm, bm, tab.ctab)   # one table for two


# ------------------------------------------------------------ whole scans
@pytest.mark.parametrize("kl", range(4))
@pytest.mark.parametrize("codec", [None, "lz4", "zstd"])
def test_multikey_query_matrix(S, tmp_path, codec, kl):
    """The CPU file's matrix (qualifier lists x key lists) through the
    kernels, against pyarrow and against the host twin."""
    from agggen import same_results
    from arrowgen import write
    from multikeygen import AGGS, BATCH_ROWS, KEY_LISTS, check, hash_by, qual_lists, table
    from nvme_strom_amd.models.arrow_scan import ArrowScan
    tbl = table()
    keys, bits = KEY_LISTS[kl]
    path = str(tmp_path / f"m_{codec}.arrow")
    write(path, tbl, codec, batch_rows=BATCH_ROWS)
    sc = ArrowScan(path, "cuda", chunk_sz=64 << 10, slot_bytes=1 << 20)
    try:
        for label, quals, ref in qual_lists():
            by = hash_by(keys, bits)
            out = sc.aggregate(quals, AGGS, by=by)
            assert out.rows == tbl.num_rows and out.groups >= 1 and out.by == tuple(keys)
            check(out, label, ref, keys)
            same_results(out, sc.host_aggregate(quals, AGGS, by=by))
    finally:
        sc.close()


def _pairs_table(n=200_000, seed=61):
    """(int32, int32) pairs: all 250 x 200 = 50,000 of a grid, each at least
    once; an int64, a float64 with nulls and an int32 value column."""
    rng = np.random.default_rng(seed)
    a = rng.choice(np.arange(-2**31, 2**31, 2**32 // 250, dtype=np.int64), 250, replace=False)
    b = rng.integers(-2**31, 2**31, 400)
    b = np.unique(b)[:200]
    grid = rng.permutation(np.stack(np.meshgrid(a, b), -1).reshape(-1, 2))
    pick = rng.integers(0, len(grid), n)
    pick[:len(grid)] = np.arange(len(grid))
    pick = rng.permutation(pick)
    return pa.table({"a": pa.array(grid[pick, 0].astype(np.int32)),
                     "b": pa.array(grid[pick, 1].astype(np.int32)),
                     "v": pa.array(rng.integers(-10**15, 10**15, n)),
                     "x": pa.array(rng.normal(0, 1e3, n), mask=rng.random(n) < 0.1),
                     "c": pa.array(rng.integers(-10**6, 10**6, n).astype(np.int32))})


def test_more_groups_than_slots(S, tmp_path):
    """200,000 rows in batches of 4,093 with 50,000 distinct (int32, int32)
    pairs: more scan groups than ring slots, so the table lives across reused
    slots; groups= just large enough passes, one fewer raises at the sync."""
    from agggen import same_results
    from arrowgen import write
    from hashagggen import check_by_runs
    from nvme_strom_amd.models.arrow_scan import ArrowScan, HashBy
    aggs = [("count", None), ("sum", "v"), ("min", "v"), ("max", "v"), ("sum", "x"), ("min", "x"),
            ("max", "x"), ("count", "x"), ("mean", "x"), ("sum", "c"), ("max", "c")]
    tbl = _pairs_table()
    path = str(tmp_path / "pairs.arrow")
    write(path, tbl, None, batch_rows=4093)
    tight = ArrowScan(path, "cuda", chunk_sz=64 << 10, slot_bytes=1 << 20)
    tight.MAX_SLOTS = 2                    # the ring at its minimum: every slot reused
    try:
        by = HashBy(["a", "b"], groups=50_000)
        g = tight.aggregate([], aggs, by=by)
        assert g.groups > len(tight._slots) and len(g.keys) == 50_000
        assert g.keys == sorted(g.keys) and g.key_columns[0][0].dtype == np.int32
        # one int64 column that orders as the pairs do, for the single-key checker
        one = np.asarray(tbl.column("a")).astype(np.int64) * 2**32 + \
            np.asarray(tbl.column("b")).astype(np.int64) + 2**31
        flat = dataclasses.replace(g, keys=[a * 2**32 + b + 2**31 for a, b in g.keys])
        check_by_runs(flat, tbl.append_column("k", pa.array(one)), "k", aggs)
        same_results(g, tight.host_aggregate([], aggs, by=by))
        with pytest.raises(RuntimeError, match=r"groups=49999\b"):
            tight.aggregate([], aggs[:2], by=HashBy(["a", "b"], groups=49_999))
        assert len(tight.aggregate([], aggs[:2], by=by).keys) == 50_000   # and works afterwards
    finally:
        tight.close()


def test_join_attribute_component(S, tmp_path):
    """[dim["cat"], "kd"] and ["ku8", dim["reg"], "klate"] after the semi-join:
    the probe leaves the attribute's codes in the slot's key buffer and the
    composite launch runs in place over it."""
    import pyarrow.compute as pc
    from agggen import same_results
    from arrowgen import write
    from joingen import dimension, joined
    from multikeygen import BATCH_ROWS, check, table
    from nvme_strom_amd.models.arrow_scan import ArrowScan, HashBy, Join, JoinTable
    from nvme_strom_amd.ops.colpred import P
    from test_arrow_multikey_cpu import JOIN_AGGS
    tbl = table()
    path = str(tmp_path / "j.arrow")
    write(path, tbl, None, batch_rows=BATCH_ROWS)
    keys, cats, regs = dimension(tbl.column("i64").combine_chunks())
    j = joined(tbl, "i64", keys, {"cat": cats, "reg": regs}, "inner")
    sc = ArrowScan(path, "cuda", chunk_sz=64 << 10, slot_bytes=1 << 20)
    dim = JoinTable(keys, {"cat": cats, "reg": regs}, device="cuda")
    rank = lambda a: {v: i for i, v in enumerate(a.values)}.get
    try:
        for label, quals, ref in (("all", [], None),
                                  ("f64", [P("f64") > 0.4],
                                   lambda t: pc.greater(t.column("f64").combine_chunks(), 0.4))):
            for comps, names, rk in (([dim["cat"], "kd"], ("cat", "kd"), [rank(dim["cat"]), None]),
                                     (["ku8", dim["reg"], "klate"], ("ku8", "reg", "klate"),
                                      [None, rank(dim["reg"]), None])):
                by = HashBy(comps)
                out = sc.aggregate(quals, JOIN_AGGS, by=by, join=Join("i64", dim))
                assert out.selected > 100
                check(out, label, ref, names, JOIN_AGGS, tbl=j, tag="join", rank=rk)
                same_results(out, sc.host_aggregate(quals, JOIN_AGGS, by=by, join=Join("i64", dim)))
    finally:
        dim.close()
        sc.close()


def test_merge_ranges_and_range_error(S, tmp_path):
    """Merged batches= ranges equal the whole scan (a GPU result merges with
    a host one; the first range has no null in klate and still packs it
    nullable); a value outside its declared bits raises at the sync, names
    the column, and the scan object works afterwards."""
    import pyarrow.compute as pc
    from agggen import same_results
    from arrowgen import write
    from multikeygen import AGGS, BATCH_ROWS, KEY_LISTS, check, hash_by, qual_lists, table
    from nvme_strom_amd.models.arrow_scan import ArrowScan, HashBy
    from nvme_strom_amd.ops.colpred import P
    tbl = table()
    path = str(tmp_path / "m.arrow")
    write(path, tbl, None, batch_rows=BATCH_ROWS)
    keys, bits = KEY_LISTS[3]
    sc = ArrowScan(path, "cuda", chunk_sz=64 << 10, slot_bytes=1 << 20)
    try:
        quals = [P("f64") > 0.4]
        full = sc.aggregate(quals, AGGS, by=hash_by(keys, bits))
        parts = [sc.aggregate(quals, AGGS, by=hash_by(keys, bits, g), batches=r)
                 for r, g in (((0, 3), 2000), ((3, 3), 1))]
        parts.append(sc.host_aggregate(quals, AGGS, by=hash_by(keys, bits), batches=(3, 6)))
        assert parts[0]._found.spec == full._found.spec and parts[0]._found.spec.comps[3].nullable
        got = parts[0].merge(parts[1]).merge(parts[2])
        assert got.rows == full.rows
        same_results(got, full)
        check(got, "one", qual_lists()[1][2], keys)
        k64 = tbl.column("k64").combine_chunks()
        n = pc.sum(pc.or_(pc.less(k64, -2**19), pc.greater_equal(k64, 2**19))).as_py()
        by = HashBy(["ku8", "k64"], bits={"k64": 20})
        with pytest.raises(RuntimeError, match=rf"k64.*bits=20\b.*\b{n} selected row"):
            sc.aggregate([], [("count", None)], by=by)
        out = sc.aggregate([P("k64").between(-2**19, 2**19 - 1)], [("count", None)], by=by)
        same_results(out, sc.host_aggregate([P("k64").between(-2**19, 2**19 - 1)],
                                            [("count", None)], by=by))
    finally:
        sc.close()
