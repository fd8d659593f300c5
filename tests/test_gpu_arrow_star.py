"""The Arrow scan's star join on the GPU (strom_column_join_star,
csrc/kernels/coljoin.hip): the kernel alone on hand-built batch tables against
its numpy twin, bit for bit, and whole scans with ``join=StarJoin(...)``
against pyarrow's Table.join chained leg by leg and the host twins."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))

import stargen as G  # noqa: E402


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nvme_strom_amd as S
    S.configure(gpu_emulation=0)
    return S


# ------------------------------------------------------------ kernel alone
def _popcount(words) -> int:
    return int(np.unpackbits(np.asarray(words).view(np.uint8)).sum())


def _payloads(keys: np.ndarray, leg: int) -> np.ndarray:
    return ((np.arange(len(keys)) * 7 + leg) % 1000).astype(np.int32)


class _Launch:
    """A stargen case on the device: tables, the legs' batch tables, the
    code buffers (one per code table, prefilled) and their batch tables."""

    def __init__(self, J, c, built: dict):
        self.c = c
        self.rows = list(G.BATCH_ROWS)
        words = [(r + 63) // 64 for r in self.rows]
        self.word_base = np.concatenate([[0], np.cumsum(words)[:-1]]).astype(np.int64)
        self.nwords = int(sum(words))
        self.keep = []
        self.dev, self.host = [], []
        for i, keys in enumerate(c["keys"]):
            tag = (keys.tobytes(), i)
            if tag not in built:
                dk = torch.from_numpy(np.ascontiguousarray(keys, np.int64)).cuda()
                dp = torch.from_numpy(_payloads(keys, i)).cuda()
                d = J.build(dk, dp)
                torch.cuda.synchronize()
                built[tag] = (d, d.to_host())
            self.dev.append(built[tag][0])
            self.host.append(built[tag][1])
        nlegs = len(c["keys"])
        tab = np.zeros((nlegs, len(self.rows), 5), np.int64)
        for i in range(nlegs):
            for b, n in enumerate(self.rows):
                v, ok = c["fks"][i][b]
                vptr = 0
                if ok is not None:
                    bits = np.zeros(((n + 63) // 64) * 64, np.uint8)
                    bits[:n] = ok
                    dv = torch.from_numpy(np.packbits(bits, bitorder="little").copy()).cuda()
                    self.keep.append(dv)
                    vptr = dv.data_ptr()
                d = torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).copy()).cuda()
                self.keep.append(d)
                tab[i, b] = (d.data_ptr(), vptr, n, self.word_base[b], 0)
        self.tab = torch.from_numpy(tab).cuda()
        self.nout = max(c["kouts"]) + 1
        self.kbuf = [torch.empty(self.nwords * 64, dtype=torch.int32, device="cuda")
                     for _ in range(self.nout)]
        ktab = np.zeros((max(self.nout, 1), len(self.rows), 5), np.int64)
        for j in range(self.nout):
            for b, n in enumerate(self.rows):
                ktab[j, b] = (self.kbuf[j].data_ptr() + int(self.word_base[b]) * 256, 0, n,
                              self.word_base[b], 0)
        self.ktab = torch.from_numpy(ktab).cuda() if self.nout else None
        self.legs = [(d, J.FK_CODE[c["fks"][i][0][0].dtype.str[1:]], c["hows"][i], c["kouts"][i])
                     for i, d in enumerate(self.dev)]

    def check(self, J, in_place: bool) -> int:
        c = self.c
        src = torch.from_numpy(c["src"].view(np.int64).copy()).cuda()
        dst = src if in_place else torch.full_like(src, 0x1234)
        cnt = torch.full((1,), 5, dtype=torch.int64, device="cuda")
        for k in self.kbuf:
            k.fill_(G.PREFILL)
        J.probe_star(self.legs, self.tab, self.nwords, src, dst, cnt, key_out=self.ktab)
        torch.cuda.synchronize()
        pre = [[np.full(n, G.PREFILL, np.int32) for n in self.rows] for _ in range(self.nout)]
        want, codes = J.host_probe_star(list(zip(self.host, c["hows"], c["kouts"])), c["fks"],
                                        c["src"], pre if self.nout else None)
        label = (c["label"], in_place)
        assert np.array_equal(dst.cpu().numpy().view(np.uint64), want), label
        assert int(cnt.item()) == 5 + _popcount(want), label
        if not in_place:
            assert np.array_equal(src.cpu().numpy().view(np.uint64), c["src"]), label
        for j in range(self.nout):
            # the whole buffer: the codes on the destination rows, the prefill on
            # every other element, the words behind each batch's rows included
            whole = np.full(self.nwords * 64, G.PREFILL, np.int32)
            for b, n in enumerate(self.rows):
                whole[int(self.word_base[b]) * 64:int(self.word_base[b]) * 64 + n] = codes[j][b]
            assert np.array_equal(self.kbuf[j].cpu().numpy(), whole), label + (j,)
            dest = np.concatenate([G.unpack(want, int(wb), n)
                                   for wb, n in zip(self.word_base, self.rows)])
            flat = np.concatenate(codes[j])
            assert (flat[~dest] == G.PREFILL).all(), label
        return _popcount(want)


@pytest.fixture(scope="module")
def built(S):
    return {}


@pytest.mark.parametrize("nlegs", [1, 2, 3, 4])
def test_star_kernel_equals_twin(S, built, nlegs):
    """Batches of 1, 63, 64, 65 and 200 rows in one launch; storage types
    cycling through all eight; validity on some legs and batches; the tables
    of joingen.key_sets() mixed across legs; dense, every-other-word-zero and
    single-bit sources with garbage beyond the rows; all semi, all anti,
    mixed; code output on all, some and no semi legs; in place and not."""
    from nvme_strom_amd.ops import coljoin as J
    cases = [c for c in G.star_cases() if len(c["keys"]) == nlegs]
    assert len(cases) >= 18
    kept = 0
    for c in cases:
        run = _Launch(J, c, built)
        for in_place in (False, True):
            kept += run.check(J, in_place)
    assert kept > 0


def test_star_kernel_coverage():
    cases = G.star_cases()
    assert {t for c in cases for t in c["tables"]} == {"0", "1", "2", "37", "5000", "chain", "wrap"}
    assert {v.dtype.str[1:] for c in cases for leg in c["fks"] for v, _ in leg} == set(G.DTYPES)
    some = [[ok is not None for leg in c["fks"] for _, ok in leg] for c in cases]
    assert any(any(s) and not all(s) for s in some)


def test_one_leg_equals_column_join(S, built):
    """One leg through the star entry: what strom_column_join gives."""
    from nvme_strom_amd.ops import coljoin as J
    for seed, (table, how) in enumerate([("5000", "semi"), ("chain", "semi"), ("wrap", "anti"),
                                         ("1", "semi"), ("37", "anti")]):
        for type0 in (0, 4, 5):                  # i8, u8, u4
            c = G.star_case(1, 50 + seed, tables=[table], hows=[how],
                            kouts=[0 if how == "semi" else -1], type0=type0)
            c["label"] = f"one-{table}-{how}-{type0}"
            run = _Launch(J, c, built)
            for in_place in (False, True):
                got = []
                for star in (False, True):
                    src = torch.from_numpy(c["src"].view(np.int64).copy()).cuda()
                    dst = src if in_place else torch.full_like(src, 0x1234)
                    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
                    for k in run.kbuf:
                        k.fill_(G.PREFILL)
                    if star:
                        J.probe_star(run.legs, run.tab, run.nwords, src, dst, cnt,
                                     key_out=run.ktab)
                    else:
                        J.probe(run.dev[0], run.legs[0][1], run.tab[0], run.nwords, src, dst, cnt,
                                how=J.HOW[how], key_out=run.ktab[0] if how == "semi" else None)
                    torch.cuda.synchronize()
                    got.append((dst.cpu().numpy(), int(cnt.item()),
                                [k.cpu().numpy() for k in run.kbuf]))
                assert np.array_equal(got[0][0], got[1][0]) and got[0][1] == got[1][1], c["label"]
                for a, b in zip(got[0][2], got[1][2]):
                    assert np.array_equal(a, b), c["label"]


def test_star_entry_refusals(S, built):
    """-EINVAL straight through the library's entry point."""
    from nvme_strom_amd._native import JoinLegs
    from nvme_strom_amd.ops import coljoin as J
    from nvme_strom_amd.ops._util import lib
    c = G.star_case(2, 3, tables=["37", "2"], hows=["semi", "anti"], kouts=[0, -1])
    c["label"] = "refusals"
    run = _Launch(J, c, built)
    src = torch.zeros(run.nwords, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")

    def legs(n=2, **over):
        a = JoinLegs()
        a.nlegs = n
        for i in range(min(n, 4)):
            d, code, how, kout = run.legs[i % 2]
            a.leg[i].table, a.leg[i].capacity = d.words.data_ptr(), d.capacity
            a.leg[i].type, a.leg[i].how, a.leg[i].kout = code, J.HOW[how], kout
        for k, v in over.items():
            setattr(a.leg[1], k, v)
        return a

    def call(a, fk=None, kout=None, s=None, d=None):
        tabs = run.tab if a.nlegs <= 2 else run.tab.repeat(2, 1, 1).contiguous()
        return lib().strom_column_join_star(
            a, tabs.data_ptr() if fk is None else fk, len(run.rows), run.nwords,
            src.data_ptr() if s is None else s, src.data_ptr() if d is None else d,
            run.ktab.data_ptr() if kout is None else kout, cnt.data_ptr(), 0)

    assert call(legs()) == 0
    assert call(legs(0)) == -22 and call(legs(5)) == -22
    assert call(legs(table=run.dev[1].words.data_ptr() + 8)) == -22       # alignment
    assert call(legs(table=0)) == -22
    assert call(legs(capacity=0)) == -22 and call(legs(capacity=96)) == -22
    assert call(legs(capacity=32)) == -22
    for code in (0, 3, 4, 11, 12, 13, 14):          # none, floats, bool, strings, decimal
        assert call(legs(type=code)) == -22
    assert call(legs(how=2)) == -22
    assert call(legs(kout=1)) == -22                 # a code table on the anti leg
    assert call(legs(how=0, kout=0)) == -22          # one table, two legs
    assert call(legs(how=0, kout=4)) == -22 and call(legs(how=0, kout=-2)) == -22
    assert call(legs(), kout=0) == -22               # kout without tables
    assert call(legs(), s=src.data_ptr() + 4) == -22 and call(legs(), d=src.data_ptr() + 4) == -22
    a4 = legs(4)
    a4.leg[2].kout, a4.leg[3].kout = -1, -1
    assert call(a4) == 0
    torch.cuda.synchronize()
    # the wrapper refuses the same before the library sees it
    with pytest.raises(ValueError):
        J.probe_star([(run.dev[0], 2, J.ANTI, 0)], run.tab[:1], run.nwords, src, src, cnt,
                     key_out=run.ktab)
    with pytest.raises(NotImplementedError):
        J.probe_star([(run.dev[0], 3, J.SEMI, -1)], run.tab[:1], run.nwords, src, src, cnt)
    with pytest.raises(ValueError):
        J.probe_star([(run.dev[0], 2, J.SEMI, -1)] * 5, run.tab.repeat(3, 1, 1)[:5].contiguous(),
                     run.nwords, src, src, cnt)


# ------------------------------------------------------------ whole scans
@pytest.fixture(scope="module")
def star(S, tmp_path_factory):
    from arrowgen import write
    from nvme_strom_amd.models.arrow_scan import JoinTable
    tbl = G.table()
    d = tmp_path_factory.mktemp("stargpu")
    paths = {}
    for codec in (None, "lz4", "zstd"):
        paths[codec] = str(d / f"star_{codec}.arrow")
        write(paths[codec], tbl, codec, batch_rows=1000)
    dims = G.dimensions(tbl)
    jt = {fk: JoinTable(keys, attrs=attrs, device="cuda") for fk, (keys, attrs) in dims.items()}
    yield tbl, paths, dims, jt
    for t in jt.values():
        t.close()


def quals_and_mask():
    import pyarrow.compute as pc
    from nvme_strom_amd.ops.colpred import P
    return [([], lambda t: t),
            ([P("x") > 0.3], lambda t: t.filter(pc.greater(t.column("x"), 0.3)))]


MIXES = [(("f64", "semi"), ("f32", "anti")),
         (("f32", "semi"), ("f16", "semi"), ("f8", "anti")),
         (("f8", "semi"), ("f64", "anti"), ("f16", "anti"), ("f32", "semi")),
         (("f64", "semi"), ("f32", "semi"), ("f16", "semi"), ("f8", "semi"))]


def _scan(path):
    from nvme_strom_amd.models.arrow_scan import ArrowScan
    return ArrowScan(path, "cuda", chunk_sz=64 << 10, slot_bytes=1 << 20)


def same_agg(a, b):
    assert a.keys == b.keys and a.selected == b.selected and a.rows == b.rows
    assert np.array_equal(a.count_all, b.count_all)
    for x, y, ox, oy in zip(a.values, b.values, a.valid, b.valid):
        assert np.array_equal(ox, oy) and np.array_equal(x[ox], y[oy])


@pytest.mark.parametrize("codec", [None, "lz4", "zstd"])
def test_scan_where_star(S, star, codec):
    """Semi and anti mixes of 2, 3 and 4 legs with and without qualifiers; an
    attribute of the third leg projected; an empty JoinTable as a leg."""
    from nvme_strom_amd.models.arrow_scan import Join, JoinTable, StarJoin
    tbl, paths, dims, jt = star
    sc = _scan(paths[codec])
    try:
        for legs in MIXES:
            sj = StarJoin(*[Join(fk, jt[fk], how) for fk, how in legs])
            for q, mf in quals_and_mask():
                want = G.ids(mf(G.reference(tbl, dims, legs)))
                assert 0 < len(want) < tbl.num_rows, legs
                out = sc.scan_where(q, join=sj)
                assert out.selected == len(want) and out.rows == tbl.num_rows
                assert np.array_equal(out.indices.cpu().numpy(), want), (legs, bool(q))
                assert np.array_equal(sc.host_scan_where(q, join=sj).indices, want)
        legs = (("f32", "anti"), ("f8", "semi"), ("f16", "semi"))
        sj = StarJoin(*[Join(fk, jt[fk], how) for fk, how in legs])
        for q, mf in quals_and_mask():
            ref = mf(G.reference(tbl, dims, legs, [("f16", "cat", "c_cat")]))
            out = sc.scan_where(q, project=jt["f16"]["cat"], join=sj)
            assert np.array_equal(out.indices.cpu().numpy(), G.ids(ref))
            codes = out.values.cpu().numpy()
            assert codes.dtype == np.int32 and out.valid is None
            assert [out.dictionary[c] for c in codes.tolist()] == ref.column("c_cat").to_pylist()
            h = sc.host_scan_where(q, project=jt["f16"]["cat"], join=sj)
            assert np.array_equal(h.values, codes) and h.dictionary == out.dictionary
        out = sc.scan_where([], project="k16", join=sj)
        ref = G.reference(tbl, dims, legs)
        assert np.array_equal(out.values.cpu().numpy(),
                              np.asarray(ref.column("k16").combine_chunks()))
        # an empty JoinTable: semi selects nothing, anti changes nothing
        empty = JoinTable(np.zeros(0, np.int64), attrs={"c": []}, device="cuda")
        base = [Join("f64", jt["f64"]), Join("f16", jt["f16"], "anti")]
        want = sc.scan_where([], join=StarJoin(*base)).indices.cpu().numpy()
        out = sc.scan_where([], join=StarJoin(base[0], Join("f32", empty, "anti"), base[1]))
        assert len(want) and np.array_equal(out.indices.cpu().numpy(), want)
        assert sc.scan_where([], join=StarJoin(base[0], Join("f32", empty), base[1])).selected == 0
        out = sc.scan_where([], project=empty["c"],
                            join=StarJoin(base[0], base[1], Join("f8", empty)))
        assert out.selected == 0 and out.values.numel() == 0
        empty.close()
        # one leg: what join=Join gives
        a = sc.scan_where([], project=jt["f64"]["reg"], join=StarJoin(base[0]))
        b = sc.scan_where([], project=jt["f64"]["reg"], join=base[0])
        assert torch.equal(a.indices, b.indices) and torch.equal(a.values, b.values)
    finally:
        sc.close()


@pytest.mark.parametrize("codec", [None, "lz4", "zstd"])
def test_aggregate_and_top_star(S, star, codec):
    """aggregate by an attribute of the second leg, by attributes of two legs
    and a column, and without by; top with an attribute carried; merged batch
    ranges — against pyarrow and the host twins."""
    from nvme_strom_amd.models.arrow_scan import HashBy, Join, StarJoin
    tbl, paths, dims, jt = star
    legs = (("f64", "semi"), ("f32", "semi"), ("f16", "semi"), ("f8", "anti"))
    sj = StarJoin(*[Join(fk, jt[fk], how) for fk, how in legs])
    attrs = [("f64", "cat", "a_cat"), ("f32", "reg", "b_reg"), ("f16", "cat", "c_cat")]
    hb = HashBy([jt["f64"]["cat"], jt["f16"]["cat"], "k16"], groups=1 << 12)
    sc = _scan(paths[codec])
    try:
        for q, mf in quals_and_mask():
            ref = mf(G.reference(tbl, dims, legs, attrs))
            assert ref.num_rows > 50
            out = sc.aggregate(q, G.AGGS, by=jt["f32"]["reg"], join=sj)
            G.check_agg(out, ref, ["b_reg"])
            same_agg(out, sc.host_aggregate(q, G.AGGS, by=jt["f32"]["reg"], join=sj))
            out = sc.aggregate(q, G.AGGS, by=hb, join=sj)
            assert out.by == ("cat[0]", "cat[1]", "k16")
            G.check_agg(out, ref, ["a_cat", "c_cat", "k16"])
            same_agg(out, sc.host_aggregate(q, G.AGGS, by=hb, join=sj))
            out = sc.aggregate(q, G.AGGS, join=sj)
            G.check_agg(out, ref)
            same_agg(out, sc.host_aggregate(q, G.AGGS, join=sj))
            for desc in (False, True):
                out = sc.top(q, "m64", 40, desc, project=jt["f32"]["reg"], join=sj)
                G.check_top(out, ref, "m64", 40, desc, "b_reg")
                h = sc.host_top(q, "m64", 40, desc, project=jt["f32"]["reg"], join=sj)
                assert np.array_equal(out.rows, h.rows)
                assert np.array_equal(out.projected, h.projected)
        # legs permuted: the same groups
        whole = sc.aggregate([], G.AGGS, by=hb, join=sj)
        perm = StarJoin(*[Join(fk, jt[fk], how) for fk, how in (legs[3], legs[2], legs[0],
                                                                 legs[1])])
        same_agg(sc.aggregate([], G.AGGS, by=hb, join=perm), whole)
        # batch ranges merge to the whole
        parts = [sc.aggregate([], G.AGGS, by=hb, join=sj, batches=r)
                 for r in ((0, 2), (2, 2), (2, 6))]
        same_agg(parts[0].merge(parts[1]).merge(parts[2]), whole)
        parts = [sc.aggregate([], G.AGGS, by=jt["f16"]["cat"], join=sj, batches=r)
                 for r in ((0, 3), (3, 6))]
        same_agg(parts[0].merge(parts[1]), sc.aggregate([], G.AGGS, by=jt["f16"]["cat"], join=sj))
        tops = [sc.top([], "m64", 25, True, project=jt["f16"]["cat"], join=sj, batches=r)
                for r in ((0, 4), (4, 6))]
        t = sc.top([], "m64", 25, True, project=jt["f16"]["cat"], join=sj)
        m = tops[0].merge(tops[1])
        assert np.array_equal(m.rows, t.rows) and np.array_equal(m.projected, t.projected)
    finally:
        sc.close()


def test_star_on_a_ring_of_two_slots(S, tmp_path):
    """More groups than ring slots (the ring held at MAX_SLOTS = 2, which
    leaves it at its minimum): every
    slot's bitmap, key buffer and both leg buffers are reused; results equal
    the default ring's and pyarrow's; the bytes read are a plain scan's."""
    from arrowgen import write
    from nvme_strom_amd.models.arrow_scan import ArrowScan, HashBy, Join, JoinTable, StarJoin
    from nvme_strom_amd.ops.colpred import P
    import pyarrow.compute as pc
    rng = np.random.default_rng(31)
    n = 200_000
    tbl = pa.table({"fa": pa.array(rng.integers(0, 10_000, n).astype(np.int32),
                                   mask=rng.random(n) < 0.05),
                    "fb": pa.array(rng.integers(0, 500, n).astype(np.uint16)),
                    "fc": pa.array(rng.integers(-50, 50, n).astype(np.int8)),
                    "m64": pa.array(rng.integers(-10**12, 10**12, n)),
                    "m32": pa.array(rng.integers(-10**6, 10**6, n).astype(np.int32),
                                    mask=rng.random(n) < 0.1),
                    "x": pa.array(rng.random(n))})
    path = str(tmp_path / "ring.arrow")
    write(path, tbl, None, batch_rows=4093)
    ka = rng.choice(20_000, 5000, replace=False).astype(np.int64)
    kb = rng.choice(1000, 300, replace=False).astype(np.int64)
    kc = np.arange(-50, 0, dtype=np.int64)
    ca = [None if k % 97 == 0 else f"c{k % 23}" for k in ka.tolist()]
    cb = [int(k % 5) for k in kb.tolist()]
    da = JoinTable(ka, attrs={"cat": ca}, device="cuda")
    db = JoinTable(kb, attrs={"cat": cb}, device="cuda")
    dc = JoinTable(kc, device="cuda")
    sj = StarJoin(Join("fa", da), Join("fc", dc, "anti"), Join("fb", db))
    hb = HashBy([da["cat"], db["cat"]], groups=1 << 10)
    quals = [P("x") > 0.1]
    left = tbl.append_column("__id", pa.array(np.arange(n, dtype=np.int64)))
    for f in ("fa", "fb", "fc"):
        left = left.set_column(left.column_names.index(f), f, left.column(f).cast(pa.int64()))
    ref = left.join(pa.table({"__k": pa.array(ka), "a_cat": pa.array(ca)}), keys="fa",
                    right_keys="__k", join_type="inner", use_threads=False)
    ref = ref.join(pa.table({"__k": pa.array(kc)}), keys="fc", right_keys="__k",
                   join_type="left anti", use_threads=False)
    ref = ref.join(pa.table({"__k": pa.array(kb), "b_cat": pa.array(cb)}), keys="fb",
                   right_keys="__k", join_type="inner", use_threads=False)
    ref = ref.filter(pc.greater(ref.column("x"), 0.1)).sort_by("__id")
    sc = ArrowScan(path, "cuda", chunk_sz=64 << 10, slot_bytes=1 << 20)
    tight = ArrowScan(path, "cuda", chunk_sz=64 << 10, slot_bytes=1 << 20)
    tight.MAX_SLOTS = 2
    try:
        g = sc.aggregate(quals, G.AGGS, by=hb, join=sj)
        t = tight.aggregate(quals, G.AGGS, by=hb, join=sj)
        assert g.groups > sc.nslots and t.groups > len(tight._slots)
        assert all(len(s.legbuf) == 2 for s in tight._slots)
        G.check_agg(g, ref, ["a_cat", "b_cat"])
        G.check_agg(t, ref, ["a_cat", "b_cat"])
        same_agg(t, g)
        assert len(g.keys) > 100 and any(k[0] is None for k in g.keys)
        out = tight.scan_where(quals, project=db["cat"], join=sj)
        assert np.array_equal(out.indices.cpu().numpy(), G.ids(ref))
        assert [out.dictionary[c] for c in out.values.cpu().tolist()] == \
            ref.column("b_cat").to_pylist()
        top = tight.top(quals, "m64", 30, project=da["cat"], join=sj)
        G.check_top(top, ref, "m64", 30, False, "a_cat")
        # the star scan reads what a scan over the same columns reads
        same = sc.scan_where(quals + [P(c).is_valid() for c in ("fa", "fc", "fb", "m64", "m32")])
        assert g.bytes_read == same.bytes_read and g.groups == same.groups
    finally:
        sc.close()
        tight.close()
        for d in (da, db, dc):
            d.close()
