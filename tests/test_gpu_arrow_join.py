"""The Arrow scan's hash join on the GPU (csrc/kernels/coljoin.hip): the
build and probe kernels alone on hand-built batch tables against the numpy
twin, bit for bit, and whole scans with ``join=`` against pyarrow's
Table.join (+ group_by) and the host twins."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nvme_strom_amd as S
    S.configure(gpu_emulation=0)
    return S


# ------------------------------------------------------------ kernels alone
ROWS = [1, 63, 64, 65, 200]
PREFILL = -0x5A5A5A5B


def _device_build(J, keys, payload=None):
    dk = torch.from_numpy(np.ascontiguousarray(keys, np.int64)).cuda()
    dp = torch.from_numpy(np.ascontiguousarray(payload, np.int32)).cuda() \
        if payload is not None else None
    t = J.build(dk, dp)
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module")
def tables(S):
    """Per key set of joingen: (keys, codes, device table, its host copy)."""
    from joingen import key_sets
    from nvme_strom_amd.ops import coljoin as J
    out = {}
    for label, keys in key_sets():
        codes = (np.arange(len(keys)) % 11).astype(np.int32)
        d = _device_build(J, keys, codes)
        out[label] = (keys, codes, d, d.to_host())
    return out


def test_device_build_equals_twin(S, tables):
    """Membership, payloads and header of the device build against the
    twin's: the same keys and counts, and a displacement bound no smaller
    than the table's true one (the slots differ with the order of arrival)."""
    from nvme_strom_amd.ops import coljoin as J
    for label, (keys, codes, dev, host) in tables.items():
        twin = J.host_build(keys, codes)
        assert host.capacity == twin.capacity == dev.capacity, label
        assert host.nkeys == twin.nkeys == len(keys) and host.dups == twin.dups == 0, label
        assert host.items() == twin.items(), label
        assert bool(host.words[J.H_HAS_EMPTY]) == bool(twin.words[J.H_HAS_EMPTY]), label
        assert host.maxdisp >= host.true_maxdisp(), label
        assert (host.words[6:8] == 0).all()
        # the device table answers through the twin's walk as well
        m, pay = J.host_lookup(host, keys)
        assert m.all() and np.array_equal(pay, codes), label
    # the one-home chain is as long on the device as in the twin
    assert tables["chain"][3].maxdisp == 199
    # duplicates are counted and not inserted; the build row is the payload
    keys = np.array([5, 9, 5, -(1 << 63), 9, 5, -(1 << 63), 11], np.int64)
    d = _device_build(J, keys).to_host()
    assert d.nkeys == 4 and d.dups == 4 and set(d.items()) == {5, 9, 11, -(1 << 63)}
    assert d.items()[11] == 7 and d.items()[5] in (0, 2, 5)


class _Batches:
    """Hand-built record batches of one fk column on the device."""

    def __init__(self, dtype, keys, rows=ROWS, seed=0, null_p=0.2):
        from joingen import probe_values
        rng = np.random.default_rng(seed)
        self.rows = list(rows)
        words = [(r + 63) // 64 for r in self.rows]
        self.word_base = np.concatenate([[0], np.cumsum(words)[:-1]]).astype(np.int64)
        self.nwords = int(sum(words))
        self.keep, self.host = [], []
        dt = np.dtype(dtype)
        tab = np.zeros((len(self.rows), 5), np.int64)
        self.kbuf = torch.full((self.nwords * 64,), PREFILL, dtype=torch.int32, device="cuda")
        ktab = tab.copy()
        for b, n in enumerate(self.rows):
            v = probe_values(keys, n, seed=seed * 100 + b)
            if dt == np.uint64:
                v = v.view(np.uint64).copy()               # negatives: values >= 2^63
            elif dt != np.int64:
                # keys that fit the type stay keys; the rest wrap to absent values
                info = np.iinfo(dt)
                fit = keys[(keys >= info.min) & (keys <= info.max)]
                v = v.astype(dt)
                if len(fit):
                    hit = rng.random(n) < 0.5
                    v[hit] = rng.choice(fit, int(hit.sum())).astype(dt)
            ok, vptr = None, 0
            if null_p:
                ok = rng.random(n) >= null_p
                bits = np.zeros(((n + 63) // 64) * 64, np.uint8)
                bits[:n] = ok
                dv = torch.from_numpy(np.packbits(bits, bitorder="little").copy()).cuda()
                self.keep.append(dv)
                vptr = dv.data_ptr()
            d = torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).copy()).cuda()
            self.keep.append(d)
            tab[b] = (d.data_ptr(), vptr, n, self.word_base[b], 0)
            ktab[b] = (self.kbuf.data_ptr() + int(self.word_base[b]) * 256, 0, n,
                       self.word_base[b], 0)
            self.host.append((v, ok))
        self.tab = torch.from_numpy(tab).cuda()
        self.ktab = torch.from_numpy(ktab).cuda()

    def bitmap(self, kind, rng):
        """Source words: random bits with garbage beyond each batch's rows,
        "zero" with every other word zero, "single" one bit per word."""
        w = rng.integers(0, 1 << 63, self.nwords, dtype=np.int64).view(np.uint64) * np.uint64(2) + \
            rng.integers(0, 2, self.nwords).astype(np.uint64)
        if kind == "zero":
            w[::2] = 0
        elif kind == "single":
            w = np.uint64(1) << rng.integers(0, 64, self.nwords).astype(np.uint64)
        return w

    def key_out(self):
        out = self.kbuf.cpu().numpy()
        return [out[int(wb) * 64:int(wb) * 64 + n] for wb, n in zip(self.word_base, self.rows)]


def _popcount(words):
    return int(np.unpackbits(np.asarray(words).view(np.uint8)).sum())


def _probe_both(J, dev, host, bt, code, src_words, how, in_place, with_keys):
    src = torch.from_numpy(src_words.view(np.int64).copy()).cuda()
    dst = src if in_place else torch.full_like(src, 0x1234)
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    bt.kbuf.fill_(PREFILL)
    J.probe(dev, code, bt.tab, bt.nwords, src, dst, cnt, how=J.HOW[how],
            key_out=bt.ktab if with_keys else None)
    torch.cuda.synchronize()
    pre = [np.full(n, PREFILL, np.int32) for n in bt.rows]
    want, kout = J.host_probe(host, bt.host, src_words, how, pre if with_keys else None)
    got = dst.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, want), (how, in_place)
    assert int(cnt.item()) == _popcount(want)
    if not in_place:
        assert np.array_equal(src.cpu().numpy().view(np.uint64), src_words)
    if with_keys:
        for g, w in zip(bt.key_out(), kout):
            assert np.array_equal(g, w)
        # the words between the batches' rows and the next batch are untouched
        whole = bt.kbuf.cpu().numpy().reshape(-1, 64)
        for wb, n in zip(bt.word_base, bt.rows):
            tail = whole[int(wb):int(wb) + (n + 63) // 64].reshape(-1)[n:]
            assert (tail == PREFILL).all()
    return want


@pytest.mark.parametrize("label", ["0", "1", "2", "37", "5000", "chain", "wrap"])
def test_probe_every_table(S, tables, label):
    """Each table of the CPU test under an int64 fk with nulls: batches of
    1, 63, 64, 65 and 200 rows in one launch, dense / zero-word / single-bit
    sources, semi and anti, in place and not, with the key output."""
    from nvme_strom_amd.ops import coljoin as J
    keys, codes, dev, host = tables[label]
    bt = _Batches("i8", keys, seed=7)
    rng = np.random.default_rng(11)
    hits = 0
    for kind in ("dense", "zero", "single"):
        src = bt.bitmap(kind, rng)
        for how in ("semi", "anti"):
            for in_place in (False, True):
                w = _probe_both(J, dev, host, bt, J.FK_CODE["i8"], src, how, in_place,
                                with_keys=how == "semi")
                hits += _popcount(w) if (how == "semi" and kind == "dense") else 0
    assert (hits > 0) == (len(keys) > 0)


@pytest.mark.parametrize("dtype", ["i1", "i2", "i4", "i8", "u1", "u2", "u4", "u8"])
def test_probe_every_fk_type(S, dtype):
    """Every supported storage type, widened to int64; uint64 values >= 2^63
    match nothing (the table holds the negative keys with the same bits)."""
    from nvme_strom_amd.ops import coljoin as J
    rng = np.random.default_rng(5)
    keys = np.unique(np.concatenate([
        rng.integers(-128, 256, 90), rng.integers(-2**15, 2**16, 200),
        rng.integers(-2**31, 2**32, 300), rng.integers(-10**15, 10**15, 64),
        np.array([0, -1, -(1 << 63), (1 << 63) - 1], np.int64)]))
    codes = (np.arange(len(keys)) % 13).astype(np.int32)
    dev = _device_build(J, keys, codes)
    host = dev.to_host()
    bt = _Batches(dtype, keys, seed=3, null_p=0.1)
    src = bt.bitmap("dense", rng)
    semi = _probe_both(J, dev, host, bt, J.FK_CODE[dtype], src, "semi", False, True)
    _probe_both(J, dev, host, bt, J.FK_CODE[dtype], src, "anti", True, False)
    assert _popcount(semi) > 0
    if dtype == "u8":
        big = sum(int(((v >= np.uint64(1 << 63)) & np.isin(v.view(np.int64), keys)).sum())
                  for v, _ in bt.host)
        assert big > 0                      # such rows exist, and the twin refused them


def test_probe_refuses_other_types(S, tables):
    from nvme_strom_amd.ops import coljoin as J
    from nvme_strom_amd.ops._util import lib
    keys, codes, dev, host = tables["37"]
    bt = _Batches("i8", keys)
    src = torch.zeros(bt.nwords, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    for code in (0, 3, 4, 11, 12, 13, 14):          # none, floats, bool, strings, decimal
        with pytest.raises(NotImplementedError):
            J.probe(dev, code, bt.tab, bt.nwords, src, src, cnt)
        rc = lib().strom_column_join(code, 0, dev.words.data_ptr(), dev.capacity,
                                     bt.tab.data_ptr(), len(bt.rows), bt.nwords, src.data_ptr(),
                                     src.data_ptr(), 0, cnt.data_ptr(), 0)
        assert rc == -22
    # an anti-join has no key output
    rc = lib().strom_column_join(2, 1, dev.words.data_ptr(), dev.capacity, bt.tab.data_ptr(),
                                 len(bt.rows), bt.nwords, src.data_ptr(), src.data_ptr(),
                                 bt.ktab.data_ptr(), cnt.data_ptr(), 0)
    assert rc == -22


# ------------------------------------------------------------ whole scans
from agggen import AGGS as JOIN_AGGS  # noqa: E402


@pytest.fixture(scope="module")
def fact(tmp_path_factory):
    from arrowgen import table, write
    tbl = table(6000, seed=11)
    d = tmp_path_factory.mktemp("joingpu")
    paths = {}
    for codec in (None, "lz4", "zstd"):
        paths[codec] = str(d / f"j_{codec}.arrow")
        write(paths[codec], tbl, codec, batch_rows=1000)
    return tbl, paths


@pytest.mark.parametrize("codec", [None, "lz4", "zstd"])
def test_scan_where_join(S, fact, codec):
    """Row ids of semi- and anti-joins with and without qualifiers against
    Table.join and the host twin; the projected attribute per row; an empty
    JoinTable."""
    import pyarrow.compute as pc
    from joingen import dimension, joined, joined_ids
    from nvme_strom_amd.models.arrow_scan import ArrowScan, Join, JoinTable
    from nvme_strom_amd.ops.colpred import P
    tbl, paths = fact
    quals = [P("f64") > 0.4]
    mask = lambda t: pc.greater(t.column("f64").combine_chunks(), 0.4)
    sc = ArrowScan(paths[codec], "cuda", chunk_sz=64 << 10, slot_bytes=1 << 20)
    try:
        for fk in ("i64", "u32"):
            keys, cats, regs = dimension(tbl.column(fk).combine_chunks())
            dim = JoinTable(keys, attrs={"category": cats, "region": regs}, device="cuda")
            for how in ("semi", "anti"):
                for q, mf in ((quals, mask), ([], None)):
                    j = Join(fk, dim, how=how)
                    out = sc.scan_where(q, join=j)
                    want = joined_ids(tbl, fk, keys, how, mf)
                    assert 0 < len(want) < tbl.num_rows
                    assert out.selected == len(want) and out.rows == tbl.num_rows
                    assert np.array_equal(out.indices.cpu().numpy(), want), (fk, how, bool(q))
                    assert np.array_equal(sc.host_scan_where(q, join=j).indices, want)
            for attr, vals in (("category", cats), ("region", regs.tolist())):
                out = sc.scan_where(quals, project=dim[attr], join=Join(fk, dim))
                ref = joined(tbl, fk, keys, {attr: vals}, "inner")
                ref = ref.filter(mask(ref).fill_null(False)).sort_by("__id")
                assert np.array_equal(out.indices.cpu().numpy(),
                                      np.asarray(ref.column("__id").combine_chunks()))
                codes = out.values.cpu().numpy()
                assert codes.dtype == np.int32 and out.valid is None
                assert [out.dictionary[c] for c in codes.tolist()] == ref.column(attr).to_pylist()
                h = sc.host_scan_where(quals, project=dim[attr], join=Join(fk, dim))
                assert np.array_equal(h.values, codes) and h.dictionary == out.dictionary
            # a file column projected under a join
            out = sc.scan_where(quals, project="f64", join=Join(fk, dim))
            want = joined_ids(tbl, fk, keys, "semi", mask)
            assert np.array_equal(out.values.cpu().numpy(),
                                  np.asarray(tbl.column("f64").combine_chunks())[want])
            dim.close()
        empty = JoinTable(np.zeros(0, np.int64), attrs={"c": []}, device="cuda")
        assert sc.scan_where([], join=Join("i64", empty)).selected == 0
        assert sc.scan_where(quals, project=empty["c"], join=Join("i64", empty)).selected == 0
        out = sc.scan_where([], join=Join("i64", empty, how="anti"))
        assert np.array_equal(out.indices.cpu().numpy(), np.arange(tbl.num_rows))
        agg = sc.aggregate([], JOIN_AGGS, by=empty["c"], join=Join("i64", empty))
        assert agg.selected == 0 and agg.keys == []
        # without a join nothing changed
        plain = sc.scan_where(quals)
        assert np.array_equal(plain.indices.cpu().numpy(),
                              np.flatnonzero(np.asarray(mask(tbl).fill_null(False))))
    finally:
        sc.close()


@pytest.mark.parametrize("codec", [None, "lz4", "zstd"])
def test_aggregate_join(S, fact, codec):
    """aggregate(by=dim[attr], join=) against pyarrow's inner join plus
    group_by and against host_aggregate; a null attribute value is a None
    group; three batch ranges merge to the whole scan."""
    from agggen import check, qual_lists, same_results
    from joingen import dimension, joined
    from nvme_strom_amd.models.arrow_scan import ArrowScan, Join, JoinTable
    tbl, paths = fact
    sc = ArrowScan(paths[codec], "cuda", chunk_sz=64 << 10, slot_bytes=1 << 20)
    try:
        for fk in ("i64", "u32"):
            keys, cats, regs = dimension(tbl.column(fk).combine_chunks())
            dim = JoinTable(keys, attrs={"category": cats, "region": regs}, device="cuda")
            ref = joined(tbl, fk, keys, {"category": cats, "region": regs.tolist()}, "inner")
            j = Join(fk, dim)
            for label, quals, mask in qual_lists()[:3]:
                for attr in ("category", "region"):
                    out = sc.aggregate(quals, JOIN_AGGS, by=dim[attr], join=j)
                    assert out.rows == tbl.num_rows and out.groups >= 1
                    check(out, ref, mask, attr, JOIN_AGGS)
                    same_results(out, sc.host_aggregate(quals, JOIN_AGGS, by=dim[attr], join=j))
                    if label == "all" and attr == "category":
                        assert None in out.keys
                out = sc.aggregate(quals, JOIN_AGGS, join=j)
                check(out, ref, mask, None, JOIN_AGGS)
            out = sc.aggregate([], JOIN_AGGS, by="b", join=j)
            check(out, ref, None, "b", JOIN_AGGS)
            label, quals, mask = qual_lists()[1]
            parts = [sc.aggregate(quals, JOIN_AGGS, by=dim["category"], join=j, batches=r)
                     for r in ((0, 2), (2, 2), (2, 6))]
            got = parts[0].merge(parts[1]).merge(parts[2])
            check(got, ref, mask, "category", JOIN_AGGS)
            same_results(got, sc.aggregate(quals, JOIN_AGGS, by=dim["category"], join=j))
            with pytest.raises(ValueError, match="merge"):
                parts[0].merge(sc.aggregate(quals, JOIN_AGGS, by=dim["region"], join=j))
            dim.close()
        dim = JoinTable(np.arange(10), attrs={"c": list("abcdefghij")}, device="cuda")
        with pytest.raises(NotImplementedError, match="f64"):
            sc.aggregate([], JOIN_AGGS, join=Join("f64", dim))
        with pytest.raises(NotImplementedError, match="one join"):
            sc.scan_where([], join=[Join("i64", dim)])
        with pytest.raises(ValueError, match="anti"):
            sc.aggregate([], JOIN_AGGS, by=dim["c"], join=Join("i64", dim, how="anti"))
        host_only = JoinTable(np.arange(10))
        with pytest.raises(ValueError, match="scan on"):
            sc.scan_where([], join=Join("i64", host_only))
        with pytest.raises(NotImplementedError, match="i64"):
            sc.aggregate([], [("count", None)], by="i64", join=Join("u32", dim))
    finally:
        sc.close()


def test_join_on_a_ring_of_two_slots(S, tmp_path):
    """More groups than ring slots (the ring held at MAX_SLOTS = 2, which
    leaves it at its minimum): every slot, its bitmap and its key buffer
    are reused; 5,000 dimension keys."""
    from agggen import check, same_results
    from joingen import joined, joined_ids
    from arrowgen import write
    from nvme_strom_amd.models.arrow_scan import ArrowScan, Join, JoinTable
    from nvme_strom_amd.ops.colpred import P
    import pyarrow.compute as pc
    rng = np.random.default_rng(29)
    n = 200_000
    fk = rng.integers(0, 10_000, n).astype(np.int32)
    tbl = pa.table({"fk": pa.array(fk, mask=rng.random(n) < 0.05),
                    "x": pa.array(rng.normal(0, 1e3, n), mask=rng.random(n) < 0.1),
                    "a": pa.array(rng.integers(-10**15, 10**15, n)),
                    "c": pa.array(rng.integers(-10**6, 10**6, n).astype(np.int32))})
    path = str(tmp_path / "ring.arrow")
    write(path, tbl, None, batch_rows=4093)
    keys = rng.choice(20_000, 5000, replace=False).astype(np.int64)
    cats = [None if k % 97 == 0 else f"c{k % 23}" for k in keys.tolist()]
    dim = JoinTable(keys, attrs={"cat": cats}, device="cuda")
    aggs = [("count", None), ("sum", "c"), ("sum", "a"), ("max", "a"), ("sum", "x"), ("min", "x"),
            ("count", "x")]
    quals = [P("c") > -900_000]
    mask = lambda t: pc.greater(t.column("c").combine_chunks(), -900_000)
    sc = ArrowScan(path, "cuda", chunk_sz=64 << 10, slot_bytes=1 << 20)
    tight = ArrowScan(path, "cuda", chunk_sz=64 << 10, slot_bytes=1 << 20)
    tight.MAX_SLOTS = 2
    try:
        j = Join("fk", dim)
        ref = joined(tbl, "fk", keys, {"cat": cats}, "inner")
        g = sc.aggregate(quals, aggs, by=dim["cat"], join=j)
        t = tight.aggregate(quals, aggs, by=dim["cat"], join=j)
        assert g.groups > sc.nslots and t.groups > len(tight._slots)
        check(g, ref, mask, "cat", aggs)
        check(t, ref, mask, "cat", aggs)
        same_results(t, g)
        assert None in g.keys and len(g.keys) == 24
        for how in ("semi", "anti"):
            want = joined_ids(tbl, "fk", keys, how, mask)
            out = tight.scan_where(quals, join=Join("fk", dim, how=how))
            assert np.array_equal(out.indices.cpu().numpy(), want)
        out = tight.scan_where(quals, project=dim["cat"], join=j)
        refs = ref.filter(mask(ref).fill_null(False)).sort_by("__id")
        assert [out.dictionary[c] for c in out.values.cpu().tolist()] == \
            refs.column("cat").to_pylist()
        # the joined scan reads what a scan over the same columns reads
        same = sc.scan_where(quals + [P("fk").is_valid(), P("a").is_valid(), P("x").is_valid()])
        assert g.bytes_read == same.bytes_read and g.groups == same.groups
    finally:
        sc.close()
        tight.close()
        dim.close()
