"""ArrowScan.aggregate on the GPU (csrc/kernels/colagg.hip): whole scans
against pyarrow and the host twin under the comparison rule of
tests/agggen.py, and the kernels alone through ops/colagg.py on hand-built
batch tables against the numpy twin."""
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


# ------------------------------------------------------------ whole scans
@pytest.mark.parametrize("codec", [None, "lz4", "zstd"])
def test_aggregate_query_matrix(S, tmp_path, codec):
    """The CPU file's matrix (qualifier lists x keys, every aggregated
    column kind) through the kernels: 15 full words and a 40-row tail per
    batch."""
    import pyarrow.compute as pc
    from agggen import AGGS, KEYS, check, qual_lists, same_results
    from arrowgen import table, write
    from nvme_strom_amd.models.arrow_scan import ArrowScan
    from nvme_strom_amd.ops.colpred import P
    tbl = table(6000, seed=11)
    path = str(tmp_path / f"a_{codec}.arrow")
    write(path, tbl, codec, batch_rows=1000)
    sc = ArrowScan(path, "cuda", chunk_sz=64 << 10, slot_bytes=1 << 20)
    try:
        for label, quals, ref in qual_lists():
            for key in KEYS:
                out = sc.aggregate(quals, AGGS, by=key)
                assert out.rows == tbl.num_rows and out.groups >= 1
                check(out, tbl, ref, key)
                same_results(out, sc.host_aggregate(quals, AGGS, by=key))
        f32 = [("count", None), ("sum", "f32"), ("mean", "f32")]
        for key in (None, "dict"):
            out = sc.aggregate([], f32, by=key)
            assert np.isnan(out.get("sum", "f32")[0]).all()
            out = sc.aggregate([P("f32") <= 1e30], f32, by=key)
            check(out, tbl, lambda t: pc.less_equal(t.column("f32").combine_chunks(), 1e30), key,
                  f32)
            # nothing selected: no groups; without a key one row of nulls
            out = sc.aggregate([P("i64") > 10**13], AGGS, by=key)
            assert out.selected == 0
            check(out, tbl, lambda t: pc.greater(t.column("i64").combine_chunks(), 10**13), key)
        quals = [P("f64") > 0.4]
        parts = [sc.aggregate(quals, AGGS, by="idict", batches=r) for r in ((0, 2), (2, 2), (2, 6))]
        got = parts[0].merge(parts[1]).merge(parts[2])
        check(got, tbl, qual_lists()[1][2], "idict")
        same_results(got, sc.aggregate(quals, AGGS, by="idict"))
        with pytest.raises(NotImplementedError, match="dec"):
            sc.aggregate([], [("sum", "dec")])
        with pytest.raises(NotImplementedError, match="i64"):
            sc.aggregate([], [("count", None)], by="i64")
        assert sc.aggregate([], [("count", None)]).count_all.tolist() == [6000]
    finally:
        sc.close()


def _big_table(n=200_000, seed=23):
    """int64, float64 with nulls, float32, int32 and an int8-index dictionary
    key of 5 entries with nulls; entry 3 only has null x, entry 4 only NaN f."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 5, n).astype(np.int8)
    knull = rng.random(n) < 0.04
    a = rng.integers(-10**15, 10**15, n)
    x = rng.normal(0, 1e3, n)
    xnull = (rng.random(n) < 0.1) | (k == 3)
    f = rng.normal(0, 5, n).astype(np.float32)
    f[k == 4] = np.nan
    c = rng.integers(-10**6, 10**6, n).astype(np.int32)
    key = pa.DictionaryArray.from_arrays(pa.array(k, mask=knull),
                                         pa.array(["ash", "birch", "cedar", "elm", "fir"]))
    return pa.table({"a": pa.array(a), "x": pa.array(x, mask=xnull), "f": pa.array(f),
                     "c": pa.array(c), "k": key})


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    from arrowgen import write
    tbl = _big_table()
    path = str(tmp_path_factory.mktemp("aggbig") / "big.arrow")
    write(path, tbl, None, batch_rows=4093)
    return path, tbl


BIG_AGGS = [("count", None), ("sum", "a"), ("min", "a"), ("max", "a"), ("sum", "x"), ("min", "x"),
            ("max", "x"), ("count", "x"), ("mean", "x"), ("min", "f"), ("max", "f"),
            ("count", "f"), ("sum", "c"), ("max", "c")]


def test_more_groups_than_slots(S, big):
    """More scan groups than ring slots: the accumulator block persists
    across groups and reused slots; a group with only null x has null sum /
    min / max, one with only NaN f has NaN min / max."""
    import pyarrow.compute as pc
    from agggen import check, same_results
    from nvme_strom_amd.models.arrow_scan import ArrowScan
    from nvme_strom_amd.ops.colpred import P
    path, tbl = big
    sc = ArrowScan(path, "cuda", chunk_sz=64 << 10, slot_bytes=1 << 20)
    tight = ArrowScan(path, "cuda", chunk_sz=64 << 10, slot_bytes=1 << 20)
    tight.MAX_SLOTS = 2                    # the ring at its minimum: every slot reused
    try:
        quals = [P("c") > -900_000]
        ref = lambda t: pc.greater(t.column("c").combine_chunks(), -900_000)
        g = sc.aggregate(quals, BIG_AGGS, by="k")
        assert g.groups > sc.nslots
        check(g, tbl, ref, "k", BIG_AGGS)
        assert g.keys == ["ash", "birch", "cedar", "elm", "fir", None]
        i = g.keys.index("elm")
        assert g.count_all[i] > 0 and g.get("count", "x")[0][i] == 0
        assert not any(g.get(fn, "x")[1][i] for fn in ("sum", "min", "max", "mean"))
        i = g.keys.index("fir")
        assert g.get("min", "f")[1][i] and np.isnan(g.get("min", "f")[0][i]) and \
            np.isnan(g.get("max", "f")[0][i])
        t = tight.aggregate(quals, BIG_AGGS, by="k")
        assert t.groups > len(tight._slots)
        check(t, tbl, ref, "k", BIG_AGGS)
        same_results(t, g)
        for q, r in ((quals, ref), ([], None)):
            u = sc.aggregate(q, BIG_AGGS)
            check(u, tbl, r, None, BIG_AGGS)
            check(tight.aggregate(q, BIG_AGGS), tbl, r, None, BIG_AGGS)
        # reproducibility: the unkeyed float sum of one scan geometry, bit for bit
        s1 = sc.aggregate(quals, [("sum", "x")]).get("sum", "x")[0]
        s2 = sc.aggregate(quals, [("sum", "x")]).get("sum", "x")[0]
        assert np.array_equal(s1.view(np.uint64), s2.view(np.uint64))
        # single pass: four aggregated columns and a key cost the bytes of one
        # scan over the same five columns
        one = sc.aggregate([P("c") > 0], [("sum", "a"), ("min", "x"), ("max", "f"), ("sum", "c")],
                           by="k")
        same = sc.scan_where([P("c") > 0, P("a").is_valid(), P("x").is_valid(),
                              P("f").is_valid(), P("k").is_valid()])
        assert one.bytes_read == same.bytes_read and one.groups == same.groups
        assert one.column_bytes == same.column_bytes
    finally:
        sc.close()
        tight.close()


def test_bad_dictionary_index_raises(S, tmp_path):
    """A key index past the dictionary is malformed data: the scan raises
    and names the key column."""
    import pyarrow.ipc as ipc
    from nvme_strom_amd.models.arrow_scan import ArrowScan
    idx = np.array([0, 1, 2, 1] * 500, np.int8)        # the engine reads files >= 4 KiB
    ok = pa.DictionaryArray.from_arrays(pa.array(idx), pa.array(["p", "q", "r"]))
    tbl = pa.table({"k": ok, "v": pa.array(np.arange(2000))})
    path = str(tmp_path / "bad.arrow")
    with ipc.new_file(path, tbl.schema) as w:
        w.write_table(tbl)
    sc = ArrowScan(path, "cuda")
    try:
        assert sc.aggregate([], [("sum", "v")], by="k").get("sum", "v")[0].sum() == 1999 * 1000
        # corrupt two indices in the file's data buffer
        off = int(sc.meta.columns[sc.meta.column_index("k")].d_off[0])
        with open(path, "r+b") as f:
            f.seek(off + 5)
            f.write(bytes([7, 0xFF]))
            f.flush()
            os.fsync(f.fileno())
    finally:
        sc.close()
    sc = ArrowScan(path, "cuda")
    try:
        with pytest.raises(RuntimeError, match="key column k: 2 "):
            sc.aggregate([], [("sum", "v")], by="k")
        with pytest.raises(RuntimeError, match="key column k: 2 "):
            sc.host_aggregate([], [("sum", "v")], by="k")
    finally:
        sc.close()


# ------------------------------------------------------------ kernels alone
class _Cols:
    """Hand-built record batches on the device: per column a (nbatches, 5)
    strom_filter_batch table over the same batches, and the host arrays."""

    def __init__(self, rows, seed=0):
        self.rows = list(rows)
        self.rng = np.random.default_rng(seed)
        words = [(r + 63) // 64 for r in self.rows]
        self.word_base = np.concatenate([[0], np.cumsum(words)[:-1]]).astype(np.int64)
        self.nwords = int(sum(words))
        self.keep = []

    def column(self, make, null_p=0.0, all_null=False):
        """(host [(values, valid or None)], device table)."""
        host, tab = [], np.zeros((len(self.rows), 5), np.int64)
        for b, n in enumerate(self.rows):
            v = make(n)
            ok = None
            vptr = 0
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
            host.append((v, ok))
        t = torch.from_numpy(tab).cuda()
        self.keep.append(t)
        return host, t

    def bitmap(self, p, garbage=True):
        """(host bool per batch, device words): bits beyond a batch's rows
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
        d = torch.from_numpy(words.view(np.int64)).cuda()
        self.keep.append(d)
        return host, d


def _run(A, lay, cols, sel_h, sel_d, entries, key=None, guard=0):
    """Every entry through the kernels and through the twin: (device block
    on the host, twin block, the whole device allocation)."""
    block = A.alloc_block(lay, "cuda", guard=guard)
    if guard:
        block._whole[:guard] = 0x5A5A5A5A5A5A5A5A
        block._whole[-guard:] = 0x5A5A5A5A5A5A5A5A
    twin = A.new_block(lay)
    for e, col in enumerate(entries):
        host, tab = col
        A.agg_batched(lay, e, block, sel_d, cols.nwords, tab, key[1] if key else None,
                      count_bad=e == 0)
        for b in range(len(cols.rows)):
            v, ok = host[b]
            A.host_agg(lay, twin, e, sel_h[b], v, ok,
                       (key[0][b][0], key[0][b][1]) if key else None, count_bad=e == 0)
    torch.cuda.synchronize()
    return A.block_to_host(block), twin, block._whole.cpu().numpy()


def _equal_blocks(A, lay, got, want):
    assert int(got[0]) == int(want[0])
    for e in range(len(lay.entries)):
        g, w = A.entry_arrays(lay, got, e), A.entry_arrays(lay, want, e)
        for name in w:
            assert np.array_equal(g[name], w[name], equal_nan=w[name].dtype.kind == "f"), \
                (e, name, g[name], w[name])


# small integers as floats: their sums are exact in any order, so the device
# and the twin agree bit for bit
_MAKERS = {
    "i8": lambda r: (lambda n: r.integers(-2**63, 2**63 - 1, n, dtype=np.int64)),
    "u8": lambda r: (lambda n: r.integers(0, 2**64 - 1, n, dtype=np.uint64)),
    "i4": lambda r: (lambda n: r.integers(-2**31, 2**31 - 1, n).astype(np.int32)),
    "u2": lambda r: (lambda n: r.integers(0, 2**16, n).astype(np.uint16)),
    "i1": lambda r: (lambda n: r.integers(-128, 128, n).astype(np.int8)),
    "f8": lambda r: (lambda n: np.where(r.random(n) < 0.1, np.nan,
                                        r.integers(-1000, 1000, n).astype(np.float64))),
    "f4": lambda r: (lambda n: np.where(r.random(n) < 0.1, np.nan,
                                        r.integers(-1000, 1000, n)).astype(np.float32)),
}


@pytest.mark.parametrize("keyed", [False, True])
def test_kernel_batch_shapes(S, keyed):
    """Batches of 1, 63, 64, 65 and 129 rows in one launch, every value
    type, nulls, NaNs; without a key and with a 5-entry key with nulls."""
    from nvme_strom_amd.ops import colagg as A
    cols = _Cols([1, 63, 64, 65, 129], seed=3)
    r = cols.rng
    ents = [A.Entry(A.COUNT | A.ALL)] + [A.Entry(15, dt, dt) for dt in _MAKERS] + \
        [A.Entry(A.COUNT, None, "validity only")]
    data = [cols.column(lambda n: np.zeros(n, np.int8))] + \
        [cols.column(_MAKERS[dt](r), null_p=0.2) for dt in _MAKERS] + \
        [cols.column(lambda n: np.zeros(n, np.int32), null_p=0.5)]
    key = None
    if keyed:
        key = cols.column(lambda n: r.integers(0, 5, n).astype(np.int32), null_p=0.1)
    lay = A.Layout(ents, 6 if keyed else 1, 1 if keyed else 0)
    for p in (1.0, 0.5, 0.0):
        sel_h, sel_d = cols.bitmap(p)
        got, want, _ = _run(A, lay, cols, sel_h, sel_d, data, key)
        _equal_blocks(A, lay, got, want)
        if p == 0.0:
            assert np.array_equal(got, A.new_block(lay))       # an all-zero bitmap


def test_kernel_all_null_column_and_8bit_keys(S):
    """A column whose validity is all zero counts nothing; bool and byte
    keys (3 and 257 slots)."""
    from nvme_strom_amd.ops import colagg as A
    cols = _Cols([300, 7, 128], seed=5)
    r = cols.rng
    data = [cols.column(lambda n: np.zeros(n, np.int8)),
            cols.column(_MAKERS["f8"](r), all_null=True),
            cols.column(_MAKERS["i4"](r), null_p=0.1)]
    ents = [A.Entry(A.COUNT | A.ALL), A.Entry(15, "f8"), A.Entry(15, "i4")]
    sel_h, sel_d = cols.bitmap(0.7)
    lay = A.Layout(ents)
    got, want, _ = _run(A, lay, cols, sel_h, sel_d, data)
    _equal_blocks(A, lay, got, want)
    a = A.entry_arrays(lay, got, 1)
    assert a["count"].tolist() == [0] and a["sum"].tolist() == [0.0]
    # byte key: the twin takes the slots, the kernel reads the bytes
    kb = cols.column(lambda n: r.integers(0, 256, n).astype(np.uint8), null_p=0.05)
    lay = A.Layout(ents, 257, 7)
    got, want, _ = _run(A, lay, cols, sel_h, sel_d, data, kb)
    _equal_blocks(A, lay, got, want)
    # bool key: bit-packed values
    hb, tb = [], np.zeros((len(cols.rows), 5), np.int64)
    for b, n in enumerate(cols.rows):
        bits = r.random(n) < 0.3
        pad = np.zeros(((n + 63) // 64) * 64, np.uint8)
        pad[:n] = bits
        d = torch.from_numpy(np.packbits(pad, bitorder="little").copy()).cuda()
        cols.keep.append(d)
        tb[b] = (d.data_ptr(), 0, n, cols.word_base[b], 0)
        hb.append((bits, None))
    lay = A.Layout(ents, 3, A.COL_BOOL)
    got, want, _ = _run(A, lay, cols, sel_h, sel_d, data, (hb, torch.from_numpy(tb).cuda()))
    _equal_blocks(A, lay, got, want)


@pytest.mark.parametrize("ops,nslots", [(15, 2048), (2, 8192), (3, 4096)])
def test_kernel_one_key_at_the_lds_limit(S, ops, nslots):
    """Every row on one key with as many slots as LDS holds (one replica of
    the accumulators, every lane on the same words), several workgroups."""
    from nvme_strom_amd.ops import colagg as A
    cols = _Cols([200_001, 65, 100_000], seed=9)       # 4,690 words: three workgroups
    r = cols.rng
    data = [cols.column(_MAKERS["f8"](r), null_p=0.05)]
    key = cols.column(lambda n: np.full(n, nslots - 2, np.int32))
    lay = A.Layout([A.Entry(ops, "f8")], nslots, 1)
    assert A.nacc(ops) * nslots * 8 == A.LDS_BYTES
    sel_h, sel_d = cols.bitmap(0.9)
    got, want, _ = _run(A, lay, cols, sel_h, sel_d, data, key)
    _equal_blocks(A, lay, got, want)
    with pytest.raises(NotImplementedError):
        A.Layout([A.Entry(ops, "f8")], nslots + 1, 1)


def test_kernel_bad_keys_touch_nothing(S):
    """Indices -1 and dict_len + 3 among valid ones: counted, and every
    accumulator equals the twin's over the remaining rows; guard words
    around the block stay as they were."""
    from nvme_strom_amd.ops import colagg as A
    cols = _Cols([1000, 129, 64], seed=13)
    r = cols.rng
    nkeys = 9

    def keys(n):
        k = r.integers(0, nkeys, n).astype(np.int32)
        k[r.random(n) < 0.05] = -1
        k[r.random(n) < 0.05] = nkeys + 3
        return k
    data = [cols.column(lambda n: np.zeros(n, np.int8)), cols.column(_MAKERS["i8"](r), null_p=0.1),
            cols.column(_MAKERS["f4"](r))]
    key = cols.column(keys, null_p=0.1)
    ents = [A.Entry(A.COUNT | A.ALL), A.Entry(15, "i8"), A.Entry(15, "f4")]
    lay = A.Layout(ents, nkeys + 1, 1)
    sel_h, sel_d = cols.bitmap(0.8)
    got, want, whole = _run(A, lay, cols, sel_h, sel_d, data, key, guard=8)
    nbad = sum(int((s & (ok if ok is not None else True) & ((k < 0) | (k >= nkeys))).sum())
               for s, (k, ok) in zip(sel_h, key[0]))
    assert nbad > 20 and int(got[0]) == nbad
    _equal_blocks(A, lay, got, want)
    guard = np.int64(0x5A5A5A5A5A5A5A5A)
    assert (whole[:8] == guard).all() and (whole[-8:] == guard).all()
