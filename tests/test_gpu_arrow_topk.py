"""ORDER BY ... LIMIT k of the Arrow scan on the GPU
(csrc/kernels/coltopk.hip): the select and merge kernels alone on hand-built
batch tables against the numpy twin, slabs and state word for word, and
whole scans with ``top`` against the host twin and pyarrow's sort_indices."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))

import topkgen as TG  # noqa: E402


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nvme_strom_amd as S
    S.configure(gpu_emulation=0)
    return S


# ------------------------------------------------------------ kernels alone
GUARD = 16
_PRE = int(np.uint64(TG.PREFILL).view(np.int64))


class _Dev:
    """Hand-built record batches of an order column and an int32 carried
    column on the device; ``codes``: the carried column lives in one int32
    buffer of 64 rows per bitmap word, as the slot's code buffer does."""

    def __init__(self, bl, pay, codes=False):
        self.keep = []
        rows = [len(b[0]) for b in bl]
        words = [(r + 63) // 64 for r in rows]
        wb = np.concatenate([[0], np.cumsum(words)[:-1]]).astype(np.int64)
        self.nwords = int(sum(words))
        tab = np.zeros((len(bl), 5), np.int64)
        ptab = np.zeros((len(bl), 5), np.int64)
        cbuf = torch.zeros(max(self.nwords, 1) * 64, dtype=torch.int32, device="cuda")
        self.keep.append(cbuf)
        for b, ((v, ok, base), (p, pok)) in enumerate(zip(bl, pay)):
            n = rows[b]
            tab[b] = (self._dev(v), self._bits(ok, n), n, wb[b], base)
            if codes:
                cbuf[int(wb[b]) * 64:int(wb[b]) * 64 + n] = torch.from_numpy(p).cuda()
                ptab[b] = (cbuf.data_ptr() + int(wb[b]) * 256, 0, n, wb[b], base)
            else:
                ptab[b] = (self._dev(p), self._bits(pok, n), n, wb[b], base)
        self.tab = torch.from_numpy(tab).cuda()
        self.ptab = torch.from_numpy(ptab).cuda()
        torch.cuda.synchronize()

    def _dev(self, a) -> int:
        a = np.ascontiguousarray(a)
        d = torch.from_numpy(np.concatenate([a.view(np.uint8), np.zeros(1, np.uint8)])).cuda()
        self.keep.append(d)
        return d.data_ptr()

    def _bits(self, ok, n) -> int:
        if ok is None:
            return 0
        bits = np.zeros(max((n + 63) // 64, 1) * 64, np.uint8)
        bits[:n] = ok
        d = torch.from_numpy(np.packbits(bits, bitorder="little").copy()).cuda()
        self.keep.append(d)
        return d.data_ptr()


def _guarded(n: int):
    """(a prefilled int64 device tensor with guards, the n words between)."""
    buf = torch.full((n + 2 * GUARD,), _PRE, dtype=torch.int64, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _check_guards(buf, n: int) -> None:
    h = buf.cpu().numpy()
    assert (h[:GUARD] == _PRE).all() and (h[GUARD + n:] == _PRE).all()


def _device_rounds(T, dev, code, srcs, k, desc, pay=True, streams=None):
    """Select + merge per source bitmap against one device state: (slabs of
    each round, the final state) on the host, every output guarded."""
    sbuf, swords = _guarded(T.state_words(k))
    state = T.init(k, "cuda", words=swords)
    slabs = []
    for src in srcs:
        n = T.grid(len(src), k) * T.slab_words(k)
        buf, words = _guarded(max(n, 1))
        if not n:
            words = words[:0]
        d_src = torch.from_numpy(src.view(np.int64).copy()).cuda()
        out, g = T.select(state, code, dev.tab, len(src), d_src, desc,
                          pay=dev.ptab if pay else None, pay_width=4 if pay else 0,
                          slabs=words if n else None)
        T.merge(state, out, g)
        torch.cuda.synchronize()
        _check_guards(buf, max(n, 1))
        slabs.append(words.cpu().numpy().view(np.uint64).reshape(g, T.slab_words(k)) if n
                     else np.zeros((0, T.slab_words(k)), np.uint64))
    _check_guards(sbuf, T.state_words(k))
    return slabs, state.to_host()


def _twin_rounds(T, bl, pay, srcs, k, desc):
    st = np.full(T.state_words(k), TG.PREFILL, np.uint64)
    st[:T.HDR_WORDS] = T.host_init(k)[:T.HDR_WORDS]
    slabs = []
    for src in srcs:
        out = np.full((T.grid(len(src), k), T.slab_words(k)), TG.PREFILL, np.uint64)
        slabs.append(T.host_select(bl, src, k, desc, st, pay, out=out))
        st = T.host_merge(st, slabs[-1], k)
    return slabs, st


def _same(a, b, label):
    (sa, ta), (sb, tb) = a, b
    for i, (x, y) in enumerate(zip(sa, sb)):
        assert x.shape == y.shape and np.array_equal(x, y), (label, "slabs of round", i)
    assert np.array_equal(ta, tb), (label, "state")


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("dtype", TG.DTYPES)
def test_kernels_equal_twin(S, dtype, desc):
    """Every storage type x direction: random values with the type's ends,
    uint64 >= 2^63, NaN, infinities and both zeros; every key equal; a batch
    sorted the worst way (every row beats the threshold: with k = 3 the
    workgroup sorts and cuts its buffer at every trip) and the best way (the
    threshold prunes); nulls on some batches only; selected bits beyond a
    batch's rows; an empty selection; k above the selected count."""
    from nvme_strom_amd.ops import coltopk as T
    code = T.TYPE_CODE[dtype]
    srcs = [TG.bitmap(TG.ROWS, "random", 1), TG.bitmap(TG.ROWS, "all", 2),
            TG.bitmap(TG.ROWS, "none"), TG.bitmap(TG.ROWS, "percent", 3)]
    for case in ("random", "equal", "worst", "best") + (("zeros",) if dtype[0] == "f" else ()):
        bl, pay = TG.batches(dtype, case, desc, seed=11)
        dev = _Dev(bl, pay)
        for k in TG.KERNEL_KS:
            _same(_device_rounds(T, dev, code, srcs, k, desc),
                  _twin_rounds(T, bl, pay, srcs, k, desc), (case, k))
    # and against plain comparison, not the twin alone
    bl, pay = TG.batches(dtype, "random", desc, seed=12)
    _, st = _device_rounds(T, _Dev(bl, pay), code, srcs[:1], 65, desc)
    rows, _, _, p, pv = T.decode(T.state_entries(st), dtype, desc)
    assert list(zip(rows.tolist(), T.payload_as(p, np.int32).tolist(), pv.astype(int).tolist())) \
        == TG.expected(bl, srcs[0], 65, desc, pay)


@pytest.mark.parametrize("dtype", ["i8", "f4", "u1"])
def test_many_workgroups_and_largest_k(S, dtype):
    """More than one workgroup, a zero-row batch, k up to MAX_K (the buffer
    at its 150 KiB), with and without a carried column."""
    from nvme_strom_amd.ops import coltopk as T
    rows = TG.ROWS + [700, 1000, 0, 130, 3000]
    srcs = [TG.bitmap(rows, "random", 4), TG.bitmap(rows, "all", 5), TG.bitmap(rows, "percent", 6)]
    for case, desc in (("random", False), ("worst", True), ("equal", False)):
        bl, pay = TG.batches(dtype, case, desc, rows=rows, seed=13)
        dev = _Dev(bl, pay)
        for k in (3, 1024, 5000, T.MAX_K):
            assert T.grid(len(srcs[0]), k) > 1
            _same(_device_rounds(T, dev, T.TYPE_CODE[dtype], srcs, k, desc),
                  _twin_rounds(T, bl, pay, srcs, k, desc), (case, k))
        _same(_device_rounds(T, dev, T.TYPE_CODE[dtype], srcs, 7, desc, pay=False),
              _twin_rounds(T, bl, None, srcs, 7, desc), (case, "no payload"))


def test_payload_from_code_buffer(S):
    """The carried column read from an int32 code buffer laid out as the
    slot's (64 rows per bitmap word, no validity)."""
    from nvme_strom_amd.ops import coltopk as T
    bl, pay = TG.batches("i4", "random", True, seed=14)
    pay = [(p, None) for p, _ in pay]
    dev = _Dev(bl, pay, codes=True)
    srcs = [TG.bitmap(TG.ROWS, "random", 7)]
    for k in (2, 64, 1024):
        _same(_device_rounds(T, dev, T.TYPE_CODE["i4"], srcs, k, True),
              _twin_rounds(T, bl, pay, srcs, k, True), k)


def test_two_selects_on_two_streams(S):
    """Two selections on two streams against one state, the first one's merge
    on a third between them: the second reads the threshold before or after
    that merge stored it, and the state equals the twin's either way."""
    from nvme_strom_amd.ops import coltopk as T
    rows = [3000, 200, 65]
    k = 7
    bla, paya = TG.batches("f8", "random", False, rows=rows, seed=15)
    blb, payb = TG.batches("f8", "best", False, rows=rows, seed=16, row_base=10**6)
    da, db = _Dev(bla, paya), _Dev(blb, payb)
    sa, sb = TG.bitmap(rows, "all", 8), TG.bitmap(rows, "random", 9)
    d_sa = torch.from_numpy(sa.view(np.int64).copy()).cuda()
    d_sb = torch.from_numpy(sb.view(np.int64).copy()).cuda()
    s1, s2, s3 = (torch.cuda.Stream() for _ in range(3))
    state = T.init(k, "cuda", stream=s3)
    ready = torch.cuda.Event()
    ready.record(s3)
    s1.wait_event(ready)
    s2.wait_event(ready)
    code = T.TYPE_CODE["f8"]
    oa, ga = T.select(state, code, da.tab, len(sa), d_sa, pay=da.ptab, pay_width=4, stream=s1)
    ea = torch.cuda.Event()
    ea.record(s1)
    ob, gb = T.select(state, code, db.tab, len(sb), d_sb, pay=db.ptab, pay_width=4, stream=s2)
    eb = torch.cuda.Event()
    eb.record(s2)
    s3.wait_event(ea)
    T.merge(state, oa, ga, stream=s3)
    s3.wait_event(eb)
    T.merge(state, ob, gb, stream=s3)
    torch.cuda.synchronize()
    st = T.host_merge(T.host_init(k), T.host_select(bla, sa, k, False, None, paya), k)
    st = T.host_merge(st, T.host_select(blb, sb, k, False, st, payb), k)
    got = state.to_host()
    assert np.array_equal(got, st)
    assert int(got[T.H_MERGES]) == 2 and int(got[T.H_ERRORS]) == 0


def test_wrapper_refuses(S):
    from nvme_strom_amd.ops import coltopk as T
    bl, pay = TG.batches("i4", "random", False, seed=17)
    dev = _Dev(bl, pay)
    src = torch.zeros(dev.nwords, dtype=torch.int64, device="cuda")
    state = T.init(3, "cuda")
    for k in (0, T.MAX_K + 1):
        with pytest.raises(ValueError):
            T.init(k, "cuda")
    with pytest.raises(NotImplementedError):
        T.select(state, 11, dev.tab, dev.nwords, src)                  # bool
    with pytest.raises(ValueError):
        T.select(state, 1, dev.tab, dev.nwords + 1, src)               # bitmap too small
    with pytest.raises(ValueError):
        T.select(state, 1, dev.tab, dev.nwords, src, pay=dev.ptab, pay_width=3)
    with pytest.raises(ValueError):
        T.select(state, 1, dev.tab, dev.nwords, src, pay_width=4)      # a width without a table
    with pytest.raises(ValueError):
        T.select(state, 1, dev.tab, dev.nwords, src,
                 slabs=torch.zeros(2, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        T.merge(state, torch.zeros(2, dtype=torch.int64, device="cuda"), 1)
    torch.cuda.synchronize()


# ------------------------------------------------------------ whole scans
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    import arrowgen
    d = tmp_path_factory.mktemp("topk_gpu")
    out = {}
    for codec in TG.CODECS:
        out[codec] = str(d / f"t_{codec}.arrow")
        arrowgen.write(out[codec], TG.table(), codec, batch_rows=TG.BATCH_ROWS)
    return out


def _scan(path, **kw):
    from nvme_strom_amd.models.arrow_scan import ArrowScan
    return ArrowScan(path, "cuda", chunk_sz=64 << 10, slot_bytes=1 << 20, **kw)


def _same_out(a, b, label=""):
    """Two TopOut are the same result, candidate for candidate."""
    assert np.array_equal(a._entries, b._entries), label
    assert a.rows.tolist() == b.rows.tolist() and a.values.tobytes() == b.values.tobytes(), label
    assert (a.nrows, a.selected) == (b.nrows, b.selected), label
    for x, y in ((a.valid, b.valid), (a.projected, b.projected),
                 (a.projected_valid, b.projected_valid)):
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), label


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("codec", TG.CODECS)
def test_top_query_matrix(S, files, codec, desc):
    """top == host_top == pc.sort_indices(...)[:k]: 9 order columns x
    (no qualifier, an Or) x k in {1, 7, 700, 5000}."""
    tbl = TG.table()
    sc = _scan(files[codec])
    try:
        for label, quals, mask in (TG.qual_lists()[0], TG.qual_lists()[3]):
            ids = TG.selected_ids(tbl, mask)
            for col in TG.ORDER_COLS:
                nulls = tbl.column(col).null_count > 0
                for k in TG.KS:
                    out = sc.top(quals, col, k, desc)
                    TG.check_result(out, tbl, TG.reference(tbl, ids, col, desc, k), col, nulls,
                                    label=(label, col, k))
                    _same_out(out, sc.host_top(quals, col, k, desc), (label, col, k))
                    assert out.selected == len(ids) and out.groups >= 1 and out.bytes_read > 0
    finally:
        sc.close()


def test_top_empty_selection_and_carried_columns(S, files):
    """A qualifier that selects nothing; a range with a fixed-width column
    with nulls and a dictionary-encoded one carried along; refusals."""
    tbl = TG.table()
    sc = _scan(files["lz4"])
    try:
        _, quals, _ = TG.qual_lists()[1]
        out = sc.top(quals, "f32", 7, True, project="i64")
        assert len(out.rows) == 0 and out.selected == 0 and out.nrows == 3000
        assert out.values.dtype == np.float32 and out.projected.dtype == np.int64
        _same_out(out, sc.host_top(quals, "f32", 7, True, project="i64"))
        _, quals, mask = TG.qual_lists()[2]
        ids = TG.selected_ids(tbl, mask)
        for col, proj, pnulls in (("f32", "i64", True), ("ts", "dict", True), ("u32", "i8", True),
                                  ("i64", "f64", False), ("f64", "f64", False)):
            for desc in (False, True):
                out = sc.top(quals, col, 50, desc, project=proj)
                TG.check_result(out, tbl, TG.reference(tbl, ids, col, desc, 50), col,
                                tbl.column(col).null_count > 0, proj, pnulls, (col, proj))
                _same_out(out, sc.host_top(quals, col, 50, desc, project=proj), (col, proj))
        for k in (0, 6145):
            with pytest.raises(ValueError):
                sc.top([], "i64", k)
        for col, kind in (("dec", "decimal"), ("b", "bool"), ("s", "utf8"),
                          ("dict", "dictionary-encoded")):
            with pytest.raises(NotImplementedError, match=kind):
                sc.top([], col, 3)
        with pytest.raises(NotImplementedError, match="utf8"):
            sc.top([], "i64", 3, project="s")
        # the scan object serves other queries afterwards
        assert sc.scan_where([("i64", -5 * 10**11, 5 * 10**11)]).selected == len(ids)
    finally:
        sc.close()


def test_every_slot_reused(S, tmp_path):
    """200,000 rows in batches of 4,093, the ring at two slots: four and five
    groups, so every slot is used again.  The order column ascends in file order and is queried
    descending, so every group replaces the whole state; ascending, the
    first group's threshold prunes every later row."""
    import arrowgen
    n = 200_000
    rng = np.random.default_rng(21)
    v = np.cumsum(rng.integers(1, 5, n)).astype(np.int64)
    tag = rng.integers(-2**31, 2**31, n).astype(np.int32)
    tbl = pa.table({"v": pa.array(v), "tag": pa.array(tag, mask=rng.random(n) < 0.1),
                    "f": pa.array(rng.random(n))})
    path = str(tmp_path / "big.arrow")
    arrowgen.write(path, tbl, None, batch_rows=4093)
    sc = _scan(path, nslots=2)
    sc.MAX_SLOTS = 2                       # the ring at its minimum: every slot reused
    try:
        for k in (100, 1024):
            out = sc.top([], "v", k, True, project="tag")
            assert out.groups == 4 and len(sc._slots) == 2
            assert out.rows.tolist() == list(range(n - 1, n - 1 - k, -1))
            assert np.array_equal(out.values, v[out.rows]) and out.valid is None
            ok = np.asarray(tbl.column("tag").combine_chunks().is_valid())[out.rows]
            assert np.array_equal(out.projected_valid, ok)
            assert np.array_equal(out.projected[ok], tag[out.rows][ok])
            assert out.selected == n
            out = sc.top([], "v", k, False, project="tag")
            assert out.rows.tolist() == list(range(k))
        quals = [("f", 0.25, 0.5)]
        out = sc.top(quals, "v", 100, True, project="tag")
        _same_out(out, sc.host_top(quals, "v", 100, True, project="tag"))
        sel = np.flatnonzero((tbl.column("f").to_numpy() >= 0.25) &
                             (tbl.column("f").to_numpy() <= 0.5))
        assert out.rows.tolist() == sel[::-1][:100].tolist() and out.selected == len(sel)
    finally:
        sc.close()


def test_top_after_semi_join(S, files):
    """join=Join(fk, dim) then ORDER BY: the select runs on the bitmap the
    probe left and carries the attribute's codes from the slot's code buffer."""
    from nvme_strom_amd.models.arrow_scan import Join, JoinTable
    tbl = TG.table()
    keys = np.arange(-40, 40, 3, dtype=np.int64)
    dim = JoinTable(keys, {"name": [f"n{int(x) % 5}" for x in keys]}, device="cuda")
    i8 = tbl.column("i8").combine_chunks()
    hit = np.isin(i8.fill_null(127).to_numpy(zero_copy_only=False), keys) & np.asarray(i8.is_valid())
    sc = _scan(files["zstd"])
    try:
        for desc in (False, True):
            for quals, m in (([], hit), ([("f64", 0.0, 0.5)],
                                         hit & (tbl.column("f64").to_numpy() <= 0.5))):
                ids = np.flatnonzero(m).astype(np.int64)
                out = sc.top(quals, "f32", 100, desc, project=dim["name"], join=Join("i8", dim))
                want = TG.reference(tbl, ids, "f32", desc, 100)
                assert out.rows.tolist() == want.tolist() and out.selected == len(ids)
                fk = i8.take(pa.array(want)).to_pylist()
                assert [out.dictionary[c] for c in out.projected.tolist()] == \
                    [f"n{x % 5}" for x in fk]
                _same_out(out, sc.host_top(quals, "f32", 100, desc, project=dim["name"],
                                           join=Join("i8", dim)))
            out = sc.top([], "i64", 20, desc, join=Join("i8", dim, how="anti"))
            rest = np.flatnonzero(~hit).astype(np.int64)
            assert out.rows.tolist() == TG.reference(tbl, rest, "i64", desc, 20).tolist()
    finally:
        sc.close()
        dim.close()


def test_merged_ranges_and_k_above_selected(S, files):
    """batches= halves merged with TopOut.merge (GPU with GPU, GPU with
    host) equal the whole file's result; k above the selected count returns
    every selected row, sorted."""
    tbl = TG.table()
    sc = _scan(files[None])
    try:
        _, quals, mask = TG.qual_lists()[2]
        ids = TG.selected_ids(tbl, mask)
        for col, desc, k, proj in (("f32", True, 40, "i64"), ("t32", False, 5000, "dict")):
            whole = sc.top(quals, col, k, desc, project=proj)
            a = sc.top(quals, col, k, desc, project=proj, batches=(0, 2))
            b = sc.top(quals, col, k, desc, project=proj, batches=(2, 5))
            hb = sc.host_top(quals, col, k, desc, project=proj, batches=(2, 5))
            for m in (a.merge(b), b.merge(a), a.merge(hb)):
                _same_out(m, whole, (col, k))
            assert len(whole.rows) == min(k, len(ids))
            TG.check_result(whole, tbl, TG.reference(tbl, ids, col, desc, k), col,
                            tbl.column(col).null_count > 0, proj, True, (col, k))
        e = sc.top([], "i64", 5, batches=(3, 3))
        assert e.nrows == 0 and len(e.rows) == 0
    finally:
        sc.close()
