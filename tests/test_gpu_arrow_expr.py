"""Computed columns of the Arrow scan on the GPU (csrc/kernels/colexpr.hip):
the kernel alone on hand-built batch tables against the numpy twin, word for
word with guarded and prefilled outputs, and whole scans with expressions in
aggregates, qualifiers, HashBy keys, ORDER BY and projections against the host
twins and pyarrow."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")
import pyarrow.compute as pc  # noqa: E402

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))

import exprgen as XG  # noqa: E402
from exprgen import E, Or, P  # noqa: E402
from nvme_strom_amd.ops import colexpr as X  # noqa: E402
from nvme_strom_amd.utils.arrow_ipc import Column  # noqa: E402


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nvme_strom_amd as S
    S.configure(gpu_emulation=0)
    return S


# ------------------------------------------------------------ the kernel alone
_KINDS = {"i1": ("int", 8, True), "i2": ("int", 16, True), "i4": ("int", 32, True),
          "i8": ("int", 64, True), "u1": ("int", 8, False), "u2": ("int", 16, False),
          "u4": ("int", 32, False), "f4": ("float", 32, True), "f8": ("float", 64, True)}
_SCHEMA = [Column(n, *k) for n, k in _KINDS.items()]
I64_MIN, I64_MAX = XG.I64_MIN, XG.I64_MAX


def _dev(a: np.ndarray) -> torch.Tensor:
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


class _Launch:
    """A Case on the device: its sources once, any number of output buffers."""

    def __init__(self, case: XG.Case):
        self.case = case
        self.vals = [_dev(v) for v in case.vals]
        self.vwords = [_dev(w) for w in case.vwords]

    def outputs(self):
        v, k = self.case.out_buffers()
        d_v, d_k = _dev(v), _dev(k)
        src, out = self.case.tables([t.data_ptr() for t in self.vals],
                                    [t.data_ptr() for t in self.vwords], d_v.data_ptr(),
                                    d_k.data_ptr())
        return d_v, d_k, torch.from_numpy(src).cuda(), torch.from_numpy(out).cuda()

    def run(self, prog, sel=None, stream=None):
        d_v, d_k, d_src, d_out = self.outputs()
        d_sel = torch.from_numpy(sel.view(np.int64).copy()).cuda() if sel is not None else None
        X.expr_batched(prog, d_src, self.case.nwords, d_out, d_sel, stream=stream)
        return d_v, d_k, (d_src, d_out, d_sel)

    def check(self, prog, got, sel=None, where=""):
        d_v, d_k = got[0], got[1]
        wv, wk = self.case.expected(prog, X.host_expr, sel)
        k = d_k.cpu().numpy().view(np.uint64)
        v = d_v.cpu().numpy().view(np.uint64)
        assert np.array_equal(k, wk), ("validity words", where)
        bad = np.flatnonzero(v != wv)
        assert not len(bad), ("values", where, bad[:5] - XG.GUARD, v[bad[:5]], wv[bad[:5]])


def _programs():
    """(label, expression): identity and widening of every source type, a
    16-op and a depth-8 program, constants on both sides."""
    out = [(f"identity {c}", E(c)) for c in _KINDS]
    out += [(f"to double {c}", E(c) + 0.0) for c in ("i1", "i8", "u4", "f4")]
    e16 = E("i4")
    for k in range(7):
        e16 = e16 * E("i2") if k % 2 else e16 - E("i8")
    out.append(("16 ops", abs(e16)))
    d8 = E("i1")
    for k in range(7):
        d8 = E("u2") - d8 if k % 2 else E("i4") * d8
    out.append(("depth 8", d8))
    out.append(("constants", 3 - (5 * E("i4") + 2) * -7))
    out.append(("float constants", 0.25 * (E("f8") - 1.5) / (2.0 + E("f4"))))
    out.append(("floor", (E("i8") // 7) % 5 - (E("i4") % (1 << 20)) // 3))
    out.append(("mixed", E("f4") * E("f8") + E("i8") / E("u2")))
    return out


@pytest.mark.parametrize("nulls", ["none", "one", "some"])
def test_kernel_equals_twin(S, nulls):
    """Batches of 1, 63, 64, 65, 127 and 200 rows in one launch; validity
    absent, on one source only, on some batches only; d_sel NULL, all ones,
    sparse and with zero words (their validity 0, their values untouched)."""
    for seed, (label, e) in enumerate(_programs()):
        prog = X.compile_expr(e, _SCHEMA)
        if label == "16 ops":
            assert len(prog.ops) == 16
        if label == "depth 8":
            assert prog.depth == 8
        L = _Launch(XG.case_of(prog.columns, nulls=nulls, seed=seed))
        runs = [(sl, sel, L.run(prog, sel)) for sl, sel in XG.selections(L.case.nwords, seed)]
        torch.cuda.synchronize()
        for sl, sel, got in runs:
            L.check(prog, got, sel, (label, nulls, sl))


def _one_batch(dtype, values):
    v = np.asarray(values, dtype)
    return _Launch(XG.Case([len(v)], [[v]])), v


def _values(L, prog):
    got = L.run(prog)
    torch.cuda.synchronize()
    L.check(prog, got)
    n = int(L.case.rows[0])
    return got[0].cpu().numpy().view(np.uint64)[XG.GUARD:XG.GUARD + n]


def test_integer_wrap_and_floor(S):
    xs = [I64_MAX, I64_MIN, -1, 0, 1, -7, -8, -6, 6, 7, 8, (1 << 40), -(1 << 40), -(1 << 40) - 1,
          (1 << 40) - 1, I64_MIN + 1, I64_MAX - 1]
    L, v = _one_batch("i8", xs)
    col = E("i8")
    i64 = lambda e: _values(L, X.compile_expr(e, _SCHEMA)).view(np.int64)
    assert i64(col + 1)[0] == I64_MIN                       # INT64_MAX + 1
    assert i64(col * -1)[1] == I64_MIN                      # INT64_MIN x -1
    assert i64(-col)[1] == I64_MIN and i64(abs(col))[1] == I64_MIN
    assert i64(-col)[0] == -I64_MAX and i64(abs(col))[2] == 1
    with np.errstate(all="ignore"):
        for c in (7, 1 << 40, 1, I64_MAX):
            assert i64(col // c).tolist() == np.floor_divide(v, np.int64(c)).tolist()
            r = i64(col % c)
            assert r.tolist() == np.remainder(v, np.int64(c)).tolist()
            assert (r >= 0).all() and (r < c).all()
    assert i64(col // 7)[5:8].tolist() == [-1, -2, -1] and i64(col % 7)[5:8].tolist() == [0, 6, 1]
    assert i64(col // (1 << 40))[12:14].tolist() == [-1, -2]


def test_float_specials_and_no_contraction(S):
    sub = 5e-324
    xs = [np.nan, np.inf, -np.inf, -0.0, 0.0, sub, -sub, 1.0, -2.5, 1e308]
    L, v = _one_batch("f8", xs)
    f = lambda e: _values(L, X.compile_expr(e, _SCHEMA))
    col = E("f8")
    assert f(col).tolist() == XG.bits(v).tolist()            # -0.0 and the subnormals kept
    assert f(col * 2.0)[5] == XG.bits([2 * sub])[0] and f(-col)[4] == XG.bits([-0.0])[0]
    assert f(1.0 / col)[3:5].tolist() == XG.bits([-np.inf, np.inf]).tolist()
    assert f(col / col)[[0, 1, 4]].tolist() == [X.NAN_BITS] * 3      # NaN, inf/inf, 0/0
    assert f(col - col)[1] == X.NAN_BITS and f(col * 10.0)[9] == XG.bits([np.inf])[0]
    assert f(abs(col))[[2, 3]].tolist() == XG.bits([np.inf, 0.0]).tolist()
    # int64 values past 2^53: converted with round-to-nearest-even
    big = [(1 << 53) + 1, (1 << 53) + 3, -(1 << 53) - 1, I64_MAX, I64_MIN, (1 << 62) + 255]
    Li, vi = _one_batch("i8", big)
    got = _values(Li, X.compile_expr(E("i8") + 0.0, _SCHEMA))
    assert got.tolist() == XG.bits(vi.astype(np.float64)).tolist()
    assert got[0] == XG.bits([float(1 << 53)])[0] and got[1] == XG.bits([float((1 << 53) + 4)])[0]
    # the contraction probe: separate rounding gives 0.0, a fused a * b + c -2^-60
    a, b = 1 + 2.0 ** -30, 1 - 2.0 ** -30
    rows = [len(x) for x in ([a] * 70, [a] * 3)]
    case = XG.Case(rows, [[np.full(n, a) for n in rows], [np.full(n, b) for n in rows],
                          [np.full(n, -1.0) for n in rows]])
    sch = [Column(n, "float", 64) for n in "abc"]
    prog = X.compile_expr(E("a") * E("b") + E("c"), sch)
    Lc = _Launch(case)
    got = Lc.run(prog)
    torch.cuda.synchronize()
    Lc.check(prog, got)
    out = got[0].cpu().numpy().view(np.float64)[XG.GUARD:XG.GUARD + 70]
    assert (out == 0.0).all() and not np.signbit(out).any()


def test_malformed_program_launches_nothing(S):
    L, _ = _one_batch("i8", np.arange(100))
    good = X.compile_expr(E("i8") + 1, _SCHEMA)
    for ops in ([(X.XOP_ADD, 0, 0)], [(X.XOP_COL, 0, 0), (X.XOP_COL, 0, 0)],
                [(X.XOP_COL, 1, 0)], [(X.XOP_COL, 0, 0), (X.XOP_DIV, 0, 0)],
                [(X.XOP_COL, 0, 0), (X.XOP_MOD, 0, 0)], [(99, 0, 0)],
                [(X.XOP_COL, 0, 0)] * 9 + [(X.XOP_ADD, 0, 0)] * 8):
        bad = X.Program(good.expr, X.INT, good.columns, good.types, ops[:16], 1, good.column)
        d_v, d_k, d_src, d_out = L.outputs()
        with pytest.raises(RuntimeError, match="-22"):
            X.expr_batched(bad, d_src, L.case.nwords, d_out)
        torch.cuda.synchronize()
        pre = np.uint64(XG.PREFILL)
        assert (d_v.cpu().numpy().view(np.uint64) == pre).all()
        assert (d_k.cpu().numpy().view(np.uint64) == pre).all()


def test_two_streams_two_outputs(S):
    """Two launches from the same sources on two streams, each into its own
    buffers: both equal the twin."""
    p1 = X.compile_expr(E("i4") * E("i2") - E("i8") % 1000, _SCHEMA)
    p2 = X.compile_expr(E("i4") / E("i2") + E("i8"), _SCHEMA)
    assert p1.columns == p2.columns
    L = _Launch(XG.case_of(p1.columns, rows=XG.ROWS * 4, nulls="some", seed=9))
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = L.run(p1, stream=s1)
    b = L.run(p2, stream=s2)
    c = L.run(p1, stream=s2)
    torch.cuda.synchronize()
    L.check(p1, a, where="stream 1")
    L.check(p2, b, where="stream 2")
    L.check(p1, c, where="stream 2 again")


# ------------------------------------------------------------ whole scans
N_ROWS, BATCH = 20_000, 1000


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    import arrowgen
    d = tmp_path_factory.mktemp("gexpr")
    out = {}
    for codec in XG.CODECS:
        out[codec] = str(d / f"x_{codec}.arrow")
        arrowgen.write(out[codec], XG.table(N_ROWS, BATCH), codec, batch_rows=BATCH)
    return out


def _twin_array(sc, tbl, e):
    """The numpy twin's values of ``e`` over the table as a pyarrow array,
    equal to the pyarrow reference bit for bit."""
    schema = {c.name: c for c in sc.meta.schema}
    prog = X.compile_expr(e, schema)
    vals, oks = [], []
    for n in prog.columns:
        a = tbl.column(n).combine_chunks()
        oks.append(np.asarray(a.is_valid()) if a.null_count else None)
        vals.append(a.fill_null(0).to_numpy(zero_copy_only=False))
    v, ok = X.host_expr(prog, vals, oks, tbl.num_rows)
    ok = np.ones(tbl.num_rows, bool) if ok is None else ok
    wv, wok = XG.ref_numpy(tbl, e)
    assert np.array_equal(ok, wok) and np.array_equal(XG.bits(v)[ok], wv[ok])
    return pa.array(v, mask=~ok)


def _same_agg(dev, host, float_sums=()):
    """A device AggOut against the host twin's: keys, counts and every exact
    aggregate equal; float sums and means within the sum's rounding."""
    assert dev.keys == host.keys and np.array_equal(dev.count_all, host.count_all)
    assert dev.rows == host.rows and dev.selected == host.selected
    for i, (fn, col) in enumerate(dev.aggs):
        assert np.array_equal(dev.valid[i], host.valid[i]), (fn, col)
        ok = dev.valid[i]
        if (fn, col) in float_sums or (fn == "mean" and ("sum", col) in float_sums):
            assert np.allclose(dev.values[i][ok], host.values[i][ok], rtol=1e-9, atol=0,
                               equal_nan=True), (fn, col)
        else:
            assert np.array_equal(dev.values[i][ok], host.values[i][ok], equal_nan=True), (fn, col)


@pytest.mark.parametrize("codec", XG.CODECS)
def test_aggregates_of_expressions(S, files, codec):
    from nvme_strom_amd.models.arrow_scan import ArrowScan, HashBy, Join, JoinTable
    tbl = XG.table(N_ROWS, BATCH)
    every = np.ones(N_ROWS, bool)
    sc = ArrowScan(files[codec], "cuda")
    try:
        fns = ("count", "sum", "min", "max", "mean")
        for label, e, domain in XG.exprs():
            ref = _twin_array(sc, tbl, e)
            aggs = [(fn, e) for fn in fns]
            out = sc.aggregate([], aggs)
            for fn in fns:
                XG.check_agg(out, fn, e, ref, every, (label, codec))
            _same_agg(out, sc.host_aggregate([], aggs),
                      [("sum", X.name_of(e))] if domain == "float" else [])
        # by name under a qualifier on a stored column
        e = E("price") * (1 - E("disc"))
        ref = _twin_array(sc, tbl, e)
        m = XG.mask_of(tbl, pc.less(tbl.column("qty"), 30))
        aggs = [("sum", e), ("count", e), ("max", e), ("sum", "qty")]
        out = sc.aggregate([P("qty") < 30], aggs, by="i8")
        XG.check_grouped(out, tbl, ["i8"], e, ref, m, ("count", "sum", "max"), codec)
        _same_agg(out, sc.host_aggregate([P("qty") < 30], aggs, by="i8"), [("sum", X.name_of(e))])
        # HashBy(E("ts_ms") // 1000) and a composite key with a declared width
        sec, val = E("ts_ms") // 1000, E("i32") * E("i16") + E("i8")
        aggs = [("sum", val), ("count", val), ("min", val)]
        out = sc.aggregate([], aggs, by=HashBy(sec, 256))
        XG.check_grouped(out, XG.with_column(tbl, "sec", sec), ["sec"], val,
                         _twin_array(sc, tbl, val), every, ("count", "sum", "min"), codec)
        _same_agg(out, sc.host_aggregate([], aggs, by=HashBy(sec, 256)))
        assert len(out.keys) == 60 and len(out.exprs) == 2
        m5 = E("i32") % 5
        hb = HashBy([m5, "i8"], 4096, bits={m5: 4})
        aggs = [("sum", e), ("count", None)]
        out = sc.aggregate([], aggs, by=hb)
        XG.check_grouped(out, XG.with_column(tbl, "m5", m5), ["m5", "i8"], e, ref, every,
                         ("sum",), codec)
        _same_agg(out, sc.host_aggregate([], aggs, by=hb), [("sum", X.name_of(e))])
        # an expression aggregated after a semi-join
        keys, names = XG.join_dim()
        dim = JoinTable(keys, {"g": names}, device="cuda")
        try:
            hit = np.isin(tbl.column("fk").to_numpy(), keys)
            aggs = [("sum", val), ("max", e), ("count", e)]
            out = sc.aggregate([], aggs, join=Join("fk", dim))
            XG.check_agg(out, "sum", val, _twin_array(sc, tbl, val), hit, codec)
            XG.check_agg(out, "max", e, ref, hit, codec)
            XG.check_agg(out, "count", e, ref, hit, codec)
            _same_agg(out, sc.host_aggregate([], aggs, join=Join("fk", dim)))
            assert out.selected == int(hit.sum())
        finally:
            dim.close()
    finally:
        sc.close()


@pytest.mark.parametrize("codec", XG.CODECS)
def test_qualifiers_order_and_projection(S, files, codec):
    from nvme_strom_amd.models.arrow_scan import ArrowScan
    tbl = XG.table(N_ROWS, BATCH)
    sc = ArrowScan(files[codec], "cuda")
    try:
        a, ratio = E("i32") + E("i16"), E("f64") / E("i8")
        ra, rr = _twin_array(sc, tbl, a), _twin_array(sc, tbl, ratio)
        wv, wok = XG.ref_numpy(tbl, ratio)
        cases = [
            ([a < 100], pc.less(ra, 100)),
            ([Or(a * 2 > 1 << 31, P("i8") < -100)],
             pc.or_kleene(pc.greater(XG.reference(tbl, a * 2), 1 << 31),
                          pc.less(tbl.column("i8"), -100))),
            ([a.between(-1000, 1000), P("i8") >= 0, ratio > 0.5],
             pc.and_(pc.and_(pc.and_(pc.greater_equal(ra, -1000), pc.less_equal(ra, 1000)),
                             pc.greater_equal(tbl.column("i8"), 0)), pc.greater(rr, 0.5))),
            ([a.is_null()], pc.is_null(ra)),
            ([a.not_in([0, 1]), a.ranges([(-50, 50), (1000, 2000)])],
             pc.or_(pc.and_(pc.greater_equal(ra, 2), pc.less_equal(ra, 50)),
                    pc.or_(pc.and_(pc.greater_equal(ra, -50), pc.less_equal(ra, -1)),
                           pc.and_(pc.greater_equal(ra, 1000), pc.less_equal(ra, 2000))))),
        ]
        for quals, want in cases:
            m = XG.mask_of(tbl, want)
            out = sc.scan_where(quals, project=ratio)
            host = sc.host_scan_where(quals, project=ratio)
            ids = out.indices.cpu().numpy()
            assert np.array_equal(ids, np.flatnonzero(m)) and np.array_equal(ids, host.indices)
            ok = out.valid.cpu().numpy().astype(bool)
            assert np.array_equal(ok, wok[m]) and out.values.dtype == torch.float64
            assert np.array_equal(XG.bits(out.values.cpu().numpy())[ok], wv[m][ok])
            assert np.array_equal(XG.bits(host.values)[ok], wv[m][ok])
        # an int64 projection without a qualifier on it
        out = sc.scan_where([P("qty") > 40], project=a * 3)
        m = XG.mask_of(tbl, pc.greater(tbl.column("qty"), 40))
        pv, pok = XG.ref_numpy(tbl, a * 3)
        ok = out.valid.cpu().numpy().astype(bool)
        assert np.array_equal(ok, pok[m]) and out.values.dtype == torch.int64
        assert np.array_equal(XG.bits(out.values.cpu().numpy())[ok], pv[m][ok])
        # ORDER BY the expression, ascending and descending (NaN, then nulls, last)
        m = XG.mask_of(tbl, pc.greater(tbl.column("qty"), 5))
        for e, ref in ((ratio, rr), (a, ra)):
            ev, eok = XG.ref_numpy(tbl, e)
            for desc in (False, True):
                for k in (1, 100, 5000):
                    out = sc.top([P("qty") > 5], e, k, desc, project=a)
                    host = sc.host_top([P("qty") > 5], e, k, desc, project=a)
                    want = XG.top_reference(ref, m, desc, k)
                    assert out.rows.tolist() == want.tolist(), (e, desc, k)
                    assert np.array_equal(out._entries, host._entries)
                    ok = np.ones(len(want), bool) if out.valid is None else out.valid
                    assert np.array_equal(ok, eok[want])
                    assert np.array_equal(XG.bits(out.values)[ok], ev[want][ok])
        # few enough rows that k reaches the NaNs and the nulls behind the values
        near = [P("i8").between(-3, 3)]
        out = sc.top(near, ratio, 6000, True)
        assert out.selected < 6000 and np.isnan(out.values).any() and not out.valid.all()
        assert np.array_equal(out._entries, sc.host_top(near, ratio, 6000, True)._entries)
    finally:
        sc.close()


def test_plain_queries_launch_no_expression(S, files, monkeypatch):
    """Without an E the expression stage is never entered."""
    from nvme_strom_amd.models import arrow_scan as M
    calls = []
    monkeypatch.setattr(M, "expr_batched", lambda *a, **k: calls.append(a))
    sc = M.ArrowScan(files["lz4"], "cuda")
    try:
        sc.aggregate([P("qty") < 30], [("sum", "price"), ("sum", "qty")], by="i8")
        sc.scan_where([P("i8") > 0], project="i64")
        sc.top([], "f64", 10)
        assert not calls and all(not s.exprbuf for s in sc._slots)
    finally:
        sc.close()


def test_expressions_on_a_small_ring(S, tmp_path):
    """200,000 rows, more groups than ring slots (the ring held at its
    minimum): each slot's expression
    buffers are allocated once and reused by its later groups."""
    import arrowgen
    from nvme_strom_amd.models.arrow_scan import ArrowScan, HashBy
    n = 200_000
    tbl = XG.table(n, 4093, seed=5)
    path = str(tmp_path / "ring.arrow")
    arrowgen.write(path, tbl, None, batch_rows=4093)
    sc = ArrowScan(path, "cuda", chunk_sz=64 << 10, slot_bytes=1 << 20)
    sc.MAX_SLOTS = 2
    try:
        e, sec = E("price") * (1 - E("disc")), E("ts_ms") // 1000
        val = E("i32") * E("i16") + E("i8")
        quals = [val > 0, P("qty") < 45]
        aggs = [("sum", e), ("sum", val), ("count", val), ("max", e)]
        out = sc.aggregate(quals, aggs, by=HashBy(sec, 256))
        assert out.groups > len(sc._slots) and len(out.exprs) == 3
        assert all(len(s.exprbuf) == 3 and len(s.exprvalid) == 3 for s in sc._slots)
        rv = _twin_array(sc, tbl, val)
        m = XG.mask_of(tbl, pc.and_(pc.greater(rv, 0), pc.less(tbl.column("qty"), 45)))
        t2 = XG.with_column(tbl, "sec", sec)
        XG.check_grouped(out, t2, ["sec"], e, _twin_array(sc, tbl, e), m, ("sum", "max"))
        XG.check_grouped(out, t2, ["sec"], val, rv, m, ("sum", "count"))
        _same_agg(out, sc.host_aggregate(quals, aggs, by=HashBy(sec, 256)),
                  [("sum", X.name_of(e))])
        top = sc.top(quals, e, 50, True)
        assert top.rows.tolist() == XG.top_reference(_twin_array(sc, tbl, e), m, True, 50).tolist()
    finally:
        sc.close()
