"""ORDER BY on several columns on the GPU (csrc/kernels/colsort.hip): the
encode and radix-pass kernels alone against the numpy twin on every key shape
and size around the tile, the gather and the character copy with sentinels
round every output and planted out-of-range permutation entries, the C
entries' refusals, and whole scans with ``order_by=`` / ``limit=`` /
``offset=`` against the host twin and pyarrow.  Every comparison is exact."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")
import pyarrow.compute as pc  # noqa: E402

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))

import sortgen as SG  # noqa: E402
from sortgen import G  # noqa: E402
from nvme_strom_amd.ops import colsort as SO  # noqa: E402


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nvme_strom_amd as S
    S.configure(gpu_emulation=0)
    return S


def _dev(a) -> "torch.Tensor":
    """The array's bytes on the device (never an empty allocation)."""
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    if not len(b):
        b = np.zeros(16, np.uint8)
    return torch.from_numpy(b.copy()).cuda()


def _dev_order(cols, n):
    """(permutation, radix passes) of the device sort of ``cols`` — (values,
    valid, descending) each, the most significant first."""
    st = SO.State(n, "cuda")
    d = [(SO.type_code(v.dtype), _dev(v[:n]), None if ok is None else _dev(ok[:n].astype(np.uint8)),
          desc) for v, ok, desc in cols]
    npass = SO.order(st, d)
    torch.cuda.synchronize()
    return st.order.cpu().numpy().view(np.uint32).astype(np.int64), npass


# ------------------------------------------------------------ kernels alone
@pytest.mark.parametrize("n", SG.SIZES)
def test_kernel_equals_twin(S, n):
    for label, v, ok in SG.key_cases(n):
        for desc in (False, True):
            cols = [(v, ok, desc)]
            got, npass = _dev_order(cols, n)
            assert np.array_equal(got, SO.host_order(cols, n)), (label, desc)
            assert npass == SO.passes(SO.type_code(v.dtype), ok is not None)
            if label == "equal":
                assert np.array_equal(got, np.arange(n))


def test_scan_kernel_loops(S):
    """More tiles than the scan kernel's workgroup has threads: its loop over
    a row of the table runs more than once, the last trip partly."""
    n = (2 * SO.SCAN_THREADS + 3) * SO.TILE + 5
    rng = np.random.default_rng(5)
    for cols in ([(rng.integers(0, 1 << 16, n).astype("u2"), None, False)],
                 [(SG.random_keys("f4", n, rng), SG.nulls(n, 0.1, rng), True)]):
        got, _ = _dev_order(cols, n)
        assert np.array_equal(got, SO.host_order(cols, n))


@pytest.mark.parametrize("nkeys", [2, 3, 4])
def test_tied_columns(S, nkeys):
    n = 100_003
    cols = SG.tied_columns(nkeys, n)
    got, _ = _dev_order(cols, n)
    assert np.array_equal(got, SO.host_order(cols, n))


GUARD = 64


class _Guarded:
    """A device output of ``nbytes`` between two sentinel runs."""

    def __init__(self, nbytes: int):
        self.nbytes = nbytes
        self.t = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")

    @property
    def ptr(self) -> int:
        return self.t.data_ptr() + GUARD

    def body(self) -> np.ndarray:
        h = self.t.cpu().numpy()
        assert (h[:GUARD] == 0xA5).all() and (h[GUARD + self.nbytes:] == 0xA5).all(), "sentinels"
        return h[GUARD:GUARD + self.nbytes]


@pytest.fixture(scope="module")
def apply_inputs():
    rng = np.random.default_rng(8)
    n = 40_001
    perm = rng.permutation(n).astype(np.uint32)
    bad = rng.choice(n, 37, replace=False)
    perm[bad] = n + rng.integers(0, 5, 37).astype(np.uint32) * 999_983
    perm[bad[:5]] = 0xFFFFFFFF
    cols = {w: rng.integers(0, 256, (n, w)).astype(np.uint8) for w in SO.WIDTHS}
    valid = {w: (rng.random(n) < 0.7).astype(np.uint8) for w in (2, 16)}
    strs = rng.integers(0, 12, n)
    strs[rng.random(n) < 0.01] = 300
    offs = np.concatenate([[0], np.cumsum(strs)]).astype(np.int64)
    chars = rng.integers(1, 256, int(offs[-1])).astype(np.uint8)
    rows = rng.integers(0, 1 << 62, n)
    return n, perm, cols, valid, offs, chars, rows


@pytest.mark.parametrize("window", [(0, None), (0, 0), (12_345, 1000), (40_001 - 10, 50),
                                    (40_001 + 5, 10), (39_000, 2**40)])
def test_apply(S, apply_inputs, window):
    n, perm, cols, valid, offs, chars, rows = apply_inputs
    first, count = window[0], n if window[1] is None else window[1]
    f = min(first, n)
    cnt = min(count, n - f)
    idx = perm[f:f + cnt].astype(np.int64)
    ok = idx < n
    safe = np.where(ok, idx, 0)
    d_perm, d_rows, d_offs, d_chars = _dev(perm), _dev(rows), _dev(offs), _dev(chars)
    d_in = {w: _dev(c) for w, c in cols.items()}
    d_valid = {w: _dev(v) for w, v in valid.items()}
    o_rows = _Guarded(cnt * 8)
    o_cols = {w: _Guarded(cnt * w) for w in cols}
    o_valid = {w: _Guarded(cnt) for w in (1, 2, 16)}       # width 1: no input validity
    o_len = _Guarded((cnt + 1) * 8)
    err = torch.full((1,), 3, dtype=torch.int64, device="cuda")
    specs = [(SO.FIXED, w, d_in[w].data_ptr(), o_cols[w].ptr,
              d_valid[w].data_ptr() if w in d_valid else 0, o_valid[w].ptr if w in o_valid else 0)
             for w in cols]
    specs.append((SO.LEN, 0, d_offs.data_ptr(), o_len.ptr + 8, 0, 0))
    from nvme_strom_amd import _native as N
    rc = N.lib().strom_sort_apply(d_perm.data_ptr(), n, first, count, d_rows.data_ptr(),
                                  o_rows.ptr, SO.sort_cols(specs).ctypes.data, len(specs),
                                  err.data_ptr(), 0)
    assert rc == 0
    torch.cuda.synchronize()
    assert int(err.item()) == 3 + int((~ok).sum())
    assert np.array_equal(o_rows.body().view(np.int64), np.where(ok, rows[safe], 0))
    for w, c in cols.items():
        want = np.where(ok[:, None], c[safe], 0).astype(np.uint8)
        assert np.array_equal(o_cols[w].body().reshape(cnt, w), want), w
    for w in o_valid:
        want = np.where(ok, valid[w][safe] if w in valid else 1, 0)
        assert np.array_equal(o_valid[w].body(), want), w
    lens = np.where(ok, offs[safe + 1] - offs[safe], 0)
    body = o_len.body().view(np.int64)
    if cnt:
        assert np.array_equal(body[1:], lens)
    # the characters behind the lengths' prefix
    out_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    total = int(out_off[-1])
    o_chars = _Guarded(total)
    d_off = _dev(out_off)
    rc = N.lib().strom_sort_chars(d_perm.data_ptr(), n, first, count, d_offs.data_ptr(),
                                  d_chars.data_ptr(), len(chars), d_off.data_ptr(), o_chars.ptr,
                                  total, 0)
    assert rc == 0
    torch.cuda.synchronize()
    src = np.repeat(offs[safe] - out_off[:-1], lens) + np.arange(total)
    assert np.array_equal(o_chars.body(), chars[src])
    if cnt == n:
        assert int((~ok).sum()) == 37 and total > 0


def test_apply_agrees_with_host_apply(S, apply_inputs):
    """The twin's gather on a clean permutation, every kind."""
    n, perm, cols, valid, offs, chars, rows = apply_inputs
    clean = np.random.default_rng(1).permutation(n)
    first, cnt = 100, 5000
    got, gok, _ = SO.host_apply(clean, first, cnt, cols[16], valid[16])
    out, vout = _Guarded(cnt * 16), _Guarded(cnt)
    err = torch.zeros(1, dtype=torch.int64, device="cuda")
    d = [_dev(clean.astype(np.uint32)), _dev(cols[16]), _dev(valid[16])]
    SO.apply(d[0], n, first, cnt, None, None,
             SO.sort_cols([(SO.FIXED, 16, d[1].data_ptr(), out.ptr, d[2].data_ptr(), vout.ptr)]),
             err)
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    assert np.array_equal(out.body().reshape(cnt, 16), got) and np.array_equal(vout.body(), gok)


def test_c_entry_refusals(S):
    from nvme_strom_amd import _native as N
    L = N.lib()
    k = [torch.zeros(8, dtype=torch.int64, device="cuda") for _ in range(2)]
    p = [torch.zeros(8, dtype=torch.int32, device="cuda") for _ in range(2)]
    work = torch.zeros(SO.work_bytes(8) // 4, dtype=torch.int32, device="cuda")
    vals = torch.arange(8, dtype=torch.int64, device="cuda")
    out = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    err = torch.zeros(1, dtype=torch.int64, device="cuda")
    P = lambda t: t.data_ptr()
    I64, big = SO.TYPE_CODE["i8"], 1 << 32
    enc = lambda code=I64, flags=0, v=P(vals), pm=P(p[0]), n=8, key=P(k[0]): \
        L.strom_sort_encode(code, flags, v, 0, pm, n, key, 0)
    assert enc(code=0) == -22 and enc(code=11) == -22 and enc(code=14) == -22 and enc(code=99) == -22
    assert enc(flags=8) == -22 and enc(v=0) == -22 and enc(pm=0) == -22 and enc(key=0) == -22
    assert enc(n=big) == -22 and enc(n=0) == 0
    rp = lambda ki=P(k[0]), pi=P(p[0]), ko=P(k[1]), po=P(p[1]), n=8, shift=0, w=P(work): \
        L.strom_sort_pass(ki, pi, ko, po, n, shift, w, 0)
    assert rp(ki=0) == -22 and rp(pi=0) == -22 and rp(ko=0) == -22 and rp(po=0) == -22
    assert rp(w=0) == -22 and rp(n=big) == -22 and rp(shift=4) == -22 and rp(shift=64) == -22
    assert rp(ko=P(k[0])) == -22 and rp(n=0) == 0
    good = SO.sort_cols([(SO.FIXED, 8, P(vals), P(out), 0, 0)])

    def ap(cols=good, ncols=None, perm=P(p[0]), n=8, rin=0, rout=0, e=P(err)):
        return L.strom_sort_apply(perm, n, 0, 8, rin, rout, cols.ctypes.data if cols is not None
                                  else 0, len(cols) if ncols is None else ncols, e, 0)
    many = np.zeros(17, SO.SORT_COL)
    many[:] = good[0]
    assert ap(cols=many) == -22 and ap(perm=0) == -22 and ap(e=0) == -22 and ap(n=big) == -22
    assert ap(cols=None, ncols=1) == -22 and ap(rin=P(vals)) == -22 and ap(rout=P(out)) == -22
    for width in (0, 3, 5, 32):
        bad = good.copy()
        bad["width"] = width
        assert ap(cols=bad) == -22, width
    for kind in (0, 3):
        bad = good.copy()
        bad["kind"] = kind
        assert ap(cols=bad) == -22, kind
    for fld in ("in", "out"):
        bad = good.copy()
        bad[fld] = 0
        assert ap(cols=bad) == -22, fld
    assert ap(n=0) == 0
    assert L.strom_sort_chars(P(p[0]), 8, 0, 8, 0, P(vals), 8, P(vals), P(out), 8, 0) == -22
    assert L.strom_sort_chars(P(p[0]), big, 0, 8, P(vals), P(vals), 8, P(vals), P(out), 8, 0) == -22
    torch.cuda.synchronize()
    # nothing was launched: the outputs and the error word are as they were
    assert int(err.item()) == 0 and bool((out == -1).all())
    with pytest.raises(ValueError, match="32 bits"):
        SO.State(big, "cuda")


# ------------------------------------------------------------ whole scans
@pytest.fixture(scope="module")
def files(S, tmp_path_factory):
    from arrowgen import write
    tbl = G.table(20_000, seed=6)
    d = tmp_path_factory.mktemp("sortgpu")
    paths = {}
    for codec in (None, "lz4"):
        paths[codec] = str(d / f"sort_{codec}.arrow")
        write(paths[codec], tbl, codec, batch_rows=3001)
    return tbl, paths


def _scan(path):
    from nvme_strom_amd.models.arrow_scan import ArrowScan
    sc = ArrowScan(path, "cuda", chunk_sz=64 << 10, slot_bytes=1 << 20, max_slot_bytes=1 << 20,
                   nslots=2)
    sc.MAX_SLOTS = 2
    return sc


def _same_columns(dev, host):
    """The device scan's ProjOuts against the host twin's, bit for bit where
    a row is valid."""
    assert [c.name for c in dev] == [c.name for c in host]
    for d, h in zip(dev, host):
        n = len(h.values) if h.offsets is None else len(h.offsets) - 1
        ok = np.ones(n, bool) if d.valid is None else d.valid.cpu().numpy() != 0
        hok = np.ones(n, bool) if h.valid is None else np.asarray(h.valid) != 0
        assert np.array_equal(ok, hok), d.name
        if h.offsets is not None:
            off = d.offsets.cpu().numpy()
            assert np.array_equal(off, h.offsets), d.name
            assert np.array_equal(d.values.cpu().numpy()[:off[-1]], h.values), d.name
            continue
        x = d.values.cpu().numpy()
        y = np.ascontiguousarray(h.values)
        assert x.shape == y.shape and x.dtype.itemsize == y.dtype.itemsize, d.name
        if n:
            xb, yb = x.view(np.uint8).reshape(n, -1), y.view(np.uint8).reshape(n, -1)
            assert np.array_equal(xb[ok], yb[ok]), d.name


def _reference(ftbl, mask, names, order_by, limit, offset):
    sel = ftbl.filter(mask)
    idx = pc.sort_indices(sel, sort_keys=SG.pa_sort_keys(order_by))
    rows = np.flatnonzero(np.asarray(mask.combine_chunks().fill_null(False)))[np.asarray(idx)]
    off = min(offset, len(rows))
    return SG.cut(sel.take(idx).select(names), limit, offset), \
        rows[off:] if limit is None else rows[off:off + limit]


@pytest.mark.parametrize("which", range(len(SG.ORDERS)))
@pytest.mark.parametrize("codec", [None, "lz4"])
def test_scan_order_by(S, files, codec, which):
    tbl, paths = files
    names, order_by = SG.ORDERS[which]
    quals, mask_of = G.quals_and_mask()
    ftbl = pa.ipc.open_file(paths[codec]).read_all()
    mask = mask_of(ftbl)
    sc = _scan(paths[codec])
    try:
        before = sc.scan_where(quals, project=names)
        for limit, offset in SG.WINDOWS:
            out = sc.scan_where(quals, project=names, order_by=order_by, limit=limit,
                                offset=offset)
            h = sc.host_scan_where(quals, project=names, order_by=order_by, limit=limit,
                                   offset=offset)
            want, ids = _reference(ftbl, mask, names, order_by, limit, offset)
            got = out.to_arrow()
            assert int(out.sort_errors.item()) == 0
            assert out.selected == before.selected > 1000
            assert np.array_equal(out.indices.cpu().numpy(), ids)
            assert np.array_equal(h.indices, ids)
            assert len(out.columns) == len(names) and out.order == h.order and \
                [k for k, _ in out.order] == [k for k, _ in SG.pa_sort_keys(order_by)]
            assert "sort_s" in out.seconds
            G.same_table(got, want)
            G.same_table(h.to_arrow(), want)
            _same_columns(out.columns, h.columns)
        # the scan without order_by is what it was: file order, the same ids
        again = sc.scan_where(quals, project=names)
        assert again.order is None and again.sort_errors is None and \
            "sort_s" not in again.seconds
        rows = np.flatnonzero(np.asarray(mask.combine_chunks().fill_null(False)))
        for o in (before, again):
            assert np.array_equal(o.indices.cpu().numpy(), rows)
            G.same_table(o.to_arrow(), G.reference(ftbl, mask, names))
    finally:
        sc.close()


def test_scan_order_by_expression_join_and_empty(S, files):
    from nvme_strom_amd.models.arrow_scan import Join, JoinTable, StarJoin
    from nvme_strom_amd.ops.colexpr import E
    from nvme_strom_amd.ops.colpred import P
    tbl, paths = files
    quals, _ = G.quals_and_mask()
    dims = G.dimensions()
    jt = {fk: JoinTable(keys, attrs=attrs, device="cuda") for fk, (keys, attrs) in dims.items()}
    sj = StarJoin(Join("fa", jt["fa"]), Join("fb", jt["fb"]))
    expr, ratio = E("i64") * 2 + E("i8"), E("f64") / E("f32")
    proj = [jt["fb"]["grp"], "s", expr, jt["fa"]["cat"], "b"]
    order_by = [("u8", "descending"), (ratio, "ascending"), expr]
    sc = _scan(paths["lz4"])
    try:
        for limit, offset in ((None, 0), (300, 11)):
            out = sc.scan_where(quals, project=proj, join=sj, order_by=order_by, limit=limit,
                                offset=offset)
            h = sc.host_scan_where(quals, project=proj, join=sj, order_by=order_by, limit=limit,
                                   offset=offset)
            assert out.selected > 300 and len(h.indices) == (limit or out.selected)
            assert np.array_equal(out.indices.cpu().numpy(), h.indices)
            assert out.to_arrow().equals(h.to_arrow())
            _same_columns(out.columns, h.columns)
        for kw in (dict(quals=[P("f64") > 2.0]), dict(quals=quals, batches=(3, 3))):
            out = sc.scan_where(kw["quals"], project=["s", "i8"], order_by=["f64n", "u8"],
                                batches=kw.get("batches"), limit=5)
            assert out.selected == 0 and out.indices.numel() == 0 and len(out.columns) == 2
            assert out.order == [("f64n", False), ("u8", False)]
            assert out.to_arrow().num_rows == 0
    finally:
        sc.close()
        for t in jt.values():
            t.close()
