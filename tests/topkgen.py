"""Shared inputs of the ORDER BY ... LIMIT k tests: the qualifier lists and
the pyarrow reference of whole scans, and hand-built record batches for the
kernels and their twins (shared by the CPU test and the GPU test)."""
from __future__ import annotations

import numpy as np

from nvme_strom_amd.ops.colpred import Or, P

ORDER_COLS = ["i8", "u32", "i64", "f32", "f64", "d32", "ts", "t32", "dur"]
KS = [1, 7, 700, 5000]
CODECS = [None, "lz4", "zstd"]
BATCH_ROWS = 700

_cache: dict = {}


def table():
    """arrowgen.table(): 3,000 rows, built once."""
    if "t" not in _cache:
        import arrowgen
        _cache["t"] = arrowgen.table()
    return _cache["t"]


def qual_lists():
    """(label, quals, pyarrow mask of the table or None for every row)."""
    import pyarrow.compute as pc
    c = lambda t, n: t.column(n).combine_chunks()
    return [
        ("none", [], None),
        ("nothing", [P("f64") > 2.0], lambda t: pc.greater(c(t, "f64"), 2.0)),
        ("range", [("i64", -5 * 10**11, 5 * 10**11)],
         lambda t: pc.and_(pc.greater_equal(c(t, "i64"), -5 * 10**11),
                           pc.less_equal(c(t, "i64"), 5 * 10**11))),
        ("or", [Or(P("i8") < -100, P("f64") > 0.9)],
         lambda t: pc.or_kleene(pc.less(c(t, "i8"), -100), pc.greater(c(t, "f64"), 0.9))),
    ]


def selected_ids(tbl, mask_fn, lo: int = 0, hi=None) -> np.ndarray:
    """The row ids ``mask_fn`` selects among rows [lo, hi), ascending."""
    hi = tbl.num_rows if hi is None else hi
    if mask_fn is None:
        return np.arange(lo, hi, dtype=np.int64)
    m = mask_fn(tbl).fill_null(False).to_numpy(zero_copy_only=False)
    ids = np.flatnonzero(m)
    return ids[(ids >= lo) & (ids < hi)].astype(np.int64)


def reference(tbl, ids: np.ndarray, col: str, descending: bool, k: int) -> np.ndarray:
    """pc.sort_indices(...)[:k] over the rows ``ids`` (ascending): the
    expected row ids, in result order.  pyarrow's sort is stable, puts NaN
    behind the numbers and nulls last in both directions."""
    import pyarrow as pa
    import pyarrow.compute as pc
    sub = pa.table({col: tbl.column(col).combine_chunks().take(pa.array(ids))})
    idx = pc.sort_indices(sub, [(col, "descending" if descending else "ascending")])
    return ids[np.asarray(idx)[:k]]


def storage(arr):
    """(values in the storage dtype with 0 for nulls, valid) of a pyarrow
    array: temporal types as their ticks."""
    import pyarrow as pa
    arr = arr.combine_chunks() if hasattr(arr, "combine_chunks") else arr
    valid = np.asarray(arr.is_valid())
    t = arr.type
    if pa.types.is_temporal(t):
        arr = arr.view(pa.int32() if t.bit_width == 32 else pa.int64())
    if pa.types.is_dictionary(arr.type):
        arr = arr.indices
    vals = arr.fill_null(0).to_numpy(zero_copy_only=False)
    return vals, valid


def check_result(out, tbl, want_ids: np.ndarray, col: str, nulls: bool, project=None,
                 pnulls: bool = False, label="") -> None:
    """``out`` (a TopOut) is exactly the rows ``want_ids`` with the table's
    values, validity and carried column."""
    import pyarrow as pa
    assert out.rows.dtype == np.int64 and out.rows.tolist() == want_ids.tolist(), label
    take = pa.array(want_ids)
    vals, valid = storage(tbl.column(col).combine_chunks().take(take))
    assert out.values.dtype == vals.dtype, label
    # a NaN comes back as a NaN, a null as 0
    assert np.array_equal(out.values, vals, equal_nan=vals.dtype.kind == "f"), label
    if vals.dtype.kind == "f":
        assert np.array_equal(np.signbit(out.values), np.signbit(vals)), label
    if nulls:
        assert np.array_equal(out.valid, valid), label
    else:
        assert out.valid is None and valid.all(), label
    if project is None:
        assert out.projected is None and out.projected_valid is None, label
        return
    pv, pok = storage(tbl.column(project).combine_chunks().take(take))
    assert out.projected.dtype == pv.dtype and np.array_equal(out.projected, pv), label
    if pnulls:
        assert np.array_equal(out.projected_valid, pok), label
    else:
        assert out.projected_valid is None, label


# ------------------------------------------------------------ kernels alone
ROWS = [1, 63, 64, 65, 200]
DTYPES = ["i1", "i2", "i4", "i8", "u1", "u2", "u4", "u8", "f4", "f8"]
KERNEL_KS = [1, 2, 3, 64, 65, 1024]
PREFILL = 0xA5A5A5A5A5A5A5A5


def _specials(dt: np.dtype) -> np.ndarray:
    if dt.kind == "f":
        return np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1.5, -1.5,
                         np.finfo(dt).max, np.finfo(dt).tiny], dt)
    info = np.iinfo(dt)
    vals = [info.min, info.max, 0, 1]
    if dt == np.uint64:
        vals += [1 << 63, (1 << 63) - 1, (1 << 64) - 1]
    if dt == np.int64:
        vals += [-1, -(1 << 63), (1 << 63) - 1]
    return np.array(vals, dt)


def values(dtype, case: str, n: int, descending: bool, seed: int = 0) -> np.ndarray:
    """``n`` values of a case: "random" (a third of them the type's special
    values: its ends, uint64 >= 2^63, NaN, infinities, both zeros), "equal"
    (one value: the row id alone orders), "zeros" (floats: -0.0 and +0.0
    mixed, equal as keys), "worst" (every row comes before all rows ahead of
    it in the query's direction) and "best" (the opposite)."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    if case == "equal":
        return np.full(n, 7, dt)
    if case == "zeros":
        v = np.zeros(n, dt)
        v[rng.random(n) < 0.5] = -0.0 if dt.kind == "f" else 0
        return v
    if dt.kind == "f":
        v = rng.normal(0, 100, n).astype(dt)
    else:
        info = np.iinfo(dt)
        v = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    if case == "random":
        sp = _specials(dt)
        hit = rng.random(n) < 0.33
        v[hit] = sp[rng.integers(0, len(sp), int(hit.sum()))]
        return v
    v = np.sort(v)                       # ascending
    if (case == "worst") != descending:
        v = v[::-1].copy()               # worst ascending query: descending values
    return v


def batches(dtype, case: str, descending: bool, rows=ROWS, seed: int = 0, null_p: float = 0.2,
            row_base: int = 0):
    """(per batch (values, valid or None, row_base), per batch (int32 payload,
    valid or None)): nulls on the odd batches only."""
    rng = np.random.default_rng(seed + 1000)
    v = values(dtype, case, int(sum(rows)), descending, seed)
    out, pay, at, base = [], [], 0, row_base
    for b, n in enumerate(rows):
        ok = (rng.random(n) >= null_p) if (b % 2 and null_p) else None
        out.append((v[at:at + n].copy(), ok, base))
        pay.append((rng.integers(-2**31, 2**31, n).astype(np.int32),
                    (rng.random(n) >= 0.3) if b % 2 == 0 else None))
        at += n
        base += n + 5                    # row ids need not be dense
    return out, pay


def nwords(rows) -> int:
    return int(sum((r + 63) // 64 for r in rows))


def bitmap(rows, kind: str, seed: int = 0) -> np.ndarray:
    """Source words: "all" and "random" with garbage beyond each batch's
    rows (set bits there must be ignored), "percent" about 1 in 100, "none"."""
    rng = np.random.default_rng(seed + 2000)
    n = nwords(rows)
    if kind == "none":
        return np.zeros(n, np.uint64)
    if kind == "all":
        return np.full(n, 0xFFFFFFFFFFFFFFFF, np.uint64)
    w = rng.integers(0, 1 << 63, n, dtype=np.int64).view(np.uint64) * np.uint64(2) + \
        rng.integers(0, 2, n).astype(np.uint64)
    if kind == "percent":
        for _ in range(6):
            w &= rng.integers(0, 1 << 63, n, dtype=np.int64).view(np.uint64) * np.uint64(2)
    return w


def expected(batch_list, src: np.ndarray, k: int, descending: bool, pay=None):
    """The k best (row, payload, payload valid) of the selected rows by plain
    Python comparison: (class, value in the direction, row)."""
    recs = []
    w0 = 0
    for b, (v, ok, base) in enumerate(batch_list):
        n = len(v)
        nw = (n + 63) // 64
        sel = np.unpackbits(src[w0:w0 + nw].view(np.uint8), bitorder="little")[:n].astype(bool)
        w0 += nw
        for r in np.flatnonzero(sel).tolist():
            x = v[r]
            if ok is not None and not ok[r]:
                key = (2, 0)
            elif v.dtype.kind == "f" and np.isnan(x):
                key = (1, 0)
            else:
                x = float(x) if v.dtype.kind == "f" else int(x)
                key = (0, -x if descending else x)
            p = (0, 0)
            if pay is not None and (pay[b][1] is None or pay[b][1][r]):
                p = (int(pay[b][0][r]), 1)
            recs.append((key, base + r) + p)
    recs.sort(key=lambda t: (t[0], t[1]))
    return [(row, p, pv) for _, row, p, pv in recs[:k]]
