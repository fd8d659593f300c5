"""Aggregate queries over the tests/arrowgen.py table, their pyarrow
references and the comparison rule (shared by the CPU test of the host twin
and the GPU test of ArrowScan.aggregate).

Comparison rule: counts, integer sums and every min / max are exact (NaN
matches NaN).  A float sum of n values x_i must be within
n * 2^-52 * sum|x_i| of math.fsum(x_i): the bound of a recursive sum in any
order, (n - 1) * 2^-53 * sum|x|, with a factor 2 for the final roundings of
result and reference."""
from __future__ import annotations

import math

import numpy as np

from nvme_strom_amd.ops.colpred import P

from arrowgen import cnf_cases

AGGS = [("count", None),
        ("sum", "i64"), ("min", "i64"), ("max", "i64"), ("count", "i64"), ("mean", "i64"),
        ("sum", "u32"), ("min", "u32"), ("max", "u32"),
        ("sum", "i8"), ("min", "i8"), ("max", "i8"),
        ("sum", "f64"), ("min", "f64"), ("max", "f64"), ("mean", "f64"),
        ("sum", "f32"), ("min", "f32"), ("max", "f32"), ("count", "f32"),
        ("min", "ts"), ("max", "ts"), ("count", "ts"),
        ("min", "d32"), ("max", "d32"), ("count", "d32"),
        ("count", "s")]
KEYS = [None, "dict", "idict", "b", "i8"]
_TICKS = {"ts": "int64", "d32": "int32"}


def qual_lists():
    """(label, qualifier list, pyarrow mask or None): the empty list, one
    predicate and both CNF lists of arrowgen."""
    import pyarrow.compute as pc
    one = lambda t: pc.greater(t.column("f64").combine_chunks(), 0.4)
    return [("all", [], None), ("one", [P("f64") > 0.4], one)] + \
        [(lab, q, ref) for lab, q, ref in cnf_cases()]


def reference(tbl, mask_fn, key, aggs):
    """{key value ("ALL" without key): {"count_all": n, (fn, col): value or
    None}} from pyarrow.compute / Table.group_by, and per (key value, col)
    the float columns' (n, fsum, sum|x|, has NaN) for the sum bound."""
    import pyarrow as pa
    import pyarrow.compute as pc
    ft = tbl
    if mask_fn is not None:
        m = mask_fn(tbl)
        m = m.combine_chunks() if hasattr(m, "combine_chunks") else m
        ft = tbl.filter(m.fill_null(False))
    cols = sorted({c for _, c in aggs if c is not None})
    data = {}
    for c in cols:
        a = ft.column(c).combine_chunks()
        data[c] = a.cast(_TICKS[c]) if c in _TICKS else a
    ref, fl = {}, {}
    if key is None:
        r = {"count_all": ft.num_rows}
        for fn, c in aggs:
            if c is None:
                continue
            a = data[c]
            if fn == "count":
                r[(fn, c)] = pc.count(a).as_py()
            elif fn in ("sum", "mean"):
                r[("sum", c)] = pc.sum(a).as_py()
                r[("count", c)] = pc.count(a).as_py()
            else:
                r[(fn, c)] = pc.min_max(a)[fn].as_py()
        ref["ALL"] = r
        kcol = ["ALL"] * ft.num_rows
    else:
        k = ft.column(key).combine_chunks()
        if pa.types.is_dictionary(k.type):
            k = k.dictionary_decode()
        t2 = pa.table({"k": k, **data})
        want = [([], "count_all")]
        for fn, c in aggs:
            if c is None:
                continue
            for f in (("sum", "count") if fn in ("sum", "mean") else (fn,)):
                if (c, f) not in want:
                    want.append((c, f))
        g = t2.group_by(["k"], use_threads=False).aggregate(want).to_pydict()
        for i, kv in enumerate(g["k"]):
            r = {"count_all": g["count_all"][i]}
            for c, f in want[1:]:
                r[(f, c)] = g[f"{c}_{f}"][i]
            ref[kv] = r
        kcol = k.to_pylist()
    kcol = np.array([("\0none" if v is None else v) for v in kcol], dtype=object)
    for c in cols:
        if not pa.types.is_floating(data[c].type):
            continue
        ok = np.asarray(data[c].is_valid())
        x = np.asarray(data[c].fill_null(0)).astype(np.float64)
        for kv in ref:
            sel = ok & (kcol == ("\0none" if kv is None else kv)) if key is not None else ok
            v = x[sel]
            nan = bool(np.isnan(v).any())
            fl[(kv, c)] = (len(v), math.fsum(v[~np.isnan(v)]), float(np.abs(v[~np.isnan(v)]).sum()),
                           nan)
    return ref, fl


def _same(a, b) -> bool:
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return a == b


def check(out, tbl, mask_fn, key, aggs=None):
    """``out`` (an AggOut) against pyarrow under the comparison rule."""
    aggs = aggs if aggs is not None else AGGS
    ref, fl = reference(tbl, mask_fn, key, aggs)
    keys = out.keys if key is not None else ["ALL"]
    assert len(keys) == len(ref) and set(keys) == set(ref), (keys, list(ref))
    assert out.selected == sum(r["count_all"] for r in ref.values())
    for gi, kv in enumerate(keys):
        r = ref[kv]
        assert int(out.count_all[gi]) == r["count_all"], (kv, "count_all")
        for i, (fn, c) in enumerate(aggs):
            v, ok = out.values[i][gi], bool(out.valid[i][gi])
            what = (kv, fn, c, v, ok)
            if c is None:
                assert ok and int(v) == r["count_all"], what
            elif fn == "count":
                assert ok and int(v) == r[(fn, c)], what
            elif fn in ("min", "max"):
                want = r[(fn, c)]
                assert ok == (want is not None), what
                if ok:
                    assert _same(v.item(), want), what + (want,)
            elif (kv, c) in fl:                      # float sum / mean: the bound
                n, fs, sabs, nan = fl[(kv, c)]
                assert ok == (n > 0), what
                if not ok:
                    continue
                if nan:
                    assert math.isnan(v), what
                    continue
                bound = n * 2.0 ** -52 * sabs
                if fn == "mean":
                    assert abs(float(v) - fs / n) <= bound / n + 2.0 ** -52 * abs(fs / n), what
                else:
                    assert abs(float(v) - fs) <= bound, what + (fs, bound)
            else:                                    # integer sum / mean: exact
                want, cnt = r[("sum", c)], r[("count", c)]
                assert ok == (cnt > 0), what
                if ok and fn == "sum":
                    assert int(v) == want, what + (want,)
                elif ok:
                    assert float(v) == float(want) / cnt, what


def same_results(a, b, aggs=None):
    """Two AggOuts of one query (GPU and host twin): everything but the
    float sums and means bit for bit, those within twice the bound's spirit
    (each is checked against pyarrow separately)."""
    aggs = aggs if aggs is not None else a.aggs
    assert a.keys == b.keys and a.selected == b.selected and a.rows == b.rows
    assert np.array_equal(a.count_all, b.count_all)
    for i, (fn, c) in enumerate(aggs):
        assert np.array_equal(a.valid[i], b.valid[i]), (fn, c)
        ok = a.valid[i]
        x, y = a.values[i][ok], b.values[i][ok]
        if x.dtype.kind == "f" and fn in ("sum", "mean"):
            assert np.array_equal(np.isnan(x), np.isnan(y)), (fn, c)
        else:
            assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), (fn, c, x, y)
