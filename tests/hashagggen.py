"""by=HashBy queries over the tests/arrowgen.py table and their pyarrow
references (shared by tests/test_arrow_hashagg_cpu.py and
tests/test_gpu_arrow_hashagg.py).  The comparison rule is tests/agggen.py's;
the reference of a (qualifier list, key) pair is computed once and reused
for every codec and for the CPU and the GPU test."""
from __future__ import annotations

import numpy as np

import agggen
from agggen import AGGS, qual_lists  # noqa: F401

ROWS, SEED, BATCH_ROWS = 6000, 11, 1000
# (HashBy column, the reference table's key column)
KEYS = [("i64", "i64"), ("u32", "u32"), ("i8", "i8"), ("ts", "ts_ticks"), ("d32", "d32_ticks")]
_TBL = []
_REF = {}


def tables():
    """(the table the files are written from, the same with ``ts`` and
    ``d32`` added as integer tick columns for the reference)."""
    if not _TBL:
        import pyarrow as pa
        from arrowgen import table
        tbl = table(ROWS, seed=SEED)
        ref = tbl.append_column("ts_ticks", tbl.column("ts").cast(pa.int64()))
        ref = ref.append_column("d32_ticks", tbl.column("d32").cast(pa.int32()))
        _TBL.extend([tbl, ref])
    return _TBL[0], _TBL[1]


def check(out, label: str, mask_fn, key: str, aggs=None, tbl=None, tag=None) -> None:
    """agggen.check of ``out`` against the reference table (or ``tbl``,
    then ``tag`` names it), with the pyarrow reference of (label, key, aggs)
    computed once."""
    ref_tbl = tbl if tbl is not None else tables()[1]
    use = aggs if aggs is not None else AGGS
    k = (tag, label, key, tuple(use))
    if k not in _REF:
        _REF[k] = agggen.reference(ref_tbl, mask_fn, key, use)
    orig = agggen.reference
    agggen.reference = lambda *a, **kw: _REF[k]
    try:
        agggen.check(out, ref_tbl, mask_fn, key, use)
    finally:
        agggen.reference = orig


def sorted_keys(out, unsigned: bool = False) -> None:
    """Rows ascending by key value, the null group last, keys Python ints."""
    ks = [k for k in out.keys if k is not None]
    assert all(type(k) is int for k in ks)
    assert ks == sorted(ks) and len(set(ks)) == len(ks)
    assert out.keys[:len(ks)] == ks                 # None, if any, is last
    if unsigned:
        assert all(k >= 0 for k in ks)


def distinct(tbl, col: str, mask_fn=None) -> int:
    """Distinct non-null values of ``col`` among the selected rows."""
    import pyarrow.compute as pc
    if mask_fn is not None:
        m = mask_fn(tbl)
        m = m.combine_chunks() if hasattr(m, "combine_chunks") else m
        tbl = tbl.filter(m.fill_null(False))
    return pc.count_distinct(tbl.column(col), mode="only_valid").as_py()


def big_table(n: int = 200_000, nkeys: int = 50_000, seed: int = 29):
    """An int64 key of ``nkeys`` distinct values (spread over the int64
    range, 3 % nulls), an int64, a float64 with nulls and an int32 column."""
    import pyarrow as pa
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(-2**62, 2**62, 2 * nkeys))[:nkeys]
    k = pool[rng.integers(0, nkeys, n)]
    k[:nkeys] = pool                                 # every key appears
    knull = rng.random(n) < 0.03
    knull[:nkeys] = False
    return pa.table({"k": pa.array(k, mask=knull),
                     "a": pa.array(rng.integers(-10**15, 10**15, n)),
                     "x": pa.array(rng.normal(0, 1e3, n), mask=rng.random(n) < 0.1),
                     "c": pa.array(rng.integers(-10**6, 10**6, n).astype(np.int32))})


def check_by_runs(out, tbl, key: str, aggs) -> None:
    """agggen's comparison rule for a table of many groups and no
    qualifier: the rows sorted by key, each group one run (agggen.reference
    compares an object column once per group: too slow for 50,000 of them)."""
    import math
    k = tbl.column(key).combine_chunks()
    kok = np.asarray(k.is_valid())
    kv = np.asarray(k.fill_null(0))
    order = np.lexsort((kv, ~kok))                    # by key, the null keys last
    skv, sok = kv[order], kok[order]
    new = np.ones(len(order), bool)
    new[1:] = (skv[1:] != skv[:-1]) | (sok[1:] != sok[:-1])
    start = np.flatnonzero(new)
    end = np.append(start[1:], len(order))
    keys = [int(skv[s]) if sok[s] else None for s in start]
    assert out.keys == keys and out.selected == tbl.num_rows
    assert out.count_all.tolist() == (end - start).tolist()
    cols = {}
    for c in {c for _, c in aggs if c is not None}:
        a = tbl.column(c).combine_chunks()
        cols[c] = (np.asarray(a.fill_null(0))[order], np.asarray(a.is_valid())[order])
    for i, (fn, c) in enumerate(aggs):
        if c is None:
            assert out.values[i].tolist() == (end - start).tolist()
    for c, (x, ok) in cols.items():
        flt = x.dtype.kind == "f"
        mine = [(i, fn) for i, (fn, cc) in enumerate(aggs) if cc == c]
        runs = [x[s:e][ok[s:e]] for s, e in zip(start.tolist(), end.tolist())]
        for (i, fn), (gi, v) in ((a, b) for a in mine for b in enumerate(runs)):
            got, has = out.values[i][gi], bool(out.valid[i][gi])
            what = (keys[gi], fn, c, got, has)
            if fn == "count":
                assert has and int(got) == len(v), what
                continue
            assert has == (len(v) > 0), what
            if not has:
                continue
            if fn in ("min", "max"):
                assert got == (v.min() if fn == "min" else v.max()), what
            elif not flt:
                want = int(v.astype(np.int64).sum())
                assert (int(got) == want) if fn == "sum" else (float(got) == want / len(v)), what
            else:
                fs, bound = math.fsum(v), len(v) * 2.0 ** -52 * float(np.abs(v).sum())
                if fn == "sum":
                    assert abs(float(got) - fs) <= bound, what + (fs, bound)
                else:
                    n = len(v)
                    assert abs(float(got) - fs / n) <= bound / n + 2.0 ** -52 * abs(fs / n), what


BIG_AGGS = [("count", None), ("sum", "a"), ("min", "a"), ("max", "a"), ("sum", "x"), ("min", "x"),
            ("max", "x"), ("count", "x"), ("mean", "x"), ("sum", "c"), ("max", "c")]
