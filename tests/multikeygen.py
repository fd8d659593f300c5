"""by=HashBy([...]) queries — GROUP BY several key columns — over a table of
low-cardinality keys, and their pyarrow references (shared by
tests/test_arrow_multikey_cpu.py and tests/test_gpu_arrow_multikey.py).  The
comparison rule is tests/agggen.py's; the reference of a (qualifier list, key
list) pair is computed once and reused for every codec and for the CPU and the
GPU test.

The table is tests/arrowgen.py's (the value and qualifier columns of
agggen.AGGS / agggen.qual_lists) plus key columns that are all functions of
one hidden group number, so that a list of four of them still has far fewer
groups than rows: a test where every row is its own group shows nothing."""
from __future__ import annotations

import math

import numpy as np

import agggen
from agggen import AGGS, qual_lists  # noqa: F401

ROWS, SEED, BATCH_ROWS, HIDDEN = 6000, 17, 1000, 180
# (components, bits=): 2, 2, 3 and 4 components; the last is exactly 64 bits
# wide (32 + 8 + 16 + 1 + 6 + 1), the third needs bits= for its int64 column
KEY_LISTS = [
    (("k16", "kd"), {}),
    (("k32", "ku8"), {}),
    (("ku8", "k64", "klate"), {"k64": 40, "klate": 8}),
    (("ku32", "ku8", "k16", "klate"), {"klate": 6}),
]
_TBL = []
_REF = {}


def table():
    """6,000 rows: k32 int32 with nulls (40 values), k16 int16 with nulls
    (25), kd date32 (10), k64 int64 within +-2^39 with nulls (30), ku8 uint8
    (4), ku32 uint32 without nulls (12, on both sides of 2^31), klate int32
    (5 values in [-32, 32)) whose nulls all lie in the last batch."""
    if _TBL:
        return _TBL[0]
    import pyarrow as pa
    from arrowgen import table as base
    tbl = base(ROWS, seed=SEED)
    rng = np.random.default_rng(SEED + 1)
    g = rng.integers(0, HIDDEN, ROWS)
    pick = lambda vals: np.asarray(vals)[g % len(vals)]
    nulls = lambda p=0.07: rng.random(ROWS) < p
    v32 = np.unique(np.concatenate([[-2**31, 2**31 - 1, 0, -1],
                                    rng.integers(-2**31, 2**31, 60)]))[:40].astype(np.int32)
    v16 = np.unique(np.concatenate([[-2**15, 2**15 - 1, 0],
                                    rng.integers(-2**15, 2**15, 40)]))[:25].astype(np.int16)
    v64 = np.unique(np.concatenate([[-2**39, 2**39 - 1, 0, -1],
                                    rng.integers(-2**39, 2**39, 50)]))[:30].astype(np.int64)
    vu32 = np.array([0, 1, 2**31 - 1, 2**31, 2**32 - 1, 77, 10**9, 3 * 10**9, 5, 6, 7, 8], np.uint32)
    late = np.zeros(ROWS, bool)
    late[ROWS - BATCH_ROWS:] = rng.random(BATCH_ROWS) < 0.2
    cols = {
        "k32": pa.array(pick(v32), mask=nulls()),
        "k16": pa.array(pick(v16), mask=nulls()),
        "kd": pa.array(pick(np.arange(18000, 20000, 200, dtype=np.int32)), pa.int32())
        .cast(pa.date32()),
        "k64": pa.array(pick(v64), mask=nulls()),
        "ku8": pa.array(pick(np.array([0, 1, 128, 255], np.uint8))),
        "ku32": pa.array(pick(vu32)),
        "klate": pa.array(pick(np.array([-32, -1, 0, 7, 31], np.int32)), mask=late),
    }
    for n, a in cols.items():
        tbl = tbl.append_column(n, a)
    assert tbl.column("ku32").null_count == 0 and tbl.column("klate").null_count > 0
    assert tbl.slice(0, ROWS - BATCH_ROWS).column("klate").null_count == 0
    _TBL.append(tbl)
    for keys, _ in KEY_LISTS:
        few_groups(tbl, keys)
    return tbl


def few_groups(tbl, keys) -> int:
    """The groups of ``keys`` over every row, asserted to be at most a
    quarter of the rows."""
    n = _key_table(tbl, keys).group_by([f"__k{i}" for i in range(len(keys))],
                                       use_threads=False).aggregate([([], "count_all")]).num_rows
    assert 1 < n <= tbl.num_rows // 4, (keys, n, tbl.num_rows)
    return n


def _key_table(tbl, keys):
    """The key columns as ``__k<i>``: dates as their day numbers."""
    import pyarrow as pa
    out = {}
    for i, k in enumerate(keys):
        a = tbl.column(k).combine_chunks()
        if pa.types.is_date32(a.type):
            a = a.cast(pa.int32())
        out[f"__k{i}"] = a
    return pa.table(out)


def reference(tbl, mask_fn, keys, aggs):
    """agggen.reference for a list of key columns: {key tuple: {"count_all":
    n, (fn, col): value or None}} from pyarrow's Table.group_by(keys), and per
    (key tuple, float column) its (n, fsum, sum|x|, has NaN)."""
    import pyarrow as pa
    ft = tbl
    if mask_fn is not None:
        m = mask_fn(tbl)
        m = m.combine_chunks() if hasattr(m, "combine_chunks") else m
        ft = tbl.filter(m.fill_null(False))
    cols = sorted({c for _, c in aggs if c is not None})
    data = {}
    for c in cols:
        a = ft.column(c).combine_chunks()
        data[c] = a.cast(agggen._TICKS[c]) if c in agggen._TICKS else a
    kt = _key_table(ft, keys)
    kn = kt.column_names
    t2 = pa.table({**{n: kt.column(n) for n in kn}, **data})
    want = [([], "count_all")]
    for fn, c in aggs:
        if c is None:
            continue
        for f in (("sum", "count") if fn in ("sum", "mean") else (fn,)):
            if (c, f) not in want:
                want.append((c, f))
    g = t2.group_by(kn, use_threads=False).aggregate(want).to_pydict()
    ref, fl = {}, {}
    tuples = list(zip(*(g[n] for n in kn)))
    for i, kv in enumerate(tuples):
        r = {"count_all": g["count_all"][i]}
        for c, f in want[1:]:
            r[(f, c)] = g[f"{c}_{f}"][i]
        ref[kv] = r
    at = {kv: i for i, kv in enumerate(tuples)}
    gid = np.array([at[kv] for kv in zip(*(kt.column(n).to_pylist() for n in kn))], np.int64)
    for c in cols:
        if not pa.types.is_floating(data[c].type):
            continue
        ok = np.asarray(data[c].is_valid())
        x = np.asarray(data[c].fill_null(0)).astype(np.float64)
        for i, kv in enumerate(tuples):
            v = x[ok & (gid == i)]
            nan = np.isnan(v)
            fl[(kv, c)] = (len(v), math.fsum(v[~nan]), float(np.abs(v[~nan]).sum()), bool(nan.any()))
    return ref, fl


def check(out, label: str, mask_fn, keys, aggs=None, tbl=None, tag=None, rank=None):
    """agggen.check of ``out`` against pyarrow's group_by(keys) of the table
    (or ``tbl``, then ``tag`` names it), computed once per (label, keys,
    aggs); then the order of the rows: lexicographic, each column ascending
    (``rank[i]``: the order of component i's values, when it is not their
    own), nulls last per column."""
    ref_tbl = tbl if tbl is not None else table()
    use = aggs if aggs is not None else AGGS
    k = (tag, label, tuple(keys), tuple(use))
    if k not in _REF:
        _REF[k] = reference(ref_tbl, mask_fn, keys, use)
    if mask_fn is None:
        # every tested key list: far fewer groups than rows
        assert 1 < len(_REF[k][0]) <= ref_tbl.num_rows // 4, (keys, len(_REF[k][0]))
    orig = agggen.reference
    agggen.reference = lambda *a, **kw: _REF[k]
    try:
        agggen.check(out, ref_tbl, mask_fn, "tuple", use)
    finally:
        agggen.reference = orig
    rank = rank or [None] * len(keys)
    # (a ranked component — a join attribute — has no nulls: None is one of its values)
    order = lambda t: tuple((False, r(x)) if r else (x is None, 0 if x is None else x)
                            for x, r in zip(t, rank))
    assert out.keys == sorted(_REF[k][0], key=order)
    assert all(type(t) is tuple and len(t) == len(keys) for t in out.keys)
    # key_columns say the same as keys
    assert len(out.key_columns) == len(keys)
    for i, (v, ok) in enumerate(out.key_columns):
        assert [x if o else None for x, o in zip(v.tolist(), ok.tolist())] == \
            [t[i] for t in out.keys]


def hash_by(keys, bits, groups=1 << 12):
    from nvme_strom_amd.models.arrow_scan import HashBy
    return HashBy(list(keys), groups=groups, bits=bits)
