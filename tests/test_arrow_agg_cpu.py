"""Arrow scan aggregation on the CPU: host_aggregate (the metadata reader,
the decoders' host twins, colpred's numpy twin of the qualifier kernel and
ops/colagg.py's numpy twin of the aggregate kernels) against
pyarrow.compute / Table.group_by.  Pins the semantics the GPU kernels
(tests/test_gpu_arrow_agg.py) are held to: wrapping integer sums, float64
float sums, NaN and null rules, null-key groups."""
import math

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")

from agggen import AGGS, KEYS, check, qual_lists  # noqa: E402
from arrowgen import table, write  # noqa: E402


@pytest.fixture(scope="module", params=[None, "lz4", "zstd"])
def arrow_file(request, tmp_path_factory):
    tbl = table(3000)
    path = str(tmp_path_factory.mktemp("agg") / f"t_{request.param}.arrow")
    write(path, tbl, request.param, batch_rows=700)
    return path, tbl


@pytest.mark.parametrize("key", KEYS, ids=[str(k) for k in KEYS])
@pytest.mark.parametrize("q", range(len(qual_lists())), ids=[c[0] for c in qual_lists()])
def test_aggregate_matches_pyarrow(arrow_file, q, key):
    from nvme_strom_amd.models.arrow_scan import host_aggregate
    path, tbl = arrow_file
    _, quals, ref = qual_lists()[q]
    out = host_aggregate(path, quals, AGGS, by=key)
    assert out.rows == tbl.num_rows
    check(out, tbl, ref, key)
    for (fn, c), col in zip(out.aggs, out.columns):
        if c == "ts":
            assert col.kind == "timestamp" and col.unit == "us"


@pytest.mark.parametrize("key", [None, "dict"])
def test_f32_sum_nan_and_numeric(arrow_file, key):
    """3 % of the f32 values are NaN: every group's sum is NaN as it is; with
    the NaNs filtered out the sum is compared numerically."""
    import pyarrow.compute as pc
    from nvme_strom_amd.models.arrow_scan import host_aggregate
    from nvme_strom_amd.ops.colpred import P
    path, tbl = arrow_file
    aggs = [("count", None), ("sum", "f32"), ("mean", "f32")]
    out = host_aggregate(path, [], aggs, by=key)
    v, ok = out.get("sum", "f32")
    assert ok.all() and np.isnan(v).all()
    check(out, tbl, None, key, aggs)
    out = host_aggregate(path, [P("f32") <= 1e30], aggs, by=key)
    v, ok = out.get("sum", "f32")
    assert ok.all() and not np.isnan(v).any()
    check(out, tbl, lambda t: pc.less_equal(t.column("f32").combine_chunks(), 1e30), key, aggs)


@pytest.mark.parametrize("key", [None, "dict", "b"])
def test_empty_selection(arrow_file, key):
    import pyarrow.compute as pc
    from nvme_strom_amd.models.arrow_scan import host_aggregate
    from nvme_strom_amd.ops.colpred import P
    path, tbl = arrow_file
    out = host_aggregate(path, [P("i64") > 10**13], AGGS, by=key)
    assert out.selected == 0 and int(out.count_all.sum()) == 0
    if key is None:
        assert out.keys is None and len(out.count_all) == 1
        for (fn, c), v, ok in zip(out.aggs, out.values, out.valid):
            assert bool(ok[0]) == (fn == "count") and (fn != "count" or v[0] == 0)
    else:
        assert out.keys == [] and all(len(v) == 0 for v in out.values)
    check(out, tbl, lambda t: pc.greater(t.column("i64").combine_chunks(), 10**13), key)


@pytest.mark.parametrize("key", [None, "idict"])
def test_merge_of_batch_ranges(arrow_file, key):
    """Record-batch ranges merged equal the whole file: integers and counts
    exactly, float sums within the bound (check applies it)."""
    from agggen import same_results
    from nvme_strom_amd.models.arrow_scan import host_aggregate
    from nvme_strom_amd.ops.colpred import P
    path, tbl = arrow_file
    quals = [P("f64") > 0.4]
    full = host_aggregate(path, quals, AGGS, by=key)
    parts = [host_aggregate(path, quals, AGGS, by=key, batches=r) for r in ((0, 2), (2, 2), (2, 5))]
    assert parts[1].rows == 0 and parts[1].selected == 0
    got = parts[0].merge(parts[1]).merge(parts[2])
    assert got.rows == full.rows
    same_results(got, full)
    check(got, tbl, qual_lists()[1][2], key)
    with pytest.raises(ValueError):
        full.merge(host_aggregate(path, quals, AGGS[:3], by=key))


def test_boundaries(arrow_file):
    from nvme_strom_amd.models.arrow_scan import host_aggregate
    path, _ = arrow_file
    for bad in ([("sum", "dec")], [("min", "s")], [("max", "b")], [("sum", "dict")],
                [("sum", "ts")]):
        with pytest.raises(NotImplementedError, match=bad[0][1]):
            host_aggregate(path, [], bad)
    with pytest.raises(NotImplementedError, match="i64"):
        host_aggregate(path, [], [("count", None)], by="i64")
    with pytest.raises(ValueError):
        host_aggregate(path, [], [("median", "i64")])
    with pytest.raises(ValueError):
        host_aggregate(path, [], [("sum", "nope")])
    with pytest.raises(ValueError):
        host_aggregate(path, [], [("count", None)], by="nope")
    # count works on every supported kind
    out = host_aggregate(path, [], [("count", c) for c in ("dec", "s", "b", "dict", "bin", "ls")])
    assert all(ok.all() for ok in out.valid)


def test_twin_semantics_and_limits():
    """ops/colagg.py on hand-made rows: wrapping sums, NaN rules, null and
    malformed keys, the order-preserving keys, the LDS limit."""
    from nvme_strom_amd.ops import colagg as A
    lay = A.Layout([A.Entry(A.COUNT | A.ALL), A.Entry(15, "i8", "x"), A.Entry(15, "f4", "f"),
                    A.Entry(15, "u8", "u")], nslots=4, key_code=1)
    blk = A.new_block(lay)
    n = 8
    sel = np.array([1, 1, 1, 1, 1, 1, 1, 0], bool)
    kv = np.array([0, 1, -1, 5, 2, 1, 0, 0], np.int32)
    kok = np.array([1, 1, 1, 1, 0, 1, 1, 1], bool)
    x = np.array([2**63 - 1, 5, 1, 1, -7, 2**63 - 1, 3, 9], np.int64)
    f = np.array([np.nan, np.nan, 0, 0, -0.5, np.nan, 1.5, 0], np.float32)
    u = np.array([2**64 - 1, 0, 0, 0, 7, 2**64 - 1, 1, 0], np.uint64)
    fok = np.array([1, 1, 1, 1, 1, 1, 0, 1], bool)
    for e, (v, ok) in enumerate([(None, None), (x, None), (f, fok), (u, None)]):
        A.host_agg(lay, blk, e, sel, v, ok, (kv, kok), count_bad=e == 0)
    assert int(blk[0]) == 2                       # indices -1 and 5
    assert A.entry_arrays(lay, blk, 0)["count"].tolist() == [2, 2, 0, 1]
    a = A.entry_arrays(lay, blk, 1)
    assert a["sum"].tolist() == [2**63 - 1 + 3 - 2**64, 5 + 2**63 - 1 - 2**64, 0, -7]   # wraps
    assert a["min"].tolist()[:2] == [3, 5] and a["max"].tolist()[3] == -7
    a = A.entry_arrays(lay, blk, 2)
    assert a["count"].tolist() == [1, 2, 0, 1]    # the null f of slot 0 is skipped
    assert math.isnan(a["sum"][0]) and math.isnan(a["min"][1]) and math.isnan(a["max"][1])
    assert a["min"][3] == -0.5 and a["min"].dtype == np.float32
    a = A.entry_arrays(lay, blk, 3)
    assert a["max"].tolist()[:2] == [2**64 - 1, 2**64 - 1] and a["sum"].tolist()[0] == 0
    for vals in (np.array([-5, 0, 3, -2**63, 2**63 - 1], np.int64),
                 np.array([0, 2**64 - 1, 17], np.uint64),
                 np.array([-np.inf, -1.5, -0.0, 0.0, 2.0, np.inf], np.float64)):
        k = A.order_keys(vals)
        assert (np.diff(k.astype(object)) >= 0).all() if vals.dtype.kind == "f" else \
            np.array_equal(np.argsort(k, kind="stable"), np.argsort(vals, kind="stable"))
        assert np.array_equal(A.key_values(k, vals.dtype.str[1:]), vals)
    assert A.max_slots(A.COUNT | A.SUM | A.MIN | A.MAX) == 2048 and A.max_slots(A.SUM) == 8192
    A.Layout([A.Entry(15, "i8")], nslots=2048, key_code=1)
    with pytest.raises(NotImplementedError, match="64 KiB"):
        A.Layout([A.Entry(15, "i8")], nslots=2049, key_code=1)
