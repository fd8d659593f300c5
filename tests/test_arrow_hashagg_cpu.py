"""by=HashBy on the CPU: host_aggregate through ops/colgroup.py's numpy twin
(key -> accumulators, the per-group arithmetic of ops/colagg.host_agg)
against pyarrow.Table.group_by under the comparison rule of tests/agggen.py.
Pins what the GPU kernels (tests/test_gpu_arrow_hashagg.py) are held to."""
import os
import sys

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")

sys.path.insert(0, os.path.dirname(__file__))

from agggen import same_results  # noqa: E402
from arrowgen import write  # noqa: E402
from hashagggen import (AGGS, BATCH_ROWS, KEYS, check, distinct, qual_lists, sorted_keys,  # noqa: E402
                        tables)


@pytest.fixture(scope="module", params=[None, "lz4", "zstd"])
def arrow_file(request, tmp_path_factory):
    tbl, _ = tables()
    path = str(tmp_path_factory.mktemp("hashagg") / f"t_{request.param}.arrow")
    write(path, tbl, request.param, batch_rows=BATCH_ROWS)
    return path


@pytest.mark.parametrize("key", KEYS, ids=[k for k, _ in KEYS])
@pytest.mark.parametrize("q", range(len(qual_lists())), ids=[c[0] for c in qual_lists()])
def test_hash_aggregate_matches_pyarrow(arrow_file, q, key):
    from nvme_strom_amd.models.arrow_scan import HashBy, host_aggregate
    label, quals, ref = qual_lists()[q]
    col, refcol = key
    out = host_aggregate(arrow_file, quals, AGGS, by=HashBy(col, groups=1 << 13))
    assert out.rows == tables()[0].num_rows and out.by == col
    check(out, label, ref, refcol)
    sorted_keys(out, unsigned=col == "u32")


def test_hashby_i8_equals_by_name(arrow_file):
    """The hash path and the key-indexed path give the same groups."""
    from nvme_strom_amd.models.arrow_scan import HashBy, host_aggregate
    for _, quals, _ in qual_lists():
        a = host_aggregate(arrow_file, quals, AGGS, by=HashBy("i8"))
        b = host_aggregate(arrow_file, quals, AGGS, by="i8")
        # by name the rows come in byte order (0..127, -128..-1), hashed by value
        order = sorted(range(len(b.keys)), key=lambda i: (b.keys[i] is None, b.keys[i] or 0))
        assert a.keys == [b.keys[i] for i in order] and a.selected == b.selected
        assert np.array_equal(a.count_all, b.count_all[order])
        for i in range(len(AGGS)):
            assert np.array_equal(a.valid[i], b.valid[i][order])
            ok = a.valid[i]
            x, y = a.values[i][ok], b.values[i][order][ok]
            if x.dtype.kind == "f" and AGGS[i][0] in ("sum", "mean"):
                # the two paths add in different orders: agggen.same_results' rule
                # (each is held to the bound against pyarrow on its own)
                assert np.array_equal(np.isnan(x), np.isnan(y)), AGGS[i]
                assert np.allclose(x, y, rtol=1e-9, atol=0, equal_nan=True), AGGS[i]
            else:
                assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), AGGS[i]


def test_merge_of_batch_ranges(arrow_file):
    """Three record-batch ranges, one of them empty, merged by key union."""
    from nvme_strom_amd.models.arrow_scan import HashBy, host_aggregate
    from nvme_strom_amd.ops.colpred import P
    quals = [P("f64") > 0.4]
    full = host_aggregate(arrow_file, quals, AGGS, by=HashBy("i64", 8000))
    parts = [host_aggregate(arrow_file, quals, AGGS, by=HashBy("i64", g), batches=r)
             for r, g in (((0, 2), 2000), ((2, 2), 1), ((2, 6), 4000))]
    assert parts[1].rows == 0 and parts[1].keys == []
    got = parts[0].merge(parts[1]).merge(parts[2])
    assert got.rows == full.rows
    same_results(got, full)
    check(got, "one", qual_lists()[1][2], "i64")
    with pytest.raises(ValueError):
        full.merge(host_aggregate(arrow_file, quals, AGGS[:3], by=HashBy("i64")))
    with pytest.raises(ValueError):
        full.merge(host_aggregate(arrow_file, quals, AGGS, by=HashBy("u32")))
    with pytest.raises(ValueError):                   # hashed with not hashed
        host_aggregate(arrow_file, quals, AGGS, by=HashBy("i8")).merge(
            host_aggregate(arrow_file, quals, AGGS, by="i8"))
    with pytest.raises(ValueError):
        host_aggregate(arrow_file, quals, AGGS, by="i8").merge(
            host_aggregate(arrow_file, quals, AGGS, by=HashBy("i8")))


def test_groups_limit(arrow_file):
    """groups = the distinct count passes, one less raises and names the
    column, groups and the distinct keys seen."""
    from nvme_strom_amd.models.arrow_scan import HashBy, host_aggregate
    aggs = [("count", None), ("sum", "f64")]
    for col in ("i64", "i8"):
        n = distinct(tables()[0], col)
        out = host_aggregate(arrow_file, [], aggs, by=HashBy(col, groups=n))
        assert len([k for k in out.keys if k is not None]) == n
        with pytest.raises(RuntimeError, match=rf"{col}.*groups={n - 1}\b.*\b{n} distinct"):
            host_aggregate(arrow_file, [], aggs, by=HashBy(col, groups=n - 1))


def test_boundaries(arrow_file):
    from nvme_strom_amd.models.arrow_scan import HashBy, host_aggregate
    aggs = [("count", None)]
    for col in ("f64", "s", "dict", "dec", "b"):
        with pytest.raises(NotImplementedError, match=col):
            host_aggregate(arrow_file, [], aggs, by=HashBy(col))
    for g in (0, (1 << 24) + 1, -3):
        with pytest.raises(ValueError):
            HashBy("i64", groups=g)
    assert HashBy("i64").groups == 1 << 16 and HashBy("i64", 1 << 24).groups == 1 << 24
    with pytest.raises(ValueError):
        host_aggregate(arrow_file, [], aggs, by=HashBy("nope"))
    # a bare integer key is still refused, and still by name
    with pytest.raises(NotImplementedError, match="i64"):
        host_aggregate(arrow_file, [], aggs, by="i64")


def test_twin_merge_and_wide_keys():
    """ops/colgroup.py on hand-made rows: uint64 keys on both sides of 2^63
    stay apart and sort by value; merge unites by key."""
    from nvme_strom_amd.ops import colagg as A
    from nvme_strom_amd.ops import colgroup as G
    ents = [A.Entry(A.COUNT | A.ALL), A.Entry(15, "i8")]
    k = np.array([5, 2**63 + 5, 2**64 - 1, 5, 0, 2**63], np.uint64)
    ok = np.array([1, 1, 1, 1, 0, 1], bool)
    v = np.array([1, 2, 3, 4, 5, -6], np.int64)
    sel = np.ones(6, bool)
    g = G.host_group_agg(ents, sel, k, ok, [(None, None), (v, None)])
    assert g.keys.dtype == np.uint64 and g.keys.tolist() == [5, 2**63, 2**63 + 5, 2**64 - 1]
    a = g.arrays(1)
    assert a["count"].tolist() == [2, 1, 1, 1, 1] and a["sum"].tolist() == [5, -6, 2, 3, 5]
    assert a["min"].tolist() == [1, -6, 2, 3, 5]
    h = G.host_group_agg(ents, sel[:2], np.array([7, 5], np.uint64), None,
                         [(None, None), (np.array([10, -20]), np.array([True, False]))])
    m = G.merge(g, h)
    assert m.keys.tolist() == [5, 7, 2**63, 2**63 + 5, 2**64 - 1]
    assert m.arrays(0)["count"].tolist() == [3, 1, 1, 1, 1, 1]
    assert m.arrays(1)["count"].tolist() == [2, 1, 1, 1, 1, 1]
    assert m.arrays(1)["max"].tolist()[:2] == [4, 10]
    i = G.host_group_agg(ents, sel, k.astype(np.int64), ok, [(None, None), (v, None)])
    assert i.keys.tolist() == [-(2**63), -(2**63) + 5, -1, 5]
    with pytest.raises(ValueError):
        G.merge(g, i)
    assert G.capacity(8) == 16 and G.capacity(1) == 2 and G.capacity(20_000) == 65536
    assert G.capacity(1 << 24) == 1 << 25
