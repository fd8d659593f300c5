"""by=HashBy([...]) — GROUP BY several key columns — on the CPU:
host_aggregate through ops/colgroup.py's KeySpec and numpy twin against
pyarrow.Table.group_by([...]) under the comparison rule of tests/agggen.py.
Pins what the GPU kernel (tests/test_gpu_arrow_multikey.py) is held to."""
import os
import sys

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")

sys.path.insert(0, os.path.dirname(__file__))

from agggen import same_results  # noqa: E402
from arrowgen import write  # noqa: E402
from multikeygen import (AGGS, BATCH_ROWS, KEY_LISTS, check, hash_by, qual_lists,  # noqa: E402
                         table)


@pytest.fixture(scope="module", params=[None, "lz4", "zstd"])
def arrow_file(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("multikey") / f"t_{request.param}.arrow")
    write(path, table(), request.param, batch_rows=BATCH_ROWS)
    return path


@pytest.fixture(scope="module")
def plain_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("multikey1") / "t.arrow")
    write(path, table(), None, batch_rows=BATCH_ROWS)
    return path


@pytest.mark.parametrize("kl", range(len(KEY_LISTS)), ids=["-".join(k) for k, _ in KEY_LISTS])
@pytest.mark.parametrize("q", range(len(qual_lists())), ids=[c[0] for c in qual_lists()])
def test_multikey_matches_pyarrow(arrow_file, q, kl):
    from nvme_strom_amd.models.arrow_scan import host_aggregate
    label, quals, ref = qual_lists()[q]
    keys, bits = KEY_LISTS[kl]
    out = host_aggregate(arrow_file, quals, AGGS, by=hash_by(keys, bits))
    assert out.rows == table().num_rows and out.by == tuple(keys)
    check(out, label, ref, keys)


def test_one_component_list_equals_plain(plain_file):
    """A list of one takes the composite path and says what the plain path
    says, as tuples."""
    from nvme_strom_amd.models.arrow_scan import HashBy, host_aggregate
    a = host_aggregate(plain_file, [], AGGS, by=HashBy(["k32"]))
    b = host_aggregate(plain_file, [], AGGS, by=HashBy("k32"))
    assert a.keys == [(k,) for k in b.keys] and b.key_columns is None
    assert a._found.spec is not None and b._found.spec is None
    assert np.array_equal(a.count_all, b.count_all)
    for i in range(len(AGGS)):
        assert np.array_equal(a.valid[i], b.valid[i])
        assert np.array_equal(a.values[i][a.valid[i]], b.values[i][b.valid[i]], equal_nan=True)


def test_keyspec_round_trip_and_order():
    """pack / unpack of every storage type with nulls and declared widths;
    unsigned order of the packed words is np.lexsort's order of the tuples,
    nulls after all values."""
    from nvme_strom_amd.ops import colgroup as G
    r = np.random.default_rng(5)
    n = 4000
    for comps in ([("a", "i4", None, True), ("b", "u4", None, False)],          # 65 bits
                  [("a", "i1", None, True), ("b", "u2", None, False), ("c", "i8", 38, True)],
                  [("a", "u1", 3, False), ("b", "i2", None, True), ("c", "u4", None, True),
                   ("d", "i1", 6, True)],
                  [("a", "i8", None, False)], [("a", "u8", 63, True)],
                  [("a", "i4", None, False), ("b", "u4", None, False)]):
        if sum((b or 8 * np.dtype(s).itemsize) + nu for _, s, b, nu in comps) > 64:
            with pytest.raises(NotImplementedError, match="bits="):
                G.KeySpec(comps)
            continue
        spec = G.KeySpec(comps)
        assert [c.shift for c in spec.comps][-1] == 0
        assert spec.comps[0].shift + spec.comps[0].width == sum(c.width for c in spec.comps) <= 64
        cols, oks = [], []
        for c in spec.comps:
            lo, hi = (-(1 << (c.bits - 1)), (1 << (c.bits - 1)) - 1) if c.signed else \
                (0, (1 << c.bits) - 1)
            # few values, the extremes among them: many equal components
            dt = np.dtype(c.storage)
            pool = np.concatenate([np.array([lo, hi, 0], dt),
                                   r.integers(lo, hi, 5, endpoint=True, dtype=dt)])
            cols.append(r.choice(pool, n))
            oks.append(r.random(n) > 0.2 if c.nullable else None)
        packed, fits = spec.pack(cols, oks)
        assert packed.dtype == np.uint64 and fits.all()
        vals, valid = spec.unpack(packed)
        for v, ok, c, o, k in zip(vals, valid, cols, oks, spec.comps):
            want = np.ones(n, bool) if o is None else o
            assert v.dtype == np.dtype(k.storage) and np.array_equal(ok, want)
            assert np.array_equal(v[want], c[want]) and (v[~want] == 0).all()
        # np.lexsort's last key is the primary one: the columns in reverse,
        # and within a column the value before its null flag
        ks = []
        for c, o in reversed(list(zip(cols, oks))):
            null = np.zeros(n, bool) if o is None else ~o
            ks += [np.where(null, 0, c), null]
        assert np.array_equal(packed[np.lexsort(ks)], np.sort(packed))
    # what does not fit: the first such component, by value and by null
    spec = G.KeySpec([("a", "i2", 4, False), ("b", "u1", 2, True)])
    packed, bad = spec.pack_why([np.array([7, 8, -8, -9, 0, 9], np.int16),
                                 np.array([3, 3, 0, 4, 4, 4], np.uint8)],
                                [np.array([1, 1, 1, 1, 1, 0], bool), np.array([1, 1, 1, 1, 1, 1], bool)])
    assert bad.tolist() == [-1, 0, -1, 0, 1, 0]
    assert packed[:3:2].tolist() == [(15 << 3) | 3, 0]
    # the free slot's pattern is an ordinary packed key
    spec = G.KeySpec([("a", "i4", None, False), ("b", "u4", None, False)])
    packed, fits = spec.pack([np.array([0], np.int32), np.array([0], np.uint32)], [None, None])
    assert packed.tolist() == [1 << 63] and fits.all()


def test_twin_by_hand():
    from nvme_strom_amd.ops import colagg as A
    from nvme_strom_amd.ops import colgroup as G
    ents = [A.Entry(A.COUNT | A.ALL), A.Entry(15, "i8")]
    spec = G.KeySpec([("a", "i1", None, True), ("b", "u2", 4, False)])
    a = np.array([5, -3, 5, 0, 5, -3, 1], np.int8)
    aok = np.array([1, 1, 1, 0, 1, 1, 1], bool)
    b = np.array([2, 2, 2, 2, 9, 2, 16], np.uint16)
    v = np.arange(7, dtype=np.int64)
    sel = np.array([1, 1, 1, 1, 1, 1, 1], bool)
    g, misfit = G.host_group_agg_multi(ents, sel, spec, [a, b], [aok, None], [(None, None), (v, None)])
    assert misfit.tolist() == [0, 1] and g.spec == spec and g.keys.dtype == np.uint64
    vals, oks = spec.unpack(g.keys)
    assert list(zip(vals[0].tolist(), oks[0].tolist(), vals[1].tolist())) == \
        [(-3, True, 2), (5, True, 2), (5, True, 9), (0, False, 2)]
    assert g.arrays(0)["count"].tolist() == [2, 2, 1, 1, 0]
    assert g.arrays(1)["sum"].tolist()[:4] == [6, 2, 4, 3]
    h, _ = G.host_group_agg_multi(ents, sel[:2], spec, [a[:2], b[:2]], [None, None],
                                  [(None, None), (v[:2], None)])
    m = G.merge(g, h)
    assert m.arrays(0)["count"].tolist() == [3, 3, 1, 1, 0] and m.spec == spec
    other = G.KeySpec([("a", "i1", None, False), ("b", "u2", 4, False)])
    o, _ = G.host_group_agg_multi(ents, sel, other, [a, b], [None, None], [(None, None), (v, None)])
    with pytest.raises(ValueError, match="packed differently"):
        G.merge(g, o)
    plain = G.host_group_agg(ents, sel, spec.pack([a, b], [aok, None])[0], None,
                             [(None, None), (v, None)])
    with pytest.raises(ValueError):
        G.merge(g, plain)


def _dim(tbl, **kw):
    from joingen import dimension
    from nvme_strom_amd.models.arrow_scan import JoinTable
    keys, cats, regs = dimension(tbl.column("i64").combine_chunks())
    return keys, cats, regs, JoinTable(keys, {"cat": cats, "reg": regs}, **kw)


JOIN_AGGS = [("count", None), ("sum", "i64"), ("min", "f64"), ("max", "f64"), ("sum", "f64"),
             ("count", "i8")]


def test_join_attribute_component(plain_file):
    """[dim["cat"], "kd"] after a semi-join against pyarrow's inner join +
    group_by; the attribute orders by its code."""
    import pyarrow.compute as pc
    from joingen import joined
    from nvme_strom_amd.models.arrow_scan import HashBy, Join, host_aggregate
    from nvme_strom_amd.ops.colpred import P
    tbl = table()
    keys, cats, regs, dim = _dim(tbl)
    j = joined(tbl, "i64", keys, {"cat": cats, "reg": regs}, "inner")
    code = {v: i for i, v in enumerate(dim["cat"].values)}
    for label, quals, ref in (("all", [], None),
                              ("f64", [P("f64") > 0.4],
                               lambda t: pc.greater(t.column("f64").combine_chunks(), 0.4))):
        for comps, names, rank in (([dim["cat"], "kd"], ("cat", "kd"), [code.get, None]),
                                   (["ku8", dim["reg"], "klate"], ("ku8", "reg", "klate"),
                                    [None, {v: i for i, v in enumerate(dim["reg"].values)}.get,
                                     None])):
            out = host_aggregate(plain_file, quals, JOIN_AGGS, by=HashBy(comps),
                                 join=Join("i64", dim))
            assert out.selected > 100 and out.by == names
            check(out, label, ref, names, JOIN_AGGS, tbl=j, tag="join", rank=rank)
            if names[0] == "cat":
                assert any(t[0] is None for t in out.keys)    # a null attribute value is a value


def test_merge_of_batch_ranges(plain_file):
    """klate has nulls in the last record batch only: a range without it
    packs the column nullable all the same (the rule looks at the whole
    file), so the ranges' packed keys agree and merge."""
    from nvme_strom_amd.models.arrow_scan import HashBy, host_aggregate
    from nvme_strom_amd.ops.colpred import P
    keys, bits = KEY_LISTS[3]
    quals = [P("f64") > 0.4]
    full = host_aggregate(plain_file, quals, AGGS, by=hash_by(keys, bits))
    parts = [host_aggregate(plain_file, quals, AGGS, by=hash_by(keys, bits, g), batches=r)
             for r, g in (((0, 3), 2000), ((3, 3), 1), ((3, 6), 4000))]
    assert parts[1].rows == 0 and parts[1].keys == [] and parts[1].key_columns is not None
    spec = parts[0]._found.spec
    assert spec == full._found.spec and [c.nullable for c in spec.comps] == [False, False, True, True]
    assert all(t[3] is not None for t in parts[0].keys) and any(t[3] is None for t in parts[2].keys)
    got = parts[0].merge(parts[1]).merge(parts[2])
    assert got.rows == full.rows
    same_results(got, full)
    check(got, "one", qual_lists()[1][2], keys)
    with pytest.raises(ValueError):                   # other components
        full.merge(host_aggregate(plain_file, quals, AGGS, by=hash_by(*KEY_LISTS[0])))
    with pytest.raises(ValueError):                   # the same columns, packed differently
        k3 = KEY_LISTS[2][0]
        host_aggregate(plain_file, quals, AGGS, by=hash_by(*KEY_LISTS[2])).merge(
            host_aggregate(plain_file, quals, AGGS, by=hash_by(k3, {"k64": 41, "klate": 8})))
    with pytest.raises(ValueError):                   # composite with plain
        host_aggregate(plain_file, quals, AGGS, by=HashBy(["k32"])).merge(
            host_aggregate(plain_file, quals, AGGS, by=HashBy("k32")))


def test_groups_limit(plain_file):
    from multikeygen import few_groups
    from nvme_strom_amd.models.arrow_scan import host_aggregate
    keys, bits = KEY_LISTS[0]
    n = few_groups(table(), keys)
    aggs = [("count", None), ("sum", "f64")]
    out = host_aggregate(plain_file, [], aggs, by=hash_by(keys, bits, n))
    assert len(out.keys) == n
    with pytest.raises(RuntimeError, match=rf"k16.*kd.*groups={n - 1}\b.*\b{n} distinct"):
        host_aggregate(plain_file, [], aggs, by=hash_by(keys, bits, n - 1))


def test_errors(plain_file):
    """Every refusal: at construction, or against the schema before any
    buffer is read."""
    from nvme_strom_amd.models.arrow_scan import HashBy, Join, host_aggregate
    tbl = table()
    _, _, _, dim = _dim(tbl)
    _, _, _, dim2 = _dim(tbl)
    aggs = [("count", None)]
    run = lambda by, **kw: host_aggregate(plain_file, [], aggs, by=by, **kw)
    with pytest.raises(NotImplementedError, match="four|4"):
        HashBy(["k32", "k16", "kd", "ku8", "ku32"])
    with pytest.raises(NotImplementedError, match=r"k64: 65.*k32: 33.*bits="):
        run(HashBy(["k64", "k32"]))
    for col in ("f64", "s", "b", "dec", "dict"):
        with pytest.raises(NotImplementedError, match=col):
            run(HashBy(["k16", col]))
    with pytest.raises(ValueError, match="twice"):
        HashBy(["k16", "kd", "k16"])
    with pytest.raises(ValueError, match="twice"):
        HashBy([dim["cat"], "kd", dim["cat"]])
    for b in (0, -1, 65, 2.5):
        with pytest.raises(ValueError, match="bits"):
            HashBy(["k16", "kd"], bits={"k16": b})
    with pytest.raises(ValueError, match="bits=17"):
        run(HashBy(["k16", "kd"], bits={"k16": 17}))
    with pytest.raises(ValueError, match="k32"):
        HashBy(["k16", "kd"], bits={"k32": 8})
    with pytest.raises(ValueError, match="bits"):
        HashBy("k16", bits={"k16": 8})
    with pytest.raises(ValueError):
        HashBy([])
    with pytest.raises(ValueError, match="nope"):
        run(HashBy(["k16", "nope"]))
    with pytest.raises(ValueError, match="join="):
        run(HashBy([dim["cat"], "kd"]))
    with pytest.raises(ValueError, match="anti"):
        run(HashBy([dim["cat"], "kd"]), join=Join("i64", dim, "anti"))
    with pytest.raises(ValueError, match="another JoinTable"):
        run(HashBy([dim2["cat"], "kd"]), join=Join("i64", dim))
    with pytest.raises(NotImplementedError, match="one JoinTable attribute"):
        HashBy([dim["cat"], dim["reg"]])
    # a plain str keeps its path
    assert HashBy("k16").comps is None and HashBy(("k16",)).comps == ["k16"]


def test_value_outside_declared_bits(plain_file):
    from nvme_strom_amd.models.arrow_scan import HashBy, host_aggregate
    import pyarrow.compute as pc
    tbl = table()
    k64 = tbl.column("k64").combine_chunks()
    n = pc.sum(pc.or_(pc.less(k64, -2**19), pc.greater_equal(k64, 2**19))).as_py()
    assert n > 100
    with pytest.raises(RuntimeError, match=rf"k64.*bits=20\b.*\b{n} selected row"):
        host_aggregate(plain_file, [], [("count", None)], by=HashBy(["ku8", "k64"], bits={"k64": 20}))
    # a qualifier that removes those rows removes the error
    from nvme_strom_amd.ops.colpred import P
    out = host_aggregate(plain_file, [P("k64").between(-2**19, 2**19 - 1)], [("count", None)],
                         by=HashBy(["ku8", "k64"], bits={"k64": 20}))
    assert out.selected > 0 and all(-2**19 <= t[1] < 2**19 for t in out.keys)
