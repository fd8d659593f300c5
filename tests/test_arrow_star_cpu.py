"""The star join of the Arrow scan on the CPU: coljoin's host_probe_star
against host_probe chained leg by leg and against a brute-force set lookup,
and host_scan_where / host_aggregate / host_top with ``join=StarJoin(...)``
against pyarrow's Table.join chained leg by leg."""
import itertools
import os
import sys

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")

sys.path.insert(0, os.path.dirname(__file__))

from nvme_strom_amd.ops import coljoin as J  # noqa: E402

import stargen as S  # noqa: E402


# ------------------------------------------------------------------ the twin
def payloads(keys: np.ndarray, leg: int) -> np.ndarray:
    return ((np.arange(len(keys)) * 7 + leg) % 1000).astype(np.int32)


def twin_run(c):
    """host_probe_star over a stargen case with prefilled code buffers."""
    tabs = [J.host_build(k, payloads(k, i)) for i, k in enumerate(c["keys"])]
    nout = max(c["kouts"]) + 1
    pre = [[np.full(n, S.PREFILL, np.int32) for n in S.BATCH_ROWS] for _ in range(nout)]
    legs = [(t, h, ko) for t, h, ko in zip(tabs, c["hows"], c["kouts"])]
    dst, codes = J.host_probe_star(legs, c["fks"], c["src"], pre if nout else None)
    assert all((p == S.PREFILL).all() for tab in pre for p in tab)     # the prefill is copied
    return tabs, dst, codes


def test_twin_star_against_chain_and_sets():
    cases = S.star_cases()
    assert {len(c["keys"]) for c in cases} == {1, 2, 3, 4}
    assert {t for c in cases for t in c["tables"]} == {"0", "1", "2", "37", "5000", "chain", "wrap"}
    assert {v.dtype.str[1:] for c in cases for leg in c["fks"] for v, _ in leg} == set(S.DTYPES)
    for c in cases:
        tabs, dst, codes = twin_run(c)
        # host_probe leg by leg, in place
        cur = c["src"]
        for t, fk, how in zip(tabs, c["fks"], c["hows"]):
            cur, _ = J.host_probe(t, fk, cur, how)
        assert np.array_equal(dst, cur), c["label"]
        for t, fk, ko in zip(tabs, c["fks"], c["kouts"]):
            if ko >= 0:
                # a semi leg's codes on the rows of the destination
                pre = [np.full(n, S.PREFILL, np.int32) for n in S.BATCH_ROWS]
                _, want = J.host_probe(t, fk, dst, "semi", pre)
                for a, b in zip(codes[ko], want):
                    assert np.array_equal(a, b), c["label"]
        # a set per table
        have = [{int(k): int(p) for k, p in zip(keys, payloads(keys, i))}
                for i, keys in enumerate(c["keys"])]
        w0 = 0
        for b, n in enumerate(S.BATCH_ROWS):
            keep = S.unpack(c["src"], w0, n)
            for i, how in enumerate(c["hows"]):
                v, ok = c["fks"][i][b]
                m = np.array([(ok is None or bool(ok[r])) and int(v[r]) in have[i]
                              for r in range(n)], bool)
                keep = keep & (m if how == "semi" else ~m)
            assert np.array_equal(S.unpack(dst, w0, n), keep), (c["label"], b)
            tail = np.unpackbits(dst[w0:w0 + (n + 63) // 64].view(np.uint8), bitorder="little")[n:]
            assert not tail.any(), (c["label"], b)
            for i, ko in enumerate(c["kouts"]):
                if ko >= 0:
                    v = c["fks"][i][b][0]
                    want = np.array([have[i][int(v[r])] if keep[r] else S.PREFILL
                                     for r in range(n)], np.int32)
                    assert np.array_equal(codes[ko][b], want), (c["label"], b, i)
            w0 += (n + 63) // 64
    # the cases are not all empty
    assert sum(int(twin_run(c)[1].any()) for c in cases) > len(cases) // 3


def test_twin_star_refusals():
    t = J.host_build(np.arange(5))
    fk = [[(np.arange(4), None)]]
    src = np.array([0xF], np.uint64)
    pre = [[np.zeros(4, np.int32)]]
    with pytest.raises(ValueError, match="legs"):
        J.host_probe_star([], [], src)
    with pytest.raises(ValueError, match="legs"):
        J.host_probe_star([(t, "semi", -1)] * 5, fk * 5, src)
    with pytest.raises(ValueError, match="anti"):
        J.host_probe_star([(t, "anti", 0)], fk, src, pre)
    with pytest.raises(ValueError, match="kout"):
        J.host_probe_star([(t, "semi", 0), (t, "semi", 0)], fk * 2, src, pre)
    with pytest.raises(ValueError, match="kout"):
        J.host_probe_star([(t, "semi", 1)], fk, src, pre)
    with pytest.raises(ValueError, match="fk_batches"):
        J.host_probe_star([(t, "semi", -1)], fk * 2, src)
    dst, out = J.host_probe_star([(t, J.SEMI, None), (t, J.ANTI, None)], fk * 2, src)
    assert out is None and not dst.any()                # nothing is in a table and out of it


# ------------------------------------------------------------------ host scans
@pytest.fixture(scope="module")
def star(tmp_path_factory):
    from arrowgen import write
    from nvme_strom_amd.models.arrow_scan import JoinTable
    tbl = S.table()
    d = tmp_path_factory.mktemp("starcpu")
    paths = {}
    for codec in (None, "lz4", "zstd"):
        paths[codec] = str(d / f"star_{codec}.arrow")
        write(paths[codec], tbl, codec, batch_rows=1000)
    dims = S.dimensions(tbl)
    jt = {fk: JoinTable(keys, attrs=attrs) for fk, (keys, attrs) in dims.items()}
    return tbl, paths, dims, jt


def quals_and_mask():
    import pyarrow.compute as pc
    from nvme_strom_amd.ops.colpred import P
    return [([], lambda t: t),
            ([P("x") > 0.3], lambda t: t.filter(pc.greater(t.column("x"), 0.3)))]


MIXES = [(("f64", "semi"), ("f32", "semi")),
         (("f32", "anti"), ("f16", "semi"), ("f8", "semi")),
         (("f8", "semi"), ("f64", "anti"), ("f16", "anti"), ("f32", "semi")),
         (("f16", "anti"),)]


@pytest.mark.parametrize("codec", [None, "lz4", "zstd"])
def test_host_scan_where_star_matches_pyarrow(star, codec):
    from nvme_strom_amd.models.arrow_scan import Join, StarJoin, host_scan_where
    tbl, paths, dims, jt = star
    for legs in MIXES:
        sj = StarJoin(*[Join(fk, jt[fk], how) for fk, how in legs])
        for q, mf in quals_and_mask():
            want = S.ids(mf(S.reference(tbl, dims, legs)))
            assert 0 < len(want) < tbl.num_rows, legs
            out = host_scan_where(paths[codec], q, join=sj)
            assert out.rows == tbl.num_rows and np.array_equal(out.indices, want), legs
    # an attribute of the third leg, gathered per selected row
    legs = (("f32", "anti"), ("f8", "semi"), ("f16", "semi"))
    sj = StarJoin(*[Join(fk, jt[fk], how) for fk, how in legs])
    for q, mf in quals_and_mask():
        ref = mf(S.reference(tbl, dims, legs, [("f16", "cat", "c_cat")]))
        out = host_scan_where(paths[codec], q, project=jt["f16"]["cat"], join=sj)
        assert np.array_equal(out.indices, S.ids(ref)) and out.values.dtype == np.int32
        assert [out.dictionary[c] for c in out.values.tolist()] == ref.column("c_cat").to_pylist()
    # an ordinary column projected under a star join
    out = host_scan_where(paths[codec], [], project="k16", join=sj)
    ref = S.reference(tbl, dims, legs)
    assert np.array_equal(out.values, np.asarray(ref.column("k16").combine_chunks()))


@pytest.mark.parametrize("codec", [None, "lz4", "zstd"])
def test_host_aggregate_star_matches_pyarrow(star, codec):
    from nvme_strom_amd.models.arrow_scan import HashBy, Join, StarJoin, host_aggregate
    tbl, paths, dims, jt = star
    legs = (("f64", "semi"), ("f32", "semi"), ("f16", "semi"), ("f8", "anti"))
    sj = StarJoin(*[Join(fk, jt[fk], how) for fk, how in legs])
    attrs = [("f64", "cat", "a_cat"), ("f32", "reg", "b_reg"), ("f16", "cat", "c_cat")]
    for q, mf in quals_and_mask():
        ref = mf(S.reference(tbl, dims, legs, attrs))
        assert ref.num_rows > 50
        out = host_aggregate(paths[codec], q, S.AGGS, by=jt["f32"]["reg"], join=sj)
        assert out.by == "reg" and out.rows == tbl.num_rows
        S.check_agg(out, ref, ["b_reg"])
        hb = HashBy([jt["f64"]["cat"], jt["f16"]["cat"], "k16"], groups=1 << 12)
        out = host_aggregate(paths[codec], q, S.AGGS, by=hb, join=sj)
        # two attributes called cat: qualified by their place in the key
        assert out.by == ("cat[0]", "cat[1]", "k16") and out._spec.keyspec.names == list(out.by)
        S.check_agg(out, ref, ["a_cat", "c_cat", "k16"])
        assert out.keys == sorted(out.keys, key=lambda k: (
            jt["f64"]["cat"].values.index(k[0]), jt["f16"]["cat"].values.index(k[1]), k[2]))
        out = host_aggregate(paths[codec], q, S.AGGS, join=sj)
        S.check_agg(out, ref)
        # the fact table's own key column under a star join
        out = host_aggregate(paths[codec], q, S.AGGS, by=HashBy("k16"), join=sj)
        S.check_agg(out, ref, ["k16"])


@pytest.mark.parametrize("codec", [None, "lz4", "zstd"])
def test_host_top_star_matches_pyarrow(star, codec):
    from nvme_strom_amd.models.arrow_scan import Join, StarJoin, host_top
    tbl, paths, dims, jt = star
    legs = (("f16", "anti"), ("f32", "semi"), ("f8", "semi"))
    sj = StarJoin(*[Join(fk, jt[fk], how) for fk, how in legs])
    for q, mf in quals_and_mask():
        ref = mf(S.reference(tbl, dims, legs, [("f32", "reg", "b_reg")]))
        for desc in (False, True):
            out = host_top(paths[codec], q, "m64", 40, desc, project=jt["f32"]["reg"], join=sj)
            S.check_top(out, ref, "m64", 40, desc, "b_reg")
            out = host_top(paths[codec], q, "m64", 7, desc, join=sj)
            S.check_top(out, ref, "m64", 7, desc)


def test_star_leg_order_single_leg_and_merge(star):
    from nvme_strom_amd.models.arrow_scan import (HashBy, Join, StarJoin, host_aggregate,
                                                  host_scan_where, host_top)
    tbl, paths, dims, jt = star
    path = paths["lz4"]
    legs = [Join("f64", jt["f64"]), Join("f32", jt["f32"], "anti"), Join("f16", jt["f16"]),
            Join("f8", jt["f8"])]
    hb = HashBy([jt["f16"]["cat"], jt["f8"]["kind"], "k16"], groups=4096)
    base = host_scan_where(path, [], join=StarJoin(*legs)).indices
    agg0 = host_aggregate(path, [], S.AGGS, by=hb, join=StarJoin(*legs))
    assert 0 < len(base) < tbl.num_rows
    for perm in itertools.permutations(range(4)):
        sj = StarJoin(*[legs[i] for i in perm])
        assert np.array_equal(host_scan_where(path, [], join=sj).indices, base), perm
    for perm in ((3, 2, 1, 0), (1, 3, 0, 2)):
        out = host_aggregate(path, [], S.AGGS, by=hb, join=StarJoin(*[legs[i] for i in perm]))
        assert out.keys == agg0.keys and np.array_equal(out.count_all, agg0.count_all)
        assert all(np.array_equal(a, b) for a, b in zip(out.values, agg0.values))
    # the same fk column and the same JoinTable in two legs
    twice = StarJoin(Join("f64", jt["f64"]), Join("f64", jt["f64"]))
    assert np.array_equal(host_scan_where(path, [], join=twice).indices,
                          host_scan_where(path, [], join=Join("f64", jt["f64"])).indices)
    none = StarJoin(Join("f64", jt["f64"]), Join("f64", jt["f64"], "anti"))
    assert len(host_scan_where(path, [], join=none).indices) == 0
    # one leg: what join=Join gives
    for j in (legs[0], legs[1]):
        a = host_scan_where(path, [], join=StarJoin(j))
        b = host_scan_where(path, [], join=j)
        assert np.array_equal(a.indices, b.indices)
    a = host_aggregate(path, [], S.AGGS, by=jt["f64"]["cat"], join=StarJoin(legs[0]))
    b = host_aggregate(path, [], S.AGGS, by=jt["f64"]["cat"], join=legs[0])
    assert a.keys == b.keys and all(np.array_equal(x, y) for x, y in zip(a.values, b.values))
    a = host_top(path, [], "m64", 9, project=jt["f64"]["reg"], join=StarJoin(legs[0]))
    b = host_top(path, [], "m64", 9, project=jt["f64"]["reg"], join=legs[0])
    assert np.array_equal(a.rows, b.rows) and np.array_equal(a.projected, b.projected)
    # batch ranges merge to the whole
    sj = StarJoin(*legs)
    parts = [host_aggregate(path, [], S.AGGS, by=hb, join=sj, batches=r)
             for r in ((0, 2), (2, 6))]
    m = parts[0].merge(parts[1])
    assert m.keys == agg0.keys and np.array_equal(m.count_all, agg0.count_all)
    assert all(np.array_equal(a, b) for a, b in zip(m.values, agg0.values))
    parts = [host_aggregate(path, [], S.AGGS, by=jt["f8"]["kind"], join=sj, batches=r)
             for r in ((0, 3), (3, 6))]
    whole = host_aggregate(path, [], S.AGGS, by=jt["f8"]["kind"], join=sj)
    m = parts[0].merge(parts[1])
    assert m.keys == whole.keys and np.array_equal(m.count_all, whole.count_all)
    tops = [host_top(path, [], "m64", 25, True, project=jt["f16"]["cat"], join=sj, batches=r)
            for r in ((0, 4), (4, 6))]
    whole = host_top(path, [], "m64", 25, True, project=jt["f16"]["cat"], join=sj)
    m = tops[0].merge(tops[1])
    assert np.array_equal(m.rows, whole.rows) and np.array_equal(m.projected, whole.projected)


def test_star_refusals(star):
    from nvme_strom_amd.models.arrow_scan import (HashBy, Join, JoinTable, StarJoin,
                                                  host_aggregate, host_scan_where, host_top)
    tbl, paths, dims, jt = star
    path = paths[None]
    aggs = [("count", None)]
    a, b, c, d = (jt[fk] for fk in S.FKS)
    with pytest.raises(ValueError, match="at least one"):
        StarJoin()
    with pytest.raises(NotImplementedError, match="at most 4"):
        StarJoin(*[Join("f8", d)] * 5)
    with pytest.raises(TypeError):
        StarJoin(Join("f8", d), "f64")
    # the two pinned refusals
    with pytest.raises(NotImplementedError, match="one join"):
        host_scan_where(path, [], join=[Join("f64", a), Join("f32", b)])
    with pytest.raises(NotImplementedError, match="one JoinTable attribute"):
        HashBy([a["cat"], a["reg"]])
    # a StarJoin inside a list is a list all the same
    with pytest.raises(NotImplementedError, match="one join"):
        host_aggregate(path, [], aggs, join=(StarJoin(Join("f64", a)),))
    sj = StarJoin(Join("f64", a), Join("f32", b, "anti"), Join("f16", c))
    # an attribute needs its table in exactly one leg, and that a semi leg
    other = JoinTable(np.arange(10), attrs={"cat": list("abcdefghij")})
    for run in (lambda at: host_scan_where(path, [], project=at, join=sj),
                lambda at: host_aggregate(path, [], aggs, by=at, join=sj),
                lambda at: host_aggregate(path, [], aggs, by=HashBy([at, "k16"]), join=sj),
                lambda at: host_top(path, [], "m64", 3, project=at, join=sj)):
        with pytest.raises(ValueError, match="another JoinTable"):
            run(other["cat"])
        with pytest.raises(ValueError, match="another JoinTable"):
            run(d["kind"])
        with pytest.raises(ValueError, match="anti"):
            run(b["reg"])
    with pytest.raises(ValueError, match="needs join"):
        host_aggregate(path, [], aggs, by=HashBy([a["cat"], c["cat"]]))
    twice = StarJoin(Join("f64", a), Join("f16", c), Join("f64", a, "anti"))
    with pytest.raises(ValueError, match="ambiguous"):
        host_aggregate(path, [], aggs, by=a["cat"], join=twice)
    with pytest.raises(ValueError, match="ambiguous"):
        host_scan_where(path, [], project=a["reg"], join=twice)
    host_aggregate(path, [], aggs, by=c["cat"], join=twice)       # the other leg's is not
    # a plain Join carries one table: the second attribute is another table's
    with pytest.raises(ValueError, match="another JoinTable"):
        host_aggregate(path, [], aggs, by=HashBy([a["cat"], c["cat"]]), join=Join("f64", a))
    # still four components and 64 bits
    with pytest.raises(NotImplementedError, match="at most"):
        HashBy([a["cat"], b["reg"], c["cat"], d["kind"], "k16"])
    with pytest.raises(NotImplementedError, match="64"):
        host_aggregate(path, [], aggs, by=HashBy([a["cat"], c["cat"], "m64"]), join=sj)
    # the legs' columns are checked like a Join's
    with pytest.raises(ValueError, match="no column"):
        host_scan_where(path, [], join=StarJoin(Join("f64", a), Join("nope", b)))
    with pytest.raises(NotImplementedError, match="x"):
        host_scan_where(path, [], join=StarJoin(Join("f64", a), Join("x", b)))
    with pytest.raises(TypeError):
        host_scan_where(path, [], join="f64")
