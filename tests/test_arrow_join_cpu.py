"""The hash join of the Arrow scan on the CPU: the coljoin twin against a
Python dict, and host_scan_where / host_aggregate with ``join=`` against
pyarrow's Table.join (+ group_by)."""
import os
import sys

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")

sys.path.insert(0, os.path.dirname(__file__))

from nvme_strom_amd.ops import coljoin as J  # noqa: E402


# ------------------------------------------------------------------ the twin
def test_capacity_and_hash():
    assert [J.capacity(n) for n in (0, 1, 32, 33, 200, 256, 257, 5000)] == \
        [64, 64, 64, 128, 512, 512, 1024, 16384]
    # murmur3 fmix64: 0 is its fixed point, and it is a bijection on the samples
    assert int(J.hash64([0])[0]) == 0
    h = J.hash64(np.arange(-5000, 5000))
    assert len(np.unique(h)) == 10000 and h.dtype == np.uint64


def test_twin_build_and_probe_against_dict():
    from joingen import SPECIAL, key_sets, probe_values
    for label, keys in key_sets():
        t = J.host_build(keys)
        want = {int(k): i for i, k in enumerate(keys)}
        assert t.capacity == J.capacity(len(keys)) and t.nkeys == len(keys) and t.dups == 0, label
        assert t.items() == want, label
        # the displacement bound is tight: it is the true largest displacement,
        # and probing every key needs no more steps than it allows
        assert t.maxdisp == t.true_maxdisp(), label
        m, pay = J.host_lookup(t, keys)
        assert m.all() and pay.tolist() == list(range(len(keys))), label
        v = np.concatenate([probe_values(keys, 500, seed=len(keys)), np.array(SPECIAL, np.int64)])
        m, pay = J.host_lookup(t, v)
        assert m.tolist() == [int(x) in want for x in v], label
        assert pay[m].tolist() == [want[int(x)] for x in v[m]], label
        # rows that are not active are not probed
        act = np.arange(len(v)) % 3 == 0
        m2, _ = J.host_lookup(t, v, act)
        assert np.array_equal(m2, m & act), label
        # a payload per key instead of the build row
        codes = (np.arange(len(keys)) % 7).astype(np.int32)
        t2 = J.host_build(keys, codes)
        m, pay = J.host_lookup(t2, keys)
        assert m.all() and np.array_equal(pay, codes), label


def test_twin_chain_and_wraparound_shapes():
    from joingen import key_sets
    sets = dict(key_sets())
    t = J.host_build(sets["chain"])
    assert t.capacity == 512 and t.maxdisp == 199
    home = J.hash64(sets["chain"]) & np.uint64(511)
    assert (home == np.uint64(300)).all()
    t = J.host_build(sets["wrap"])
    assert t.capacity == 64
    used = np.flatnonzero(t.slots[:, 0] != J.EMPTY)
    assert used.tolist() == list(range(0, 10)) + [62, 63]      # past the last slot: slot 0 on
    assert 9 <= t.maxdisp == t.true_maxdisp() <= 11 and J.host_lookup(t, sets["wrap"])[0].all()


def test_twin_probe_words_and_key_output():
    """host_probe: tail words, validity, unselected rows, garbage bits beyond
    a batch, anti-join keeping null keys, the key output's untouched rows."""
    from joingen import key_sets, probe_values
    keys = dict(key_sets())["37"]
    t = J.host_build(keys, (np.arange(37) % 5).astype(np.int32))
    rng = np.random.default_rng(2)
    rows = [1, 63, 64, 65, 200]
    batches, sel = [], []
    for n in rows:
        batches.append((probe_values(keys, n, seed=n), rng.random(n) < 0.8))
        sel.append(rng.random(n) < 0.6)
    words = []
    for n, s in zip(rows, sel):
        bits = np.ones(((n + 63) // 64) * 64, np.uint8)         # garbage beyond the rows
        bits[:n] = s
        words.append(np.packbits(bits, bitorder="little").view(np.uint64))
    src = np.concatenate(words)
    pre = [np.full(n, -77, np.int32) for n in rows]
    semi, kout = J.host_probe(t, batches, src, "semi", pre)
    anti, _ = J.host_probe(t, batches, src, "anti")
    w0 = 0
    have = {int(k): i % 5 for i, k in enumerate(keys)}
    for b, n in enumerate(rows):
        nw = (n + 63) // 64
        v, ok = batches[b]
        m = np.array([ok[i] and int(v[i]) in have for i in range(n)])
        unpack = lambda w: np.unpackbits(w[w0:w0 + nw].view(np.uint8), bitorder="little")
        s, a = unpack(semi), unpack(anti)
        assert np.array_equal(s[:n].astype(bool), sel[b] & m) and not s[n:].any()
        assert np.array_equal(a[:n].astype(bool), sel[b] & ~m) and not a[n:].any()
        want = np.where(sel[b] & m, [have.get(int(x), 0) for x in v], -77)
        assert np.array_equal(kout[b], want)
        assert (pre[b] == -77).all()                            # the prefill is copied
        w0 += nw
    with pytest.raises(ValueError):
        J.host_probe(t, batches, src, "anti", pre)


def test_twin_unsigned_and_narrow_keys():
    t = J.host_build(np.array([0, 5, 200, -1, 2**31, 2**63 - 1], np.int64))
    u8 = np.array([0, 5, 2**63 - 1, 2**63, 2**64 - 1], np.uint64)
    k, can = J.widen(u8)
    assert can.tolist() == [True, True, True, False, False]
    assert J.host_lookup(t, k, can)[0].tolist() == [True, True, True, False, False]
    for dt, vals, want in (("i1", [-1, 5, 100], [True, True, False]),
                           ("u1", [255, 200, 5], [False, True, True]),
                           ("u4", [2**31, 2**32 - 1], [True, False]),
                           ("i4", [-1, 5], [True, True])):
        k, can = J.widen(np.array(vals, dt))
        assert can.all() and J.host_lookup(t, k)[0].tolist() == want, dt
    with pytest.raises(NotImplementedError):
        J.widen(np.zeros(3, np.float32))


def test_twin_duplicates_are_counted():
    t = J.host_build(np.array([5, 9, 5, -(1 << 63), 9, 5, -(1 << 63)], np.int64))
    assert t.nkeys == 3 and t.dups == 4
    assert set(t.items()) == {5, 9, -(1 << 63)}


# ------------------------------------------------------------------ JoinTable
def test_join_table():
    from nvme_strom_amd.models.arrow_scan import Join, JoinTable
    with pytest.raises(ValueError, match="duplicate"):
        JoinTable(np.array([1, 2, 3, 2]))
    with pytest.raises(ValueError, match="integer"):
        JoinTable(np.array([1.0, 2.0]))
    with pytest.raises(ValueError, match="2\\^63"):
        JoinTable(np.array([1, 2**63], np.uint64))
    with pytest.raises(ValueError, match="values for"):
        JoinTable(np.array([1, 2]), attrs={"a": ["x"]})
    # null keys are dropped with their attribute values; a null attribute
    # value is one ordinary code whose value is None
    dim = JoinTable(pa.array([10, None, 30, 40, None, 60]),
                    attrs={"c": ["x", "gone", None, "x", "gone", None],
                           "n": pa.array([7, 0, 8, 7, 0, 9]),
                           "f": [True, None, False, False, None, True]})
    assert len(dim) == 4 and dim.keys.tolist() == [10, 30, 40, 60]
    assert dim["c"].values == ["x", None] and dim["c"].codes.tolist() == [0, 1, 0, 1]
    assert dim["n"].values == [7, 8, 9] and dim["n"].codes.tolist() == [0, 1, 0, 2]
    assert dim["f"].values == [True, False] and dim["f"].codes.tolist() == [0, 1, 1, 0]
    assert dim.host().nkeys == 4
    with pytest.raises(ValueError, match="no attribute"):
        dim["nope"]
    with pytest.raises(ValueError, match="how"):
        Join("fk", dim, how="outer")
    empty = JoinTable(np.zeros(0, np.int32), attrs={"c": []})
    assert len(empty) == 0 and empty["c"].values == [] and empty.host().nkeys == 0
    dim.close()


# ------------------------------------------------------------------ host scans
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from arrowgen import table, write
    tbl = table(3000)
    d = tmp_path_factory.mktemp("joincpu")
    paths = {}
    for codec in (None, "lz4", "zstd"):
        paths[codec] = str(d / f"t_{codec}.arrow")
        write(paths[codec], tbl, codec)
    return tbl, paths


@pytest.mark.parametrize("codec", [None, "lz4", "zstd"])
def test_host_scan_where_join_matches_pyarrow(files, codec):
    import pyarrow.compute as pc
    from joingen import dimension, joined, joined_ids
    from nvme_strom_amd.models.arrow_scan import Join, JoinTable, host_scan_where
    from nvme_strom_amd.ops.colpred import P
    tbl, paths = files
    quals = [P("f64") > 0.4]
    mask = lambda t: pc.greater(t.column("f64").combine_chunks(), 0.4)
    for fk in ("i64", "u32"):
        keys, cats, regs = dimension(tbl.column(fk).combine_chunks())
        dim = JoinTable(keys, attrs={"category": cats, "region": regs})
        for how in ("semi", "anti"):
            for q, mf in ((quals, mask), ([], None)):
                out = host_scan_where(paths[codec], q, join=Join(fk, dim, how=how))
                want = joined_ids(tbl, fk, keys, how, mf)
                assert 0 < len(want) < tbl.num_rows
                assert np.array_equal(out.indices, want), (fk, how, bool(q))
        # the anti-join keeps the null keys, the semi-join drops them
        if tbl.column(fk).null_count:
            nulls = np.flatnonzero(~np.asarray(tbl.column(fk).combine_chunks().is_valid()))
            anti = host_scan_where(paths[codec], [], join=Join(fk, dim, how="anti")).indices
            semi = host_scan_where(paths[codec], [], join=Join(fk, dim)).indices
            assert np.isin(nulls, anti).all() and not np.isin(nulls, semi).any()
        # the joined attribute per selected row
        for attr, vals in (("category", cats), ("region", regs.tolist())):
            out = host_scan_where(paths[codec], quals, project=dim[attr], join=Join(fk, dim))
            ref = joined(tbl, fk, keys, {attr: vals}, "inner")
            ref = ref.filter(mask(ref).fill_null(False)).sort_by("__id")
            assert np.array_equal(out.indices, np.asarray(ref.column("__id").combine_chunks()))
            assert [out.dictionary[c] for c in out.values.tolist()] == ref.column(attr).to_pylist()
            assert out.valid is None and out.values.dtype == np.int32
    # an empty dimension: the semi-join selects nothing, the anti-join everything
    empty = JoinTable(np.zeros(0, np.int64))
    assert len(host_scan_where(paths[codec], [], join=Join("i64", empty)).indices) == 0
    assert np.array_equal(host_scan_where(paths[codec], [], join=Join("i64", empty, "anti")).indices,
                          np.arange(tbl.num_rows))


from agggen import AGGS as JOIN_AGGS  # noqa: E402


@pytest.mark.parametrize("codec", [None, "lz4", "zstd"])
def test_host_aggregate_join_matches_pyarrow(files, codec):
    from agggen import check, qual_lists
    from joingen import dimension, joined
    from nvme_strom_amd.models.arrow_scan import Join, JoinTable, host_aggregate
    tbl, paths = files
    for fk in ("i64", "u32"):
        keys, cats, regs = dimension(tbl.column(fk).combine_chunks())
        dim = JoinTable(keys, attrs={"category": cats, "region": regs})
        ref = joined(tbl, fk, keys, {"category": cats, "region": regs.tolist()}, "inner")
        for label, quals, mask in qual_lists()[:3]:
            out = host_aggregate(paths[codec], quals, JOIN_AGGS, by=dim["category"],
                                 join=Join(fk, dim))
            assert out.rows == tbl.num_rows and out.by == "category"
            check(out, ref, mask, "category", JOIN_AGGS)
            if label == "all":
                assert None in out.keys                      # the null attribute's group
            out = host_aggregate(paths[codec], quals, JOIN_AGGS, by=dim["region"],
                                 join=Join(fk, dim))
            check(out, ref, mask, "region", JOIN_AGGS)
            # a join without an attribute: the joined rows as one group
            out = host_aggregate(paths[codec], quals, JOIN_AGGS, join=Join(fk, dim))
            check(out, ref, mask, None, JOIN_AGGS)
        # the fact table's own key still works under a join
        out = host_aggregate(paths[codec], [], JOIN_AGGS, by="b", join=Join(fk, dim))
        check(out, ref, None, "b", JOIN_AGGS)
    # batch ranges merge; results over different attributes do not
    dim2 = JoinTable(keys, attrs={"category": cats[::-1]})
    parts = [host_aggregate(paths[codec], [], JOIN_AGGS, by=dim["category"], join=Join("u32", dim),
                            batches=r) for r in ((0, 2), (2, 5))]
    check(parts[0].merge(parts[1]), ref, None, "category", JOIN_AGGS)
    other = host_aggregate(paths[codec], [], JOIN_AGGS, by=dim2["category"],
                           join=Join("u32", dim2), batches=(2, 5))
    if other._spec.keyvals != parts[0]._spec.keyvals:
        with pytest.raises(ValueError, match="merge"):
            parts[0].merge(other)
    plain = host_aggregate(paths[codec], [], JOIN_AGGS, by="dict", batches=(2, 5))
    with pytest.raises(ValueError, match="merge"):
        parts[0].merge(plain)


def test_join_refusals(files):
    from nvme_strom_amd.models.arrow_scan import Join, JoinTable, host_aggregate, host_scan_where
    tbl, paths = files
    path = paths[None]
    dim = JoinTable(np.arange(10), attrs={"c": list("abcdefghij")})
    other = JoinTable(np.arange(10), attrs={"c": list("abcdefghij")})
    aggs = [("count", None)]
    for col in ("f64", "f32", "s", "b", "dec", "dict", "idict", "ts"):
        with pytest.raises(NotImplementedError, match=col):
            host_scan_where(path, [], join=Join(col, dim))
        with pytest.raises(NotImplementedError, match=col):
            host_aggregate(path, [], aggs, join=Join(col, dim))
    with pytest.raises(ValueError, match="no column"):
        host_scan_where(path, [], join=Join("nope", dim))
    with pytest.raises(ValueError, match="no column"):
        host_scan_where(path, [("nope", 0, 1)])
    with pytest.raises(NotImplementedError, match="one join"):
        host_scan_where(path, [], join=[Join("i64", dim), Join("u32", dim)])
    with pytest.raises(NotImplementedError, match="one join"):
        host_aggregate(path, [], aggs, join=[Join("i64", dim)])
    # an attribute needs its own table's semi-join
    with pytest.raises(ValueError, match="anti"):
        host_aggregate(path, [], aggs, by=dim["c"], join=Join("i64", dim, how="anti"))
    with pytest.raises(ValueError, match="anti"):
        host_scan_where(path, [], project=dim["c"], join=Join("i64", dim, how="anti"))
    with pytest.raises(ValueError, match="another JoinTable"):
        host_aggregate(path, [], aggs, by=other["c"], join=Join("i64", dim))
    with pytest.raises(ValueError, match="another JoinTable"):
        host_scan_where(path, [], project=other["c"], join=Join("i64", dim))
    with pytest.raises(ValueError, match="needs join"):
        host_aggregate(path, [], aggs, by=dim["c"])
    with pytest.raises(ValueError, match="needs join"):
        host_scan_where(path, [], project=dim["c"])
    # without a join an empty qualifier list is still refused, and the limits
    # of GROUP BY and SUM stay where they were
    with pytest.raises(ValueError, match="at least one qualifier"):
        host_scan_where(path, [])
    with pytest.raises(NotImplementedError, match="i64"):
        host_aggregate(path, [], aggs, by="i64")
    with pytest.raises(NotImplementedError, match="i64"):
        host_aggregate(path, [], aggs, by="i64", join=Join("u32", dim))
    with pytest.raises(NotImplementedError, match="dec"):
        host_aggregate(path, [], [("sum", "dec")], join=Join("u32", dim))
    # the Layout limit applies to the attribute's codes
    big = JoinTable(np.arange(9000), attrs={"c": np.arange(9000)})
    with pytest.raises(NotImplementedError, match="64 KiB"):
        host_aggregate(path, [], [("sum", "i64")], by=big["c"], join=Join("u32", big))
