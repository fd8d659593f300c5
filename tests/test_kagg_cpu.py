"""The numpy twins of the aggregate, group and join kernels (ops/colagg.py,
ops/colgroup.py, ops/coljoin.py) against the brute-force reference of
tests/kagggen.py: the twins are the oracle of host_aggregate and of every
whole-scan test, and this pins them — over every value type, every ops mask
1 .. 15, COUNT with and without ALL, the float pools and the batch geometry
of kagggen."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

import kagggen as K  # noqa: E402
from nvme_strom_amd.ops import colagg as A  # noqa: E402
from nvme_strom_amd.ops import colgroup as G  # noqa: E402
from nvme_strom_amd.ops import coljoin as J  # noqa: E402

GEOMS = list(K.GEOMETRIES)


def _bitmaps(case, seed):
    rng = np.random.default_rng(seed)
    return [(p,) + K.bitmap(case.geometry, p, rng) for p in K.BITMAPS]


def _twin_block(case, lay, bits):
    blk = A.new_block(lay)
    for e in range(len(lay.entries)):
        for b, sel in enumerate(bits):
            vb = case.val.batches[b]
            key = None
            if case.key is not None:
                kb = case.key.batches[b]
                key = (np.asarray(kb.values), kb.valid)
            with np.errstate(invalid="ignore"):         # inf - inf is a case
                A.host_agg(lay, blk, e, sel, vb.values, vb.valid, key, count_bad=e == 0)
    return blk


def _check_colagg(case, seed, ents=None, full=True):
    lay = A.Layout(ents or case.entries(), case.nslots, K.KEY_TYPES[case.key_dt] if case.key else 0)
    for p, bits, words in _bitmaps(case, seed):
        ref = K.case_reference(case, bits)
        K.assert_pools(case, ref[0], full and p == 1.0)
        blk = _twin_block(case, lay, bits)
        K.check_block(case, lay, blk, ref, (case.label, p))
        if p == 0.0:
            assert np.array_equal(blk, A.new_block(lay))
    return ref


@pytest.mark.parametrize("geom", GEOMS)
def test_host_agg_flat(geom):
    for i, case in enumerate(K.flat_cases(geom)):
        ref = _check_colagg(case, 100 + i)
        del ref
    for dt in ("i8", "u8"):
        case = next(c for c in K.flat_cases(geom) if c.dt == dt)
        K.assert_wraps(dt, K.case_reference(case, K.bitmap(case.geometry, 1.0,
                                                           np.random.default_rng(0))[0])[0])


@pytest.mark.parametrize("geom", GEOMS)
def test_host_agg_keyed(geom):
    """Every key type and its malformed keys, every value type."""
    for i, case in enumerate(K.keyed_type_cases(geom)):
        _check_colagg(case, 200 + i)
        bits, words = K.bitmap(case.geometry, 1.0, np.random.default_rng(7))
        groups, nbad, _ = K.case_reference(case, bits)
        assert nbad > 0 or case.key_dt == "b1" and case.nslots == 3, case.label
        if case.dt in ("i8", "u8"):
            K.assert_wraps(case.dt, groups)


@pytest.mark.parametrize("geom", GEOMS)
def test_generator_witnesses(geom):
    """The keyed tables contain what they are meant to: one-key words, a
    flush between two of them, a mixed word whose first key repeats and has a
    NaN among its rows, a batch without a valid row, garbage next to the
    last rows of a batch — under the dense and the 50 % bitmap."""
    cases = [c for c in K.keyed_type_cases(geom) if c.key_dt == "i4" and c.dt in K.FLOATS] + \
        [c for c in K.group_cases(geom) if c.key_dt == "i4" and c.dt in K.FLOATS]
    assert len(cases) == 4
    for case in cases:
        gid = K.value_gid if case.label.startswith("group") else None
        for p, bits, words in _bitmaps(case, 31)[:2]:
            _, _, log = K.case_reference(case, bits, gid_of=gid)
            assert K.witnesses(log, case.val, case.geometry, words) == K.WITNESSES, (case.label, p)


def test_replica_rule_and_twin():
    """launch_agg's replica count R and the reduce's lanes L of the pairs
    the GPU test runs: every class once."""
    assert [(K.replicas(*a), K.reduce_lanes(*a)) for a, _ in K.REPLICA_CASES] == \
        [rl for _, rl in K.REPLICA_CASES]
    assert {r for _, (r, _) in K.REPLICA_CASES} == {256, 32, 4, 2, 1}
    assert {l for _, (_, l) in K.REPLICA_CASES} == {64, 8, 4, 2}
    for (ops, nslots), _ in K.REPLICA_CASES:
        for dt in ("f8", "i8"):
            case, ent = K.replica_case(ops, nslots, dt)
            _check_colagg(case, 300 + nslots, [ent], full=nslots <= 40)


def test_big_unkeyed_twin():
    """The shape at which the reduce kernel folds two slabs in one lane."""
    assert K.nwords_of(K.BIG_ROWS) == 1094
    for dt in ("f8", "i8"):
        case = K.big_case(dt)
        rng = np.random.default_rng(41)
        bits, _ = K.bitmap(case.geometry, 0.9, rng)
        lay = A.Layout([A.Entry(15, dt)])
        ref = K.case_reference(case, bits)
        K.check_block(case, lay, _twin_block(case, lay, bits), ref, case.label)
        if dt == "i8":
            K.assert_wraps(dt, ref[0])


# ------------------------------------------------------------ hash GROUP BY
def _twin_groups(case, ents, bits, multi=None):
    with np.errstate(invalid="ignore"):                 # inf - inf is a case
        return _twin_groups_(case, ents, bits, multi)


def _twin_groups_(case, ents, bits, multi):
    unsigned = multi is not None or np.dtype(case.key_dt).kind == "u"
    want = G.empty_groups(ents, unsigned, multi[0] if multi else None)
    for b, sel in enumerate(bits):
        vb, kb = case.val.batches[b], case.key.batches[b]
        cols = [(vb.values, vb.valid)] * len(ents)
        if multi:
            spec, other = multi
            ob = other.batches[b]
            g, misfit = G.host_group_agg_multi(ents, sel, spec, [kb.values, ob.values],
                                               [kb.valid, ob.valid], cols)
            assert not misfit.any()
        else:
            g = G.host_group_agg(ents, sel, kb.values, kb.valid, cols)
        want = G.merge(want, g)
    return want


@pytest.mark.parametrize("geom", GEOMS)
def test_host_group_agg(geom):
    for i, case in enumerate(K.group_cases(geom)):
        ents = case.entries()
        for p, bits, _ in _bitmaps(case, 400 + i):
            groups, nbad, _ = K.case_reference(case, bits, gid_of=K.value_gid)
            assert nbad == 0
            K.assert_pools(case, groups, p == 1.0)
            got = _twin_groups(case, ents, bits)
            K.check_groups([int(k) for k in got.keys], got.layout, got.block, groups,
                           (case.label, p))


@pytest.mark.parametrize("geom", GEOMS)
def test_host_group_agg_multi(geom):
    spec = G.KeySpec(K.MULTI_SPEC)
    for i, dt in enumerate(["f8", "f4", "i8", None]):
        case, kb = K.multi_case(geom, dt, np.random.default_rng(50 + i))
        ents = case.entries()
        for p, bits, _ in _bitmaps(case, 500 + i):
            groups, _, _ = K.case_reference(case, bits, [case.key, kb], lambda k: k)
            K.assert_pools(case, groups, p == 1.0)
            got = _twin_groups(case, ents, bits, (spec, kb))
            K.check_groups(K.multi_keys(spec, got.keys), got.layout, got.block, groups,
                           (case.label, p))


# --------------------------------------------------------------------- join
def _host_table(dim):
    return J.host_build(np.array(list(dim), np.int64), np.array(list(dim.values()), np.int32))


def _batches(t):
    return [(np.asarray(b.values), b.valid) for b in t.batches]


@pytest.mark.parametrize("geom", GEOMS)
def test_host_probe(geom):
    """Semi and anti, with and without key output, every fk type."""
    geometry = K.GEOMETRIES[geom][0]
    for i, fk_dt in enumerate(K.INTS):
        rng = np.random.default_rng(600 + i)
        fk, dim = K.join_fk(geom, fk_dt, rng), K.join_dim(fk_dt)
        t = _host_table(dim)
        assert t.items() == dim                         # negative payloads among them
        for p in K.BITMAPS:
            bits, words = K.bitmap(geometry, p, rng)
            for how in (J.SEMI, J.ANTI):
                keep, pays = K.join_reference(bits, [fk], [dim], [how])
                assert p < 1 or 0 < sum(int(k.sum()) for k in keep) < sum(geometry)
                pre = [np.full(n, K.PREFILL, np.int32) for n in geometry]
                kout = pre if how == J.SEMI else None
                dst, out = J.host_probe(t, _batches(fk), words, "anti" if how else "semi", kout)
                assert np.array_equal(dst, K.pack_bits(geometry, keep)), (fk_dt, p, how)
                if out is not None:
                    for b, n in enumerate(geometry):
                        want = [pays[0][b][r] if keep[b][r] else K.PREFILL for r in range(n)]
                        assert out[b].tolist() == want, (fk_dt, p, b)


@pytest.mark.parametrize("geom", GEOMS)
def test_host_probe_star(geom):
    """Two legs, one semi with key output and one anti, in both orders."""
    geometry = K.GEOMETRIES[geom][0]
    for i, (da, db) in enumerate([("i4", "u8"), ("i8", "u1"), ("u2", "i1")]):
        rng = np.random.default_rng(700 + i)
        fks = [K.join_fk(geom, da, rng), K.join_fk(geom, db, rng)]
        dims = [K.join_dim(da, 0), K.join_dim(db, 1)]
        tabs = [_host_table(d) for d in dims]
        for hows, kouts in (([J.SEMI, J.ANTI], [0, -1]), ([J.ANTI, J.SEMI], [-1, 0])):
            for p in K.BITMAPS:
                bits, words = K.bitmap(geometry, p, rng)
                keep, pays = K.join_reference(bits, fks, dims, hows)
                pre = [[np.full(n, K.PREFILL, np.int32) for n in geometry]]
                dst, out = J.host_probe_star(list(zip(tabs, hows, kouts)),
                                             [_batches(f) for f in fks], words, pre)
                assert np.array_equal(dst, K.pack_bits(geometry, keep)), (da, db, hows, p)
                leg = kouts.index(0)
                for b, n in enumerate(geometry):
                    want = [pays[leg][b][r] if keep[b][r] else K.PREFILL for r in range(n)]
                    assert out[0][b].tolist() == want, (da, db, hows, p, b)


# ------------------------------------------------- the reference's own sum
def test_reference_sum_within_rule():
    """A plain float64 left-to-right sum of every pool stays within the
    rule: the rule asks nothing a correct summation cannot give."""
    rng = np.random.default_rng(9)
    for dt in K.FLOATS:
        for pool in K.POOLS[:-1]:
            for n in (1, 2, 65, 1000):
                v = K.pool_values(dt, pool, n, rng).astype(np.float64)
                for order in (v, v[::-1], np.sort(v)):
                    s = np.float64(0)
                    with np.errstate(invalid="ignore"):
                        for x in order:
                            s = s + x
                    K.check_float_sum(float(s), order.tolist(), (dt, pool, n))
    v = K.pool_values("f8", "subnormal", 500, rng)
    assert float(np.add.reduce(v)) == math.fsum(v.tolist())       # subnormals: exact
