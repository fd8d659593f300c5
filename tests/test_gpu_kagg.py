"""The aggregate, group and join kernels (csrc/kernels/colagg.hip,
colgroup.hip, coljoin.hip) through the ops/ wrappers against the brute-force
reference of tests/kagggen.py — not against the numpy twins: real floats
(infinities, NaN payloads, signed zeros, subnormals, cancelling values), every
value type and ops mask on its own, every key type, every replica count and
reduce width, a reduce that folds two slabs per lane, empty batches, dirty
validity and planted codes outside the accumulator arrays.

Measured on an MI355X (gfx950, -munsafe-fp-atomics): the float64 LDS atomic
(ds_add_f64) and the float64 L2 atomic (global_atomic_add_f64) keep subnormal
operands and results — the subnormal pools below sum exactly through the
register run, the LDS path, the HBM path and the reduce."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))

import kagggen as K  # noqa: E402

GEOMS = list(K.GEOMETRIES)
GUARD = 8
GUARD_WORD = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nvme_strom_amd as S
    S.configure(gpu_emulation=0)
    return S


def _words(words):
    return torch.from_numpy(np.asarray(words).view(np.int64).copy()).cuda()


# ------------------------------------------------------------------ colagg
class _Dev:
    """A case's tables on the device."""

    def __init__(self, case):
        self.keep = []
        self.vtab = K.upload(case.val, "cuda", self.keep, values=case.dt is not None)
        self.ktab = K.upload(case.key, "cuda", self.keep) if case.key is not None else None


def _dev_block(A, case, dev, lay, words):
    """Every entry of ``lay`` through launch and reduce: (the block on the
    host, the guard words around it)."""
    block = A.alloc_block(lay, "cuda", guard=GUARD)
    block._whole[:GUARD] = GUARD_WORD
    block._whole[-GUARD:] = GUARD_WORD
    sel = _words(words)
    for e in range(len(lay.entries)):
        A.agg_batched(lay, e, block, sel, case.nwords, dev.vtab, dev.ktab, count_bad=e == 0)
    torch.cuda.synchronize()
    whole = block._whole.cpu().numpy()
    return A.block_to_host(block), np.concatenate([whole[:GUARD], whole[-GUARD:]])


def _check_colagg(A, case, seed, ents=None, full=True):
    lay = A.Layout(ents or case.entries(), case.nslots, K.KEY_TYPES[case.key_dt] if case.key else 0)
    dev = _Dev(case)
    rng = np.random.default_rng(seed)
    for p in K.BITMAPS:
        bits, words = K.bitmap(case.geometry, p, rng)
        ref = K.case_reference(case, bits)
        K.assert_pools(case, ref[0], full and p == 1.0)
        if p and full and case.key_dt == "i4" and case.dt in K.FLOATS and \
                len(case.keyvals) >= K.NPOOLS:
            assert K.witnesses(ref[2], case.val, case.geometry, words) == K.WITNESSES, case.label
        got, guards = _dev_block(A, case, dev, lay, words)
        K.check_block(case, lay, got, ref, (case.label, p))
        assert (guards == GUARD_WORD).all(), (case.label, p)
        if p == 0.0:
            assert np.array_equal(got, A.new_block(lay))


@pytest.mark.parametrize("geom", GEOMS)
def test_colagg_flat(S, geom):
    """No key: every integer type, every float pool in a launch of its own,
    the validity-only column; ops masks 1 .. 15 and COUNT | ALL each alone."""
    from nvme_strom_amd.ops import colagg as A
    for i, case in enumerate(K.flat_cases(geom)):
        _check_colagg(A, case, 100 + i)


@pytest.mark.parametrize("geom", GEOMS)
def test_colagg_keyed(S, geom):
    """Every key type with its malformed keys (negative, >= nslots - 1,
    uint64 >= 2^63: counted, never followed, the guard words untouched), every
    value type, one float pool per key."""
    from nvme_strom_amd.ops import colagg as A
    for i, case in enumerate(K.keyed_type_cases(geom)):
        _check_colagg(A, case, 200 + i)


@pytest.mark.parametrize("pair,rl", K.REPLICA_CASES)
def test_colagg_replicas(S, pair, rl):
    """R = 256, 32, 4, 2 and 1 replicas of the LDS accumulators and reduce
    widths L = 64, 8, 4 and 2, by launch_agg's rule."""
    from nvme_strom_amd.ops import colagg as A
    ops, nslots = pair
    assert (K.replicas(ops, nslots), K.reduce_lanes(ops, nslots)) == rl
    assert A.nacc(ops) * nslots * 8 * rl[0] <= A.LDS_BYTES
    assert rl[0] == 256 or A.nacc(ops) * nslots * 8 * rl[0] * 2 > A.LDS_BYTES
    for dt in ("f8", "i8"):
        case, ent = K.replica_case(ops, nslots, dt)
        _check_colagg(A, case, 300 + nslots, [ent], full=nslots <= 40)


def test_colagg_reduce_second_trip(S):
    """40,000 + 0 + 30,001 rows are 1,094 words and 69 slabs: lanes 0 .. 4 of
    the reduce fold two slabs each.  Cancelling float64 values and wrapping
    int64 ones; the unkeyed float sum is the same bit for bit on a second run."""
    from nvme_strom_amd.ops import colagg as A
    from nvme_strom_amd.ops._util import lib
    for dt in ("f8", "i8"):
        case = K.big_case(dt)
        assert case.nwords == 1094
        assert int(lib().strom_column_agg_grid(case.nwords, 15, 1)) == 69 > 64
        bits, words = K.bitmap(case.geometry, 0.9, np.random.default_rng(41))
        lay = A.Layout([A.Entry(15, dt)])
        dev = _Dev(case)
        ref = K.case_reference(case, bits)
        got, guards = _dev_block(A, case, dev, lay, words)
        K.check_block(case, lay, got, ref, case.label)
        assert (guards == GUARD_WORD).all()
        again, _ = _dev_block(A, case, dev, lay, words)
        assert np.array_equal(got, again)


# ---------------------------------------------------------------- colgroup
def _dev_groups(G, case, dev, ents, bits, words, combine, in_place, multi=None, plant=None):
    """group_codes (or its composite form) and every entry's group_agg:
    (device Groups, header, the table).  ``plant``: [(batch, row, code)] written
    over the codes of selected rows before the accumulate launches, their
    bits left set; the accumulator arrays then lie between guard words."""
    geometry = case.geometry
    unsigned = multi is not None or np.dtype(case.key_dt).kind == "u"
    t = G.DeviceGroups(ents, 32, "cuda", unsigned, spec=multi[0] if multi else None)
    whole = None
    if plant:
        from nvme_strom_amd.ops._util import check, lib, ptr, stream_handle
        assert all(K.A.nacc(e.ops) == 1 for e in ents)          # guards around every array
        whole = torch.full((len(ents), t.stride + 2 * GUARD), GUARD_WORD, dtype=torch.int64,
                           device="cuda")
        t.acc = whole[:, GUARD:GUARD + t.stride]
        for i in range(len(ents)):
            t.args[i].acc = whole.data_ptr() + 8 * (i * (t.stride + 2 * GUARD) + GUARD)
        check(lib().strom_group_init(ptr(t.table), t.capacity, C.byref(t.args), len(t.args),
                                     stream_handle(None)),
              "group_init")
    buf, ctab = K.code_buffers(geometry, "cuda", dev.keep)
    src = _words(words)
    dst = src if in_place else torch.full_like(src, 0x1234)
    if multi:
        G.group_codes_multi(t, multi[1], case.nwords, src, dst, ctab)
    else:
        G.group_codes(t, G.KEY_CODE[case.key_dt], dev.ktab, case.nwords, src, dst, ctab)
    torch.cuda.synchronize()
    # no overflow: the destination is the selected rows, garbage cleared; only
    # their codes were written, and every code lies inside the arrays
    assert np.array_equal(dst.cpu().numpy().view(np.uint64), K.pack_bits(geometry, bits))
    codes = buf.cpu().numpy()
    flat_sel = np.concatenate([np.pad(b, (0, -len(b) % 64)) for b in bits] + [np.zeros(0, bool)])
    assert (codes[:len(flat_sel)][~flat_sel] == K.PREFILL).all()
    assert ((codes[:len(flat_sel)][flat_sel] >= 0) & (codes[:len(flat_sel)][flat_sel] < t.stride)).all()
    if plant:
        w0 = np.concatenate([[0], np.cumsum([(n + 63) // 64 for n in geometry])])
        for b, r, code in plant:
            assert bits[b][r]
            codes[int(w0[b]) * 64 + r] = code
        buf.copy_(torch.from_numpy(codes))
    for e in range(len(ents)):
        G.group_agg(t, e, dst, case.nwords, dev.vtab, ctab, combine=combine)
    hdr, got = G.compact(t)
    torch.cuda.synchronize()
    assert int(hdr[G.H_OVERFLOW]) == 0 and int(hdr[G.H_CAPACITY]) == t.capacity
    if whole is not None:
        w = whole.cpu().numpy()
        assert (w[:, :GUARD] == GUARD_WORD).all() and (w[:, -GUARD:] == GUARD_WORD).all()
    return got, hdr


@pytest.mark.parametrize("geom", GEOMS)
def test_colgroup(S, geom):
    """group_codes + group_agg by key: every key type (INT64_MIN and 2^63,
    the free slot's pattern, among the keys), every value type and ops mask,
    one float pool per key, combine off and on, in place and not."""
    from nvme_strom_amd.ops import colgroup as G
    for i, case in enumerate(K.group_cases(geom)):
        ents = case.entries()
        dev = _Dev(case)
        rng = np.random.default_rng(400 + i)
        for p in K.BITMAPS:
            bits, words = K.bitmap(case.geometry, p, rng)
            groups, nbad, log = K.case_reference(case, bits, gid_of=K.value_gid)
            K.assert_pools(case, groups, p == 1.0)
            if p and case.key_dt == "i4" and case.dt in K.FLOATS:
                assert K.witnesses(log, case.val, case.geometry, words) == K.WITNESSES, case.label
            for combine in (0, 1):
                got, hdr = _dev_groups(G, case, dev, ents, bits, words, combine, bool(combine))
                assert int(hdr[G.H_NKEYS]) == len([k for k in groups if k is not None])
                K.check_groups([int(k) for k in got.keys], got.layout, got.block, groups,
                               (case.label, p, combine))


@pytest.mark.parametrize("geom", GEOMS)
def test_colgroup_multi(S, geom):
    """GROUP BY a nullable int16 and a uint32 over the same geometry."""
    from nvme_strom_amd.ops import colgroup as G
    spec = G.KeySpec(K.MULTI_SPEC)
    for i, dt in enumerate(["f8", "f4", "i8", None]):
        case, kb = K.multi_case(geom, dt, np.random.default_rng(50 + i))
        ents = case.entries()
        dev = _Dev(case)
        ktabs = torch.stack([dev.ktab, K.upload(kb, "cuda", dev.keep)]).contiguous()
        rng = np.random.default_rng(500 + i)
        for p in K.BITMAPS:
            bits, words = K.bitmap(case.geometry, p, rng)
            groups, _, _ = K.case_reference(case, bits, [case.key, kb], lambda k: k)
            K.assert_pools(case, groups, p == 1.0)
            for combine in (0, 1):
                got, hdr = _dev_groups(G, case, dev, ents, bits, words, combine, bool(combine),
                                       multi=(spec, ktabs))
                assert not hdr[G.H_RANGE:G.H_RANGE + 2].any()
                K.check_groups(K.multi_keys(spec, got.keys), got.layout, got.block, groups,
                               (case.label, p, combine))


@pytest.mark.parametrize("dt", ["f8", "i8"])
def test_colgroup_codes_outside_the_arrays(S, dt):
    """Selected rows whose codes are -77, capacity + 2 and 2^31 - 1 (never
    written by the codes launch) are not followed: every accumulator equals the
    reference over the remaining rows, the guard words around each accumulator
    array stay as they were."""
    from nvme_strom_amd.ops import colagg as A
    from nvme_strom_amd.ops import colgroup as G
    case = next(c for c in K.group_cases("plain") if c.label == f"group-i4-{dt}")
    ents = [A.Entry(op, dt) for op in (A.COUNT, A.SUM, A.MIN, A.MAX)] + \
        [A.Entry(A.COUNT | A.ALL, None)]
    dev = _Dev(case)
    geometry = case.geometry
    b = geometry.index(1000)
    at = K.plant_at(geometry) - sum(geometry[:b])
    for p in K.BITMAPS[:2]:
        bits, words = K.bitmap(geometry, p, np.random.default_rng(61))
        first = lambda bb, lo: lo + int(np.flatnonzero(bits[bb][lo:])[0])
        b257, b65 = geometry.index(257), geometry.index(65)
        # the first selected row of a one-key word, the second of the next, a row of
        # the mixed word, the last of another batch, the lone row of a last word
        spots = [(b, first(b, at)), (b, first(b, first(b, at + 64) + 1)), (b, first(b, at + 200)),
                 (b257, int(np.flatnonzero(bits[b257])[-1]))] + ([(b65, 64)] if bits[b65][64] else [])
        outside = [-77, G.capacity(32) + 2, 2**31 - 1]
        rows = [(bb, r, outside[j % 3]) for j, (bb, r) in enumerate(spots)]
        assert len({r[:2] for r in rows}) == len(rows) >= 4
        left = [x.copy() for x in bits]
        for bb, r, _ in rows:
            left[bb][r] = False
        groups, _, _ = K.case_reference(case, left, gid_of=K.value_gid)
        for combine in (0, 1):
            got, _ = _dev_groups(G, case, dev, ents, bits, words, combine, False, plant=rows)
            K.check_groups([int(k) for k in got.keys], got.layout, got.block, groups,
                           (case.label, p, combine))


# ----------------------------------------------------------------- coljoin
def _dev_table(J, dim):
    t = J.build(torch.from_numpy(np.array(list(dim), np.int64)).cuda(),
                torch.from_numpy(np.array(list(dim.values()), np.int32)).cuda())
    torch.cuda.synchronize()
    return t


def _expect_codes(geometry, keep, pays):
    return K.expected_buffer(geometry, [[pays[b][r] if keep[b][r] else K.PREFILL for r in range(n)]
                                        for b, n in enumerate(geometry)])


@pytest.mark.parametrize("geom", GEOMS)
def test_coljoin_probe(S, geom):
    """Semi and anti, in place and not, with and without key output, every
    fk type with dirty and all-null validity, against a per-row dict lookup;
    the key-output words between a batch's rows and the next batch stay
    untouched."""
    from nvme_strom_amd.ops import coljoin as J
    geometry = K.GEOMETRIES[geom][0]
    nwords = K.nwords_of(geometry)
    for i, fk_dt in enumerate(K.INTS):
        rng = np.random.default_rng(600 + i)
        fk, dim = K.join_fk(geom, fk_dt, rng), K.join_dim(fk_dt)
        keep_alive = []
        ftab = K.upload(fk, "cuda", keep_alive)
        table = _dev_table(J, dim)
        for p in K.BITMAPS:
            bits, words = K.bitmap(geometry, p, rng)
            for how, with_out in ((J.SEMI, True), (J.SEMI, False), (J.ANTI, False)):
                keep, pays = K.join_reference(bits, [fk], [dim], [how])
                want = K.pack_bits(geometry, keep)
                for in_place in (False, True):
                    src = _words(words)
                    dst = src if in_place else torch.full_like(src, 0x1234)
                    cnt = torch.full((1,), 5, dtype=torch.int64, device="cuda")
                    buf, ctab = K.code_buffers(geometry, "cuda", keep_alive)
                    J.probe(table, J.FK_CODE[fk_dt], ftab, nwords, src, dst, cnt, how,
                            key_out=ctab if with_out else None)
                    torch.cuda.synchronize()
                    what = (fk_dt, p, how, with_out, in_place)
                    assert np.array_equal(dst.cpu().numpy().view(np.uint64), want), what
                    assert int(cnt.item()) == 5 + sum(int(k.sum()) for k in keep), what
                    if not in_place:
                        assert np.array_equal(src.cpu().numpy().view(np.uint64), words), what
                    exp = _expect_codes(geometry, keep, pays[0]) if with_out else \
                        K.expected_buffer(geometry, [[K.PREFILL] * n for n in geometry])
                    assert np.array_equal(buf.cpu().numpy(), exp), what
                    del keep_alive[-2:]


@pytest.mark.parametrize("geom", GEOMS)
def test_coljoin_probe_star(S, geom):
    """Two legs in one walk, one semi with key output and one anti, in both
    orders."""
    from nvme_strom_amd.ops import coljoin as J
    geometry = K.GEOMETRIES[geom][0]
    nwords = K.nwords_of(geometry)
    for i, (da, db) in enumerate([("i4", "u8"), ("i8", "u1"), ("u2", "i1")]):
        rng = np.random.default_rng(700 + i)
        fks = [K.join_fk(geom, da, rng), K.join_fk(geom, db, rng)]
        dims = [K.join_dim(da, 0), K.join_dim(db, 1)]
        keep_alive = []
        ftabs = torch.stack([K.upload(f, "cuda", keep_alive) for f in fks]).contiguous()
        tabs = [_dev_table(J, d) for d in dims]
        for hows, kouts in (([J.SEMI, J.ANTI], [0, -1]), ([J.ANTI, J.SEMI], [-1, 0])):
            legs = [(t, J.FK_CODE[dt], how, ko) for t, dt, how, ko in zip(tabs, (da, db), hows, kouts)]
            for p in K.BITMAPS:
                bits, words = K.bitmap(geometry, p, rng)
                keep, pays = K.join_reference(bits, fks, dims, hows)
                for in_place in (False, True):
                    src = _words(words)
                    dst = src if in_place else torch.full_like(src, 0x1234)
                    cnt = torch.full((1,), 5, dtype=torch.int64, device="cuda")
                    buf, ctab = K.code_buffers(geometry, "cuda", keep_alive)
                    kout = ctab.unsqueeze(0).contiguous()
                    J.probe_star(legs, ftabs, nwords, src, dst, cnt, key_out=kout)
                    torch.cuda.synchronize()
                    what = (da, db, hows, p, in_place)
                    assert np.array_equal(dst.cpu().numpy().view(np.uint64),
                                          K.pack_bits(geometry, keep)), what
                    assert int(cnt.item()) == 5 + sum(int(k.sum()) for k in keep), what
                    exp = _expect_codes(geometry, keep, pays[kouts.index(0)])
                    assert np.array_equal(buf.cpu().numpy(), exp), what
                    del keep_alive[-2:]
