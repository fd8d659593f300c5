"""The column filter, qualifier and row-emit kernels (colfilter.hip) called
directly on hand-built batch tables, against the brute-force reference of
tests/qualgen.py.  Every comparison is exact: all bitmap words (tail bits
included), the counts, the row ids and the projected bytes."""
import numpy as np
import pytest
import torch

import qualgen as G
from nvme_strom_amd.ops import colpred as CP

pytestmark = pytest.mark.gpu

_TORCH = {"i4": torch.int32, "i8": torch.int64, "f4": torch.float32, "f8": torch.float64}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def _dev_words(w, dev):
    return torch.from_numpy(np.ascontiguousarray(w).view(np.int64).copy()).to(dev)


def _host_words(t):
    return t.cpu().numpy().view(np.uint64)


def _run_case(dev, case, combos=((False, False), (True, False), (False, True), (True, True))):
    """kernel == brute force in each combination mode; one count accumulates
    over the launches."""
    t = case.table
    dtab = G.DeviceTable(t, dev)
    pred = G.pack_words(t, G.brute(t, case.ref))
    rng = np.random.default_rng(len(case.name))
    nw = t.nwords
    old = rng.integers(0, 1 << 64, nw + 1, dtype=np.uint64, endpoint=False)
    orw = rng.integers(0, 1 << 64, nw, dtype=np.uint64, endpoint=False)
    or_t = _dev_words(orw, dev)
    cnt = torch.full((1,), 7, dtype=torch.int64, device=dev)
    total = 7
    for use_or, and_dst in combos:
        bm = _dev_words(old, dev)                       # the last word is a guard
        CP.qual_batched(case.compiled, dtab.qtab, nw, bm, cnt, or_src=or_t if use_or else None,
                        and_dst=and_dst)
        exp = G.expected_words(pred, orw if use_or else None, and_dst, old[:nw])
        got = _host_words(bm)
        bad = np.flatnonzero(got[:nw] != exp)
        assert not len(bad), (case.name, use_or, and_dst, bad[:8],
                              [hex(x) for x in got[bad[:4]]], [hex(x) for x in exp[bad[:4]]])
        assert got[nw] == old[nw], case.name
        total += G.popcount(exp)
        assert int(cnt.item()) == total, (case.name, use_or, and_dst)


# ------------------------------------------------------- 1. numeric ranges
@pytest.mark.parametrize("dt", G.INT_TYPES + ["f4", "f8", "b1", "d16"])
def test_qual_numeric_ranges(dev, dt):
    rng = np.random.default_rng(11)
    cases = G.numeric_cases(dt, rng)
    if dt == "u8":
        cases.append(G.u64_high_case(rng))
    if dt in G.INT_TYPES:
        cases += [G.in_list_case(dt, 9, rng, False), G.in_list_case(dt, 40, rng, True)]
    for case in cases:
        _run_case(dev, case)


def test_qual_grid_stride(dev):
    """nwords just above 8192 blocks x 16 words: the grid-stride loop takes a
    second trip.  The reference is the brute force per distinct u8 value."""
    rng = np.random.default_rng(21)
    geo = [64 * 50000 + 1, 64 * 60000 + 63, 64 * 21109 + 5]
    vals = rng.integers(0, 256, sum(geo), dtype=np.uint8)
    t = G.table("u1", vals, rng, geo, [None, "dirty", None])
    assert t.nwords == 8192 * 16 + 40
    rs = [(3, 3), (10, 12), (40, 41), (60, 60), (77, 90), (100, 100), (130, 140), (200, 201),
          (250, 255)]
    c = CP.compile_pred(CP.Pred("c", "ranges", tuple(rs)), G.column("u1"))
    assert c.nconst == 9
    by_value = np.array([any(lo <= v <= hi for lo, hi in rs) for v in range(256)], bool)
    bits = [by_value[b.values] & (b.valid if b.valid is not None else True) for b in t.batches]
    pred = G.pack_words(t, bits)
    dtab = G.DeviceTable(t, dev)
    old = rng.integers(0, 1 << 64, t.nwords + 1, dtype=np.uint64, endpoint=False)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    total = 0
    for and_dst in (False, True):
        bm = _dev_words(old, dev)
        CP.qual_batched(c, dtab.qtab, t.nwords, bm, cnt, and_dst=and_dst)
        exp = G.expected_words(pred, None, and_dst, old[:t.nwords])
        got = _host_words(bm)
        assert np.array_equal(got[:t.nwords], exp) and got[t.nwords] == old[t.nwords]
        total += G.popcount(exp)
        assert int(cnt.item()) == total


# ------------------------------------------------------------------ 2. LUT
@pytest.mark.parametrize("dt", G.LUT_INDEX_TYPES)
def test_qual_lut(dev, dt):
    rng = np.random.default_rng(13)
    for nconst in G.LUT_SIZES:
        _run_case(dev, G.lut_case(dt, nconst, rng))


# -------------------------------------------------------------- 3. strings
@pytest.mark.parametrize("malformed", [False, True])
@pytest.mark.parametrize("dt", ["s4", "s8"])
def test_qual_strings(dev, dt, malformed):
    """Equality, IN, prefix and range predicates over rows at every start
    alignment; with ``malformed``, rows whose offsets are negative,
    decreasing or past the characters: selected by no string predicate,
    NEGATE or not, still counted by is_valid / is_null."""
    rng = np.random.default_rng(14)
    for case in G.str_cases(dt, rng, malformed):
        _run_case(dev, case, combos=((False, False), (True, True)))


# --------------------------------------------------------------- 6. limits
def test_qual_limit_operands(dev):
    """The largest operands compile_pred accepts (64 KiB of constants: int64
    ranges, a LUT, a string IN-list with its offsets) launch and are right."""
    for case in G.limit_cases(np.random.default_rng(16)):
        _run_case(dev, case, combos=((False, False), (True, True)))


# -------------------------------------------------------- 4. range filters
def _filter_table(dt, rng):
    return G.table(dt, G.filter_values(dt, sum(G.GEOMETRY), rng), rng)


@pytest.mark.parametrize("dt", ["i4", "i8", "f4", "f8"])
def test_column_filter_bounds(dev, dt):
    from nvme_strom_amd.ops.colfilter import column_filter
    rng = np.random.default_rng(31)
    n = 1000 + 37
    v = G.filter_values(dt, n, rng)
    vt = torch.from_numpy(v).to(dev)
    for with_valid in (False, True):
        b = G.Batch(n, v, rng.random(n) < 0.85 if with_valid else None, "dirty")
        t = G.Table(dt, [b])
        vb = torch.from_numpy(G.valid_words(b).view(np.uint8).copy()).to(dev) if with_valid else None
        for lo, hi in G.TYPE_BOUNDS[dt]:
            bm, cnt = column_filter(vt, lo, hi, vb)
            exp = G.pack_words(t, G.brute_filter(t, lo, hi))
            assert np.array_equal(_host_words(bm), exp), (dt, lo, hi, with_valid)
            assert cnt == G.popcount(exp), (dt, lo, hi, with_valid)


@pytest.mark.parametrize("dt", ["i4", "i8", "f4", "f8"])
def test_filter_batched_bounds(dev, dt):
    """filter_batched over the batch geometry: count += the selected rows;
    with combine the predicate is ANDed into the words already there and
    count += the rows left selected.  An empty or NaN range writes zero
    words and leaves the count as it was."""
    from nvme_strom_amd.ops.colfilter import filter_batched
    rng = np.random.default_rng(32)
    t = _filter_table(dt, rng)
    dtab = G.DeviceTable(t, dev)
    nw = t.nwords
    old = rng.integers(0, 1 << 64, nw + 1, dtype=np.uint64, endpoint=False)
    bounds = G.TYPE_BOUNDS[dt]
    cnt = torch.full((1,), 5, dtype=torch.int64, device=dev)
    total = 5
    for k, (lo, hi) in enumerate(bounds):
        bm = _dev_words(old, dev)
        filter_batched(_TORCH[dt], dtab.ftab, nw, lo, hi, bm, cnt)
        exp = G.pack_words(t, G.brute_filter(t, lo, hi))
        got = _host_words(bm)
        assert np.array_equal(got[:nw], exp) and got[nw] == old[nw], (dt, lo, hi)
        total += G.popcount(exp)
        assert int(cnt.item()) == total, (dt, lo, hi)
        # the next qualifier of a conjunction, on the words just written
        lo2, hi2 = bounds[(k + 3) % len(bounds)]
        filter_batched(_TORCH[dt], dtab.ftab, nw, lo2, hi2, bm, cnt, combine=True)
        exp2 = exp & G.pack_words(t, G.brute_filter(t, lo2, hi2))
        got = _host_words(bm)
        assert np.array_equal(got[:nw], exp2) and got[nw] == old[nw], (dt, lo, hi, lo2, hi2)
        total += G.popcount(exp2)
        assert int(cnt.item()) == total, (dt, lo, hi, lo2, hi2)
        # combine into words nobody cleared: tail bits and empty ranges end as zeros
        bm = _dev_words(old, dev)
        filter_batched(_TORCH[dt], dtab.ftab, nw, lo, hi, bm, cnt, combine=True)
        exp3 = exp & old[:nw]
        assert np.array_equal(_host_words(bm)[:nw], exp3), (dt, lo, hi)
        total += G.popcount(exp3)
        assert int(cnt.item()) == total, (dt, lo, hi)


# ------------------------------------------------------------- 5. row emit
_PROJ = {1: "u1", 2: "u2", 4: "i4", 8: "i8", 16: "d16"}


def _proj_table(width, rng, row0):
    dt = _PROJ[width]
    n = sum(G.GEOMETRY)
    if width == 16:
        vals = [int(rng.integers(-1 << 62, 1 << 62)) << int(rng.integers(0, 65)) for _ in range(n)]
    else:
        info = np.iinfo(np.dtype(dt))
        vals = rng.integers(info.min, info.max, n, dtype=np.dtype(dt), endpoint=True)
    return G.table(dt, vals, rng, row0=row0)


def _row_bits(t, rng, density):
    return [rng.random(b.nrows) < density for b in t.batches]


@pytest.mark.parametrize("width", [1, 2, 4, 8, 16])
def test_bitmap_to_rows_proj(dev, width):
    """Row ids = numpy.nonzero + row_base, the projected values and their
    validity next to them; the cursor starts at 5 and a second call appends."""
    from nvme_strom_amd.ops.colfilter import bitmap_to_rows
    rng = np.random.default_rng(40 + width)
    t = _proj_table(width, rng, row0=1000)
    dtab = G.DeviceTable(t, dev)
    nw = t.nwords
    calls = [_row_bits(t, rng, 0.3), _row_bits(t, rng, 0.9)]
    refs = [G.emit_reference(t, bits) for bits in calls]
    n_out = 5 + sum(len(ids) for ids, _ in refs) + 3
    out = torch.full((n_out,), -1, dtype=torch.int64, device=dev)
    tdt = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64, 16: torch.int64}[width]
    pout = torch.zeros((n_out, 2) if width == 16 else (n_out,), dtype=tdt, device=dev)
    pvalid = torch.full((n_out,), 9, dtype=torch.uint8, device=dev)
    cursor = torch.full((1,), 5, dtype=torch.int64, device=dev)
    at = 5
    for bits, (ids, sel) in zip(calls, refs):
        bm = _dev_words(G.pack_words(t, bits), dev)
        bitmap_to_rows(bm, nw, dtab.ftab, out, cursor, proj=dtab.ftab, proj_out=pout,
                       proj_valid=pvalid)
        end = at + len(ids)
        assert int(cursor.item()) == end
        assert np.array_equal(out[at:end].cpu().numpy(), ids)
        raw = b"".join(G.values_bytes(t.dt, G.Batch(len(s), [b.values[i] for i in s] if width == 16
                                                    else b.values[s], None))
                       for b, s in zip(t.batches, sel))
        assert pout[at:end].cpu().numpy().tobytes() == raw
        vref = np.concatenate([b.valid[s] if b.valid is not None else np.ones(len(s), bool)
                               for b, s in zip(t.batches, sel)]).astype(np.uint8)
        assert np.array_equal(pvalid[at:end].cpu().numpy(), vref)
        at = end
    assert (out[:5] == -1).all() and (out[at:] == -1).all()
    assert (pvalid[:5] == 9).all() and (pvalid[at:] == 9).all()


def test_bitmap_to_rows_proj_without_valid_output(dev):
    from nvme_strom_amd.ops.colfilter import bitmap_to_rows
    rng = np.random.default_rng(39)
    t = _proj_table(4, rng, row0=0)
    dtab = G.DeviceTable(t, dev)
    bits = _row_bits(t, rng, 0.5)
    ids, sel = G.emit_reference(t, bits)
    out = torch.full((len(ids) + 1,), -1, dtype=torch.int64, device=dev)
    pout = torch.zeros(len(ids) + 1, dtype=torch.int32, device=dev)
    cursor = torch.zeros(1, dtype=torch.int64, device=dev)
    bitmap_to_rows(_dev_words(G.pack_words(t, bits), dev), t.nwords, dtab.ftab, out, cursor,
                   proj=dtab.ftab, proj_out=pout)
    assert int(cursor.item()) == len(ids)
    assert np.array_equal(out[:-1].cpu().numpy(), ids) and int(out[-1]) == -1
    assert np.array_equal(pout[:-1].cpu().numpy(),
                          np.concatenate([b.values[s] for b, s in zip(t.batches, sel)]))


@pytest.mark.parametrize("density", [0.0, 0.01])
def test_bitmap_to_rows_many_blocks(dev, density):
    """300 001 words: 1172 blocks of 256 words, so the one-workgroup scan of
    the block counts gives each of its 1024 threads more than one block."""
    from nvme_strom_amd.ops.colfilter import bitmap_to_rows
    rng = np.random.default_rng(45)
    geo = [64 * 150000 - 37, 64 * 150001 - 1]
    t = G.Table("u1", [G.Batch(n, None, None) for n in geo], row0=123)
    assert t.nwords == 300001
    dtab = G.DeviceTable(t, dev, with_values=False)
    bits = _row_bits(t, rng, density)
    ids, _ = G.emit_reference(t, bits)
    out = torch.full((7 + len(ids) + 2,), -1, dtype=torch.int64, device=dev)
    cursor = torch.full((1,), 7, dtype=torch.int64, device=dev)
    bitmap_to_rows(_dev_words(G.pack_words(t, bits), dev), t.nwords, dtab.ftab, out, cursor)
    assert int(cursor.item()) == 7 + len(ids)
    got = out.cpu().numpy()
    assert np.array_equal(got[7:7 + len(ids)], ids)
    assert (got[:7] == -1).all() and (got[7 + len(ids):] == -1).all()


@pytest.mark.parametrize("dt", ["s4", "s8"])
def test_bitmap_to_rows_str(dev, dt):
    """String projection with a validity output, both cursors starting
    non-zero, two calls appending; empty strings, and malformed offset
    pairs, which project as empty strings."""
    from nvme_strom_amd.ops.colfilter import bitmap_to_rows_str
    rng = np.random.default_rng(46)
    t = G.str_table(dt, rng, malformed=True, row0=77)
    dtab = G.DeviceTable(t, dev)
    calls = [_row_bits(t, rng, 0.5), _row_bits(t, rng, 1.0)]
    for b, h in zip(t.batches, calls[0]):           # the malformed rows in the first call too
        h |= np.array([G.row_bytes(b, i) is None for i in range(b.nrows)], bool)
    refs = []
    for bits in calls:
        ids, sel = G.emit_reference(t, bits)
        strs = [G.row_bytes(b, i) or b"" for b, s in zip(t.batches, sel) for i in s]
        vref = np.concatenate([b.valid[s] if b.valid is not None else np.ones(len(s), bool)
                               for b, s in zip(t.batches, sel)]).astype(np.uint8)
        refs.append((ids, strs, vref))
    assert any(s == b"" for s in refs[0][1])
    nrow = 5 + sum(len(r[0]) for r in refs) + 2
    nchar = 11 + sum(len(s) for r in refs for s in r[1]) + 16
    out = torch.full((nrow,), -1, dtype=torch.int64, device=dev)
    poff = torch.full((nrow,), -1, dtype=torch.int64, device=dev)
    pvalid = torch.full((nrow,), 9, dtype=torch.uint8, device=dev)
    pchars = torch.full((nchar,), 0xA5, dtype=torch.uint8, device=dev)
    cursor = torch.full((1,), 5, dtype=torch.int64, device=dev)
    ccursor = torch.full((1,), 11, dtype=torch.int64, device=dev)
    at, cat = 5, 11
    for bits, (ids, strs, vref) in zip(calls, refs):
        bm = _dev_words(G.pack_words(t, bits), dev)
        bitmap_to_rows_str(bm, t.nwords, dtab.ftab, out, cursor, dtab.qtab, 4 if dt == "s4" else 8,
                           poff, pchars, ccursor, pvalid=pvalid)
        end, cend = at + len(ids), cat + sum(len(s) for s in strs)
        assert (int(cursor.item()), int(ccursor.item())) == (end, cend)
        assert np.array_equal(out[at:end].cpu().numpy(), ids)
        starts = cat + np.concatenate([[0], np.cumsum([len(s) for s in strs])])[:-1]
        assert np.array_equal(poff[at:end].cpu().numpy(), starts)
        assert pchars[cat:cend].cpu().numpy().tobytes() == b"".join(strs)
        assert np.array_equal(pvalid[at:end].cpu().numpy(), vref)
        at, cat = end, cend
    assert (out[:5] == -1).all() and (out[at:] == -1).all()
    assert (pchars[:11] == 0xA5).all() and (pchars[cat:] == 0xA5).all()
