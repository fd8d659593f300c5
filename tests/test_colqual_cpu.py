"""The numpy twin of the qualifier kernel (colpred.evaluate), the host bound
conversion of the range filters and the operand limits, against the
brute-force reference of tests/qualgen.py.  No GPU; the same cases run on
the device in tests/test_gpu_colqual.py."""
import ctypes as C
import math

import numpy as np
import pytest

import qualgen as G
from nvme_strom_amd.ops import colpred as CP


def _check_twin(case):
    ref = G.brute(case.table, case.ref)
    for k, b in enumerate(case.table.batches):
        got = CP.evaluate(case.compiled, G.host_values(case.table, b), b.valid, b.nrows)
        assert got.dtype == bool and got.shape == (b.nrows,), (case.name, k)
        assert np.array_equal(got, ref[k]), (case.name, k, np.flatnonzero(got != ref[k])[:8])


def _selective(case):
    """The case can fail: the reference selects some rows and leaves some."""
    ref = np.concatenate(G.brute(case.table, case.ref))
    return 0 < ref.sum() < len(ref)


@pytest.mark.parametrize("dt", G.INT_TYPES + ["f4", "f8", "b1", "d16"])
def test_twin_numeric_ranges(dt):
    rng = np.random.default_rng(11)
    cases = G.numeric_cases(dt, rng)
    if dt == "u8":
        cases.append(G.u64_high_case(rng))
    if dt in G.INT_TYPES:
        cases += [G.in_list_case(dt, 9, rng, False), G.in_list_case(dt, 40, rng, True)]
    for case in cases:
        _check_twin(case)
        assert _selective(case), case.name


def test_range_values_reach_the_edges():
    """Every numeric case holds rows on both endpoints of a range, just
    outside them, below the first range and above the last."""
    rng = np.random.default_rng(12)
    for dt in ("i2", "u8", "f4", "d16"):
        for case in G.numeric_cases(dt, rng):
            rs = case.ref["ranges"]
            vals = [v for b in case.table.batches for v in list(b.values)]
            vals = [float(v) if dt[0] == "f" else int(v) for v in vals]
            has = lambda p: any(p(v) for v in vals)            # noqa: E731
            assert has(lambda v: any(v == lo for lo, _ in rs)), case.name
            if rs != [(-0.0, 0.1)]:                 # 0.1 is no float32: 0.1f sits just above it
                assert has(lambda v: any(v == hi for _, hi in rs)), case.name
            tmin, tmax = (-math.inf, math.inf) if dt[0] == "f" else G.int_domain(dt)
            if rs[0][0] != tmin:
                assert has(lambda v: v < rs[0][0]), case.name
            if rs[-1][1] != tmax:
                assert has(lambda v: v > rs[-1][1]), case.name
            if len(rs) > 1:
                assert has(lambda v: rs[0][1] < v < rs[1][0]), case.name


@pytest.mark.parametrize("dt", G.LUT_INDEX_TYPES)
def test_twin_lut(dt):
    rng = np.random.default_rng(13)
    for nconst in G.LUT_SIZES:
        case = G.lut_case(dt, nconst, rng)
        _check_twin(case)
        assert len(case.compiled.consts) * 8 >= nconst


@pytest.mark.parametrize("malformed", [False, True])
@pytest.mark.parametrize("dt", ["s4", "s8"])
def test_twin_strings(dt, malformed):
    rng = np.random.default_rng(14)
    cases = G.str_cases(dt, rng, malformed)
    t = cases[0].table
    # every row under test at every start alignment of the character buffer
    seen = set()
    for b in t.batches:
        offs = b.values[0]
        for i in range(b.nrows):
            x = G.row_bytes(b, i)
            if x is not None:
                seen.add((x, int(offs[i]) % 4))
    if not malformed:
        assert {(r, a) for r in G.str_rows(np.random.default_rng(14)) if r for a in range(4)} <= seen
    nbad = sum(G.row_bytes(b, i) is None for b in t.batches for i in range(b.nrows))
    assert (nbad >= 6) if malformed else nbad == 0
    for case in cases:
        _check_twin(case)
        if case.ref["kind"] != "valid" and "empty" not in case.name:
            assert _selective(case), case.name


def test_malformed_rows_are_selected_by_nothing():
    """A malformed offset pair is selected by no string predicate, negated
    or not, and still counts for is_valid / is_null."""
    rng = np.random.default_rng(15)
    for case in G.str_cases("s4", rng, True):
        for b in case.table.batches:
            bad = np.array([G.row_bytes(b, i) is None for i in range(b.nrows)], bool)
            got = CP.evaluate(case.compiled, G.host_values(case.table, b), b.valid, b.nrows)
            ok = np.ones(b.nrows, bool) if b.valid is None else b.valid
            if case.ref["kind"] == "valid":
                assert np.array_equal(got[bad], (~ok if case.ref.get("neg") else ok)[bad])
            else:
                assert not got[bad].any(), case.name


def test_twin_limit_operands():
    for case in G.limit_cases(np.random.default_rng(16)):
        _check_twin(case)
        assert _selective(case), case.name


# ------------------------------------------------------------- filter bounds
_CODE = {"i4": 1, "i8": 2, "f4": 3, "f8": 4}
_CT = {"i4": C.c_int32, "i8": C.c_int64, "f4": C.c_float, "f8": C.c_double}


def _native_bounds(dt, lo, hi):
    from nvme_strom_amd._native import lib
    a, b = _CT[dt](), _CT[dt]()
    rc = lib().strom_filter_bounds(_CODE[dt], lo, hi, C.byref(a), C.byref(b))
    assert rc in (0, 1), rc
    return rc, a.value, b.value


@pytest.mark.parametrize("dt", ["i4", "i8", "f4", "f8"])
def test_filter_bounds(dt):
    for lo, hi in G.TYPE_BOUNDS[dt]:
        rc, a, b = _native_bounds(dt, lo, hi)
        ref = G.bounds_reference(dt, lo, hi)
        if ref is None:
            assert (rc, a, b) == (0, 1, 0), (dt, lo, hi)
            continue
        assert rc == 1, (dt, lo, hi)
        if dt[0] == "i":
            assert (a, b) == ref, (dt, lo, hi)
            # the definition itself: the least integer of the type >= lo, the largest <= hi
            tmin, tmax = G.int_domain(dt)
            assert a >= lo and (a == tmin or a - 1 < lo), (dt, lo, hi)
            assert b <= hi and (b == tmax or b + 1 > hi), (dt, lo, hi)
        else:
            f = np.dtype(dt).type
            assert f(a) == ref[0] and f(b) == ref[1], (dt, lo, hi)
            assert math.copysign(1, a) == math.copysign(1, float(ref[0])) or a != 0
            assert float(f(a)) >= lo and float(f(b)) <= hi, (dt, lo, hi)
            if float(f(a)) > lo:
                assert float(np.nextafter(f(a), f(-math.inf))) < lo, (dt, lo, hi)
            if float(f(b)) < hi:
                assert float(np.nextafter(f(b), f(math.inf))) > hi, (dt, lo, hi)


def test_filter_bounds_bad_type():
    from nvme_strom_amd._native import lib
    a = C.c_int64()
    assert lib().strom_filter_bounds(7, 0.0, 1.0, C.byref(a), C.byref(a)) == -22
    assert lib().strom_filter_bounds(1, 0.0, 1.0, None, C.byref(a)) == -22


def test_filter_bounds_select_what_the_doubles_do():
    """Comparing in the column's type with the converted bounds selects
    exactly the rows the double bounds select."""
    rng = np.random.default_rng(17)
    for dt in ("i4", "i8", "f4", "f8"):
        v = G.filter_values(dt, 400, rng)
        t = G.Table(dt, [G.Batch(len(v), v, None)])
        for lo, hi in G.TYPE_BOUNDS[dt]:
            rc, a, b = _native_bounds(dt, lo, hi)
            a, b = np.dtype(dt).type(a), np.dtype(dt).type(b)
            with np.errstate(invalid="ignore"):
                got = (v >= a) & (v <= b)
            assert np.array_equal(got, G.brute_filter(t, lo, hi)[0]), (dt, lo, hi)


# -------------------------------------------------------------------- limits
def _refused(pred, dt):
    with pytest.raises(ValueError, match=r"column c\b"):
        CP.compile_pred(pred, G.column(dt))


def test_limits_refused_in_python():
    """What strom_column_qual refuses with -7 (constants + string offsets
    over 64 KiB) never compiles."""
    for n in (2049, 4096):
        _refused(CP.Pred("c", "ranges", tuple((10 * k, 10 * k + 3) for k in range(n))), "d16")
    # string ranges: 24 bytes of (start, len, mode) per range + the blob
    for n in (2731, 4096):
        _refused(CP.Pred("c", "ranges", tuple((b"%05da" % k, b"%05dz" % k) for k in range(n))), "s4")
    _refused(CP.Pred("c", "ranges", tuple((b"%05d" % k + b"a" * 19, b"%05d" % k + b"z" * 19)
                                          for k in range(1000))), "s8")
    # string IN-list: 4096 constants and 48 KiB of blob
    _refused(CP.Pred("c", "in", tuple(b"%012d" % k for k in range(4096))), "s4")
    _refused(CP.Pred("c", "not in", tuple(b"%08dx" % k for k in range(4096))), "s8")
    _refused(CP.Pred("c", "prefix", [b"%08dx" % k for k in range(4096)]), "s4")
    _refused(CP.Pred("c", "ranges", tuple((10 * k, 10 * k + 3) for k in range(4097))), "i8")


def test_library_limit_is_the_python_limit():
    """strom_column_qual refuses one dword more than MAX_QUAL_BYTES with -7,
    before it looks at any of the (here made-up) device addresses."""
    from nvme_strom_amd._native import lib
    for typ, op, cb, ob in [(CP.COL_CODE["i8"], CP.QOP_RANGES, CP.MAX_QUAL_BYTES + 4, 0),
                            (CP.COL_STR32, CP.QOP_STR_IN, CP.MAX_QUAL_BYTES - 8, 12),
                            (CP.COL_STR64, CP.QOP_STR_RANGES, 4, CP.MAX_QUAL_BYTES)]:
        q = CP.ColQual(typ, op, 0, 1, 0x1000, 0x2000, cb, ob)
        assert lib().strom_column_qual(C.byref(q), 0x3000, 1, 1, 0x4000, 0, 0, 0x5000, None) == -7


def test_limits_accepted_fit_the_kernel():
    """The largest operands that compile stay within the kernel's 64 KiB."""
    ok = [(CP.Pred("c", "ranges", tuple((10 * k, 10 * k + 3) for k in range(2048))), "d16"),
          (CP.Pred("c", "ranges", tuple((10 * k, 10 * k + 3) for k in range(4096))), "i8"),
          (CP.Pred("c", "ranges", tuple((10 * k, 10 * k + 3) for k in range(4096))), "u8"),
          (CP.Pred("c", "ranges", tuple((float(k), k + 0.5) for k in range(4096))), "f8"),
          (CP.Pred("c", "ranges", tuple((b"%03xa" % k, b"%03xz" % k) for k in range(2048))), "s4"),
          (CP.Pred("c", "in", tuple(b"k%07d" % k for k in range(4096))), "s8"),
          (CP.Pred("c", "prefix", [b"k%07d" % k for k in range(4096)]), "s4")]
    for p, dt in ok:
        c = CP.compile_pred(p, G.column(dt))
        total = len(c.consts) + (len(c.offs) if dt in ("s4", "s8") else 0)
        assert total <= 64 << 10, (dt, p.op, total)
    assert total == 64 << 10
    for case in G.limit_cases(np.random.default_rng(18)):
        c = case.compiled
        assert len(c.consts) + (len(c.offs) if case.table.dt == "s4" else 0) == 64 << 10, case.name
