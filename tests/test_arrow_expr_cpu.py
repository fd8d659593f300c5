"""Computed columns of the Arrow scan on the CPU: the expression compiler and
the kernel's numpy twin against pyarrow.compute bit for bit, the library's
host copy of the kernel against the twin word for word, the compiler's and
strom_expr_check's refusals, the host_* queries with expressions against
pyarrow on the table with the computed column appended, and the host copy
under ASan + UBSan."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")
import pyarrow.compute as pc  # noqa: E402

sys.path.insert(0, os.path.dirname(__file__))

import exprgen as XG  # noqa: E402
from exprgen import E, Or, P  # noqa: E402
from nvme_strom_amd.ops import colexpr as X  # noqa: E402
from nvme_strom_amd.utils.arrow_ipc import read_metadata  # noqa: E402


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    import arrowgen
    d = tmp_path_factory.mktemp("expr")
    out = {}
    for codec in XG.CODECS:
        out[codec] = str(d / f"x_{codec}.arrow")
        arrowgen.write(out[codec], XG.table(), codec, batch_rows=700)
    return out


@pytest.fixture(scope="module")
def schema(files):
    return {c.name: c for c in read_metadata(files[None]).schema}


def _columns(tbl, prog):
    vals, oks = [], []
    for n in prog.columns:
        a = tbl.column(n).combine_chunks()
        oks.append(np.asarray(a.is_valid()) if a.null_count else None)
        vals.append(a.fill_null(0).to_numpy(zero_copy_only=False))
    return vals, oks


# ------------------------------------------------------------------ the twin
def test_operators_build_expressions():
    e = (E("a") * 2 + P("b")) // 7
    assert e.key() == ("//", ("+", ("*", ("col", "a"), ("const", 2)), ("col", "b")), 7)
    assert e.columns() == ["a", "b"] and hash(e) == hash((E("a") * 2 + E("b")) // 7)
    assert (1 - P("a")).key() == ("-", ("const", 1), ("col", "a"))
    assert (P("a") * 2 > 5).col.key() == ("*", ("col", "a"), ("const", 2))
    assert abs(-P("a")).key() == ("abs", ("neg", ("col", "a")))
    # comparisons build predicates: they cannot serve as identity
    p = E("a") == E("a")
    assert p.op == "==" and isinstance(p.col, E)
    assert (E("a") + 1.5).isin([1, 2]).op == "in" and E("a").is_null().op == "is_null"
    for bad in (lambda: E("a") // 0, lambda: E("a") % -3, lambda: E("a") // 2.0,
                lambda: E("a") // E("b"), lambda: 5 // E("a"), lambda: 5 % E("a")):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        E("a") + "x"


@pytest.mark.parametrize("label,e,domain", XG.exprs(), ids=[x[0] for x in XG.exprs()])
def test_twin_equals_pyarrow(schema, label, e, domain):
    """host_expr == the pyarrow reference: the bits of every valid row (NaN
    as one NaN) and the validity."""
    tbl = XG.table()
    prog = X.compile_expr(e, schema)
    assert prog.domain == (X.FLT if domain == "float" else X.INT)
    assert prog.column.storage == ("f8" if domain == "float" else "i8")
    vals, oks = _columns(tbl, prog)
    got, ok = X.host_expr(prog, vals, oks, tbl.num_rows)
    want, wok = XG.ref_numpy(tbl, e)
    ok = np.ones(tbl.num_rows, bool) if ok is None else ok
    assert np.array_equal(ok, wok)
    assert np.array_equal(XG.bits(got)[ok], want[ok])
    assert (got[~ok] == 0).all()
    if label == "ratio":
        # the file is built to give inf and NaN here (top orders them)
        assert np.isnan(got[ok]).any() and np.isinf(got[ok]).any()


@pytest.mark.parametrize("col", XG.INT_COLS + XG.FLT_COLS)
def test_every_source_type_widens(schema, col):
    tbl = XG.table()
    for e in (E(col), E(col) + 0.0):
        prog = X.compile_expr(e, schema)
        vals, oks = _columns(tbl, prog)
        got, ok = X.host_expr(prog, vals, oks, tbl.num_rows)
        want, wok = XG.ref_numpy(tbl, e)
        ok = np.ones(tbl.num_rows, bool) if ok is None else ok
        assert np.array_equal(ok, wok) and np.array_equal(XG.bits(got)[ok], want[ok])


def test_compiler_folds_and_describes(schema):
    p = X.compile_expr(E("i32") * (2 + 3) + (10 // 3), schema)
    assert [o[0] for o in p.ops] == [X.XOP_COL, X.XOP_CONST, X.XOP_MUL, X.XOP_CONST, X.XOP_ADD]
    assert [o[2] for o in p.ops if o[0] == X.XOP_CONST] == [5, 3] and p.depth == 2
    assert p.column.kind == "int" and p.column.bit_width == 64 and p.column.signed
    # nullable iff a source has nulls in the file
    nulls = lambda n: n == "i16"
    assert X.compile_expr(E("i32") + E("i16"), schema, nulls).column.nullable
    assert not X.compile_expr(E("i32") + E("i8"), schema, nulls).column.nullable
    # a negative constant is its two's complement, a float one its bits
    assert X.compile_expr(E("i8") + -1, schema).ops[1][2] == 0xFFFFFFFFFFFFFFFF
    assert X.compile_expr(E("i8") + 1.0, schema).ops[1][2] == 0x3FF0000000000000
    assert X.compile_expr(E("i8") / 2, schema).domain == X.FLT


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("col,what", [("u64", "uint64"), ("b", "bool"), ("dec", "decimal"),
                                      ("s", "utf8"), ("ts", "timestamp"),
                                      ("dict", "dictionary-encoded")])
def test_refused_source_columns(schema, col, what):
    with pytest.raises(ValueError, match=what):
        X.compile_expr(E(col) + 1, schema)


def test_refused_unknown_column(schema):
    with pytest.raises(ValueError, match="nope"):
        X.compile_expr(E("nope") + 1, schema)


def test_refused_too_many_columns(schema):
    with pytest.raises(ValueError, match="5 source columns"):
        X.compile_expr(E("i8") + E("i16") + E("i32") + E("i64") + E("u8"), schema)


def test_refused_too_many_ops(schema):
    e = E("i8")
    for k in range(8):
        e = e * E("i16")
    with pytest.raises(ValueError, match="17 ops"):
        X.compile_expr(e, schema)
    e = E("i8")
    for k in range(7):
        e = e * E("i16")
    assert len(X.compile_expr(abs(e), schema).ops) == 16


def test_refused_depth(schema):
    e = E("i8")
    for k in range(8):
        e = E("i16") - e                 # the deeper operand on the right: 9 pushes first
    with pytest.raises(ValueError, match="depth 9"):
        X.compile_expr(e, schema)
    e = E("i8")
    for k in range(7):
        e = E("i16") - e
    assert X.compile_expr(e, schema).depth == 8


def test_refused_integer_division_in_float_domain(schema):
    for e in (E("f32") // 2, (E("i8") + 0.5) % 3, (E("i8") / 2) // 3):
        with pytest.raises(ValueError, match="integer operations"):
            X.compile_expr(e, schema)


def test_refused_constant_outside_int64(schema):
    with pytest.raises(ValueError, match="outside int64"):
        X.compile_expr(E("i64") + (1 << 63), schema)
    with pytest.raises(ValueError, match="outside int64"):
        X.compile_expr(E("i64") + (1 << 62) * 2, schema)      # after folding
    assert X.compile_expr(E("i64") + -(1 << 63), schema).ops[1][2] == 1 << 63
    with pytest.raises(ValueError, match="at least one column"):
        X.compile_expr(E._of(("const", 3)), schema)


def _struct(domain, types, ops):
    s = X.ExprStruct()
    s.domain, s.nops, s.ncols = domain, len(ops), len(types)
    for i, t in enumerate(types[:X.MAX_COLS]):
        s.col_type[i] = t
    for i, (op, arg, imm) in enumerate(ops[:X.MAX_OPS]):
        s.ops[i].op, s.ops[i].arg, s.ops[i].imm = op, arg, imm & 0xFFFFFFFFFFFFFFFF
    return s


def test_expr_check_refusals():
    """strom_expr_check through ctypes: every rule of strom.h."""
    from nvme_strom_amd import _native as N
    chk = lambda *a: N.lib().strom_expr_check(C.byref(_struct(*a)))
    I4, F8, U8 = X.COL_CODE["i4"], X.COL_CODE["f8"], X.COL_CODE["u8"]
    col, const = (X.XOP_COL, 0, 0), (X.XOP_CONST, 0, 1)
    assert chk(X.INT, [I4], [col]) == 0
    assert chk(X.INT, [I4], [col, const, (X.XOP_ADD, 0, 0), (X.XOP_MOD, 0, 7)]) == 0
    assert chk(X.FLT, [I4, F8], [col, (X.XOP_COL, 1, 0), (X.XOP_DIV, 0, 0)]) == 0
    assert chk(X.INT, [], [const]) == 0
    bad = [
        (X.INT, [I4], [col, (0, 0, 0)]),                              # unknown opcode
        (X.INT, [I4], [col, (11, 0, 0)]),
        (X.INT, [I4], [(X.XOP_NEG, 0, 0)]),                           # underflow
        (X.INT, [I4], [col, (X.XOP_ADD, 0, 0)]),
        (X.INT, [I4], [col] * 9 + [(X.XOP_ADD, 0, 0)] * 7),           # overflow
        (X.INT, [I4], [col, col]),                                    # final depth 2
        (X.INT, [I4], []),                                            # no ops
        (X.INT, [I4], [(X.XOP_COL, 1, 0)]),                           # column index
        (X.INT, [I4], [col] + [(X.XOP_NEG, 0, 0)] * 16),              # 17 ops
        (X.INT, [I4] * 5, [col]),                                     # 5 columns
        (X.INT, [U8], [col]),                                         # source types
        (X.INT, [X.COL_CODE["b1"]], [col]),
        (X.INT, [0], [col]),
        (X.INT, [F8], [col]),                                         # float source, int domain
        (X.INT, [I4], [col, col, (X.XOP_DIV, 0, 0)]),                 # DIV in the int domain
        (X.FLT, [I4], [col, (X.XOP_FDIV, 0, 3)]),                     # FDIV / MOD in the float
        (X.FLT, [I4], [col, (X.XOP_MOD, 0, 3)]),
        (X.INT, [I4], [col, (X.XOP_FDIV, 0, 0)]),                     # divisor <= 0
        (X.INT, [I4], [col, (X.XOP_MOD, 0, -1)]),
        (2, [I4], [col]),                                             # domain
    ]
    for b in bad:
        assert chk(*b) == -22, b
    assert N.lib().strom_expr_check(None) == -22


# ------------------------------------------------------------------ the host copy
@pytest.mark.parametrize("nulls", ["none", "one", "some"])
def test_host_copy_equals_twin(nulls):
    """strom_column_expr_host (the kernel's walk, compiled for the CPU) ==
    host_expr word for word: values where valid, validity words everywhere,
    the prefill everywhere else and in the guards; every selection kind."""
    from nvme_strom_amd import _native as N
    from nvme_strom_amd.utils.arrow_ipc import Column
    kinds = {"i1": ("int", 8, True), "i2": ("int", 16, True), "i4": ("int", 32, True),
             "i8": ("int", 64, True), "u1": ("int", 8, False), "u2": ("int", 16, False),
             "u4": ("int", 32, False), "f4": ("float", 32, True), "f8": ("float", 64, True)}
    sch = [Column(n, *k) for n, k in kinds.items()]
    progs = [E("i1") * E("i2") - E("u4") // 7, (E("i8") % (1 << 40)) + abs(-E("i4")) * E("u1"),
             E("f4") * E("f8") + E("i8") / E("u2"), abs(E("f8")) - -E("i4") * 0.5]
    for seed, e in enumerate(progs):
        prog = X.compile_expr(e, sch)
        case = XG.case_of(prog.columns, nulls=nulls, seed=seed)
        for label, sel in XG.selections(case.nwords, seed):
            vals, valid = case.out_buffers()
            src, out = case.tables([v.ctypes.data for v in case.vals],
                                   [w.ctypes.data for w in case.vwords], vals.ctypes.data,
                                   valid.ctypes.data)
            st = prog.struct()
            rc = N.lib().strom_column_expr_host(C.byref(st), src.ctypes.data, len(case.rows),
                                                case.nwords,
                                                sel.ctypes.data if sel is not None else None,
                                                out.ctypes.data)
            assert rc == 0
            wv, wk = case.expected(prog, X.host_expr, sel)
            assert np.array_equal(valid, wk), (e, label)
            assert np.array_equal(vals, wv), (e, label)


# ------------------------------------------------------------------ whole queries
def _host(files, codec):
    from functools import partial
    from nvme_strom_amd.models import arrow_scan as S
    meta, dicts = read_metadata(files[codec]), {}
    kw = dict(meta=meta, dicts=dicts)

    class Q:
        aggregate = staticmethod(partial(S.host_aggregate, files[codec], **kw))
        scan_where = staticmethod(partial(S.host_scan_where, files[codec], **kw))
        top = staticmethod(partial(S.host_top, files[codec], **kw))
    return Q


@pytest.mark.parametrize("codec", XG.CODECS)
def test_host_aggregate_of_expressions(files, codec):
    from nvme_strom_amd.models.arrow_scan import HashBy
    tbl, Q = XG.table(), _host(files, codec)
    every = np.ones(tbl.num_rows, bool)
    fns = ("count", "sum", "min", "max", "mean")
    for label, e, _ in XG.exprs():
        ref = XG.reference(tbl, e)
        out = Q.aggregate([], [(fn, e) for fn in fns])
        for fn in fns:
            XG.check_agg(out, fn, e, ref, every, (label, codec))
        assert out.rows == tbl.num_rows and [p.expr.key() for p in out.exprs] == [e.key()]
    # under a qualifier on a stored column, keyed by name
    e = E("price") * (1 - E("disc"))
    ref = XG.reference(tbl, e)
    m = XG.mask_of(tbl, pc.less(tbl.column("qty"), 30))
    out = Q.aggregate([P("qty") < 30], [("sum", e), ("count", e), ("max", e), ("sum", "qty")],
                      by="i8")
    XG.check_grouped(out, tbl, ["i8"], e, ref, m, ("count", "sum", "max"), codec)
    # by=HashBy(expression), and a composite key with a declared width
    sec = E("ts_ms") // 1000
    val = E("i32") * E("i16") + E("i8")
    t2 = XG.with_column(tbl, "sec", sec)
    out = Q.aggregate([], [("sum", val), ("count", val), ("min", val)], by=HashBy(sec, 256))
    XG.check_grouped(out, t2, ["sec"], val, XG.reference(tbl, val), every,
                     ("count", "sum", "min"), codec)
    assert len(out.keys) > 50 and len(out.exprs) == 2
    m5 = E("i32") % 5
    t3 = XG.with_column(tbl, "m5", m5)
    out = Q.aggregate([], [("sum", e), ("count", None)], by=HashBy([m5, "i8"], 4096, bits={m5: 4}))
    XG.check_grouped(out, t3, ["m5", "i8"], e, ref, every, ("sum",), codec)


@pytest.mark.parametrize("codec", XG.CODECS)
def test_host_scan_where_and_top_of_expressions(files, codec):
    tbl, Q = XG.table(), _host(files, codec)
    a = E("i32") + E("i16")
    ra = XG.reference(tbl, a)
    ratio = E("f64") / E("i8")
    rr = XG.reference(tbl, ratio)
    cases = [
        ([a < 100], pc.less(ra, 100)),
        ([a.between(-1000, 1000), P("i8") >= 0],
         pc.and_(pc.and_(pc.greater_equal(ra, -1000), pc.less_equal(ra, 1000)),
                 pc.greater_equal(tbl.column("i8"), 0))),
        ([Or(a * 2 > 1 << 31, P("i8") < -100)],
         pc.or_kleene(pc.greater(XG.reference(tbl, a * 2), 1 << 31),
                      pc.less(tbl.column("i8"), -100))),
        ([a.isin([0, 1, -1, 77])], pc.is_in(ra, value_set=pa.array([0, 1, -1, 77]))),
        ([a.not_in([0, 1])], pc.and_(pc.invert(pc.is_in(ra, value_set=pa.array([0, 1]))),
                                     pc.is_valid(ra))),
        ([a.ranges([(-50, 50), (1000, 2000)])],
         pc.or_(pc.and_(pc.greater_equal(ra, -50), pc.less_equal(ra, 50)),
                pc.and_(pc.greater_equal(ra, 1000), pc.less_equal(ra, 2000)))),
        ([a.is_null()], pc.is_null(ra)),
        ([a.is_valid(), ratio > 0.5], pc.and_(pc.is_valid(ra), pc.greater(rr, 0.5))),
        ([ratio != 0.0], pc.not_equal(rr, 0.0)),
    ]
    for quals, want in cases:
        m = XG.mask_of(tbl, want)
        out = Q.scan_where(quals, project=ratio)
        assert np.array_equal(out.indices, np.flatnonzero(m)), quals
        wv, wok = XG.ref_numpy(tbl, ratio)
        ok = np.ones(len(out.indices), bool) if out.valid is None else out.valid
        assert np.array_equal(ok, wok[m])
        assert np.array_equal(XG.bits(out.values)[ok], wv[m][ok])
    # ORDER BY an expression: NaN after the values, nulls last, both directions
    m = XG.mask_of(tbl, pc.greater(tbl.column("qty"), 5))
    for e, ref in ((ratio, rr), (a, ra)):
        for desc in (False, True):
            for k in (1, 50, 2900):
                out = Q.top([P("qty") > 5], e, k, desc, project=a)
                want = XG.top_reference(ref, m, desc, k)
                assert out.rows.tolist() == want.tolist(), (e, desc, k)
                wv, wok = XG.ref_numpy(tbl, e)
                ok = np.ones(len(want), bool) if out.valid is None else out.valid
                assert np.array_equal(ok, wok[want])
                assert np.array_equal(XG.bits(out.values)[ok], wv[want][ok])
                pv, pok = XG.ref_numpy(tbl, a)
                assert np.array_equal(XG.bits(out.projected)[pok[want]], pv[want][pok[want]])
    out = Q.top([], ratio, 2900, True)
    assert np.isnan(out.values).any() and not out.valid.all()


def test_shared_expression_is_compiled_once(files):
    Q = _host(files, None)
    e = E("i32") * E("i16")
    out = Q.aggregate([e > 0, (E("i32") * E("i16")).is_valid()],
                      [("sum", E("i32") * E("i16")), ("max", e), ("sum", e + 1)])
    assert [p.expr.key() for p in out.exprs] == [e.key(), (e + 1).key()]
    assert out.get("sum", e)[0] == out.get("sum", E("i32") * E("i16"))[0]
    # at most four distinct expressions per scan
    with pytest.raises(ValueError, match="more than 4"):
        Q.aggregate([], [("sum", E("i8") + k) for k in range(5)])


def test_query_refusals(files):
    from nvme_strom_amd.models.arrow_scan import HashBy, Join, JoinTable
    Q = _host(files, None)
    with pytest.raises(NotImplementedError, match="by=HashBy"):
        Q.aggregate([], [("count", None)], by=E("i8") + 1)
    with pytest.raises(NotImplementedError, match="join key"):
        Join(E("fk") + 1, JoinTable(np.arange(4)))
    with pytest.raises(NotImplementedError, match="float"):
        Q.aggregate([], [("count", None)], by=HashBy(E("f32") * 2, 16))
    with pytest.raises(ValueError, match="uint64"):
        Q.aggregate([], [("sum", E("u64") + 1)])
    with pytest.raises(ValueError, match="timestamp"):
        Q.top([], E("ts") + 1, 3)
    with pytest.raises(ValueError, match="nope"):
        Q.scan_where([E("nope") + 1 > 0])
    with pytest.raises(ValueError, match="bits="):
        HashBy([E("i8") % 3, "i16"], 16, bits={E("i8") % 5: 3})


# ------------------------------------------------------------------ sanitizer
def test_colexpr_fuzz_asan():
    """Random valid programs over random batches through the host copy of the
    kernel built with ASan + UBSan (csrc/tests/colexpr_fuzz.cc) against a plain
    scalar evaluation, and random malformed programs, which strom_expr_check
    refuses and the walk never evaluates: exits 0."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if shutil.which("make") is None or not (
            os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))):
        pytest.skip("no make / hipcc")
    r = subprocess.run(["make", "-s", "build/colexpr_fuzz"], cwd=root, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([os.path.join(root, "build", "colexpr_fuzz"), "1500"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "1500 cases ok" in r.stdout
