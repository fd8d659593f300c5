"""ORDER BY on several columns without a GPU: the numpy twin of the sort
against ``pyarrow.compute.sort_indices`` (default null placement), the
kernels' C++ host copies against the twin, ``host_scan_where(order_by=...)``
against pyarrow's filter / sort / take, every refusal, and the ASan/UBSan
fuzzer of the host copies.  Every comparison is exact: the order is total."""
import os
import subprocess
import sys

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")
import pyarrow.compute as pc  # noqa: E402

sys.path.insert(0, os.path.dirname(__file__))

import sortgen as SG  # noqa: E402
from sortgen import G  # noqa: E402
from nvme_strom_amd.ops import colsort as SO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pa_order(names, columns):
    tbl = SG.arrow_table(names, columns)
    return np.asarray(pc.sort_indices(tbl, sort_keys=SG.sort_keys_of(names, columns)))


# ------------------------------------------------------------------- twin
@pytest.mark.parametrize("n", [0, 1, 65, SG.TILE + 1])
def test_twin_equals_pyarrow_every_shape(n):
    for label, v, ok in SG.key_cases(n):
        for desc in (False, True):
            cols = [(v, ok, desc)]
            assert np.array_equal(SO.host_order(cols, n), _pa_order(["k"], cols)), (label, desc)


@pytest.mark.parametrize("nkeys", [1, 2, 3, 4])
def test_twin_equals_pyarrow_tied_columns(nkeys):
    n = 20_000
    cols = SG.tied_columns(nkeys, n)
    names = [f"k{i}" for i in range(nkeys)]
    got = SO.host_order(cols, n)
    assert np.array_equal(got, _pa_order(names, cols))
    # ties are real: every column has few distinct values, so the later keys
    # and the file order decide most positions
    assert all(len(np.unique(c[0].view(f"u{c[0].dtype.itemsize}"))) <= 16 for c in cols)
    # every direction flipped
    flip = [(v, ok, not d) for v, ok, d in cols]
    assert np.array_equal(SO.host_order(flip, n), _pa_order(names, flip))


def test_twin_of_the_issue():
    """An int8 key of six values with 10 % nulls, descending, then a float32
    key with NaN, +-0.0 and 10 % nulls, ascending, at 200,000 rows."""
    n = 200_000
    cols = SG.tied_columns(2, n, seed=1)
    assert cols[0][2] and not cols[1][2] and cols[0][0].dtype == np.int8
    assert np.array_equal(SO.host_order(cols, n), _pa_order(["x", "y"], cols))


# -------------------------------------------------------------- host copy
@pytest.mark.parametrize("n", SG.SIZES)
def test_host_copy_equals_twin(n):
    for label, v, ok in SG.key_cases(n):
        for desc in (False, True):
            cols = [(v, ok, desc)]
            got = SO.native_host_order(cols, n)
            assert np.array_equal(got, SO.host_order(cols, n)), (label, desc)
            if label == "equal":
                assert np.array_equal(got, np.arange(n))


@pytest.mark.parametrize("nkeys", [2, 3, 4])
def test_host_copy_tied_columns(nkeys):
    n = 30_000
    cols = SG.tied_columns(nkeys, n)
    assert np.array_equal(SO.native_host_order(cols, n), SO.host_order(cols, n))


def test_passes_and_state_size():
    c = SO.TYPE_CODE
    assert [SO.passes(c[t], False) for t in ("i1", "u2", "i4", "u8", "f4", "f8")] == \
        [1, 2, 4, 8, 5, 9]
    assert SO.passes(c["i4"], True) == 5
    assert SO.work_bytes(0) == 1024 and SO.work_bytes(3 * SO.TILE + 17) == 5 * 1024


def test_host_apply_every_kind():
    rng = np.random.default_rng(2)
    n = 500
    perm = rng.permutation(n)
    v = rng.integers(0, 1 << 62, (n, 2))
    ok = (rng.random(n) < 0.8).astype(np.uint8)
    got, gok, goff = SO.host_apply(perm, 10, 50, v, ok)
    assert goff is None and np.array_equal(got, v[perm[10:60]]) and \
        np.array_equal(gok, ok[perm[10:60]])
    strs = [bytes(rng.integers(65, 91, int(k)).astype(np.uint8)) for k in rng.integers(0, 7, n)]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in strs])])
    chars = np.frombuffer(b"".join(strs), np.uint8)
    for first, count in ((0, n), (7, 20), (n, 0), (n - 3, 3)):
        got, _, goff = SO.host_apply(perm, first, count, chars, None, offs)
        want = [strs[i] for i in perm[first:first + count]]
        assert [bytes(got[goff[i]:goff[i + 1]]) for i in range(count)] == want
        assert len(goff) == count + 1


# ------------------------------------------------------------ whole scans
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from arrowgen import write
    tbl = G.table(3000)
    d = tmp_path_factory.mktemp("sort")
    paths = {}
    for codec in (None, "lz4"):
        paths[codec] = str(d / f"sort_{codec}.arrow")
        write(paths[codec], tbl, codec, batch_rows=700)
    return tbl, paths


def _reference(ftbl, mask, names, order_by, limit=None, offset=0):
    sel = ftbl.filter(mask)
    idx = pc.sort_indices(sel, sort_keys=SG.pa_sort_keys(order_by))
    rows = np.flatnonzero(np.asarray(mask.combine_chunks().fill_null(False)))
    want = SG.cut(sel.take(idx).select(names), limit, offset)
    ids = rows[np.asarray(idx)]
    off = min(offset, len(ids))
    return want, ids[off:] if limit is None else ids[off:off + limit]


@pytest.mark.parametrize("codec", [None, "lz4"])
def test_host_scan_order_equals_pyarrow(files, codec):
    from nvme_strom_amd.models.arrow_scan import host_scan_where
    tbl, paths = files
    quals, mask_of = G.quals_and_mask()
    ftbl = pa.ipc.open_file(paths[codec]).read_all()
    mask = mask_of(ftbl)
    for names, order_by in SG.ORDERS:
        for limit, offset in SG.WINDOWS:
            out = host_scan_where(paths[codec], quals, project=names, order_by=order_by,
                                  limit=limit, offset=offset)
            want, ids = _reference(ftbl, mask, names, order_by, limit, offset)
            assert [c.name for c in out.columns] == names
            G.same_table(out.to_arrow(), want)
            assert np.array_equal(out.indices, ids)
            assert out.order == [(k, d == "descending") for k, d in SG.pa_sort_keys(order_by)]
    # nothing ordered: file order, order None
    out = host_scan_where(paths[codec], quals, project=["i8"])
    assert out.order is None and np.array_equal(out.indices, np.sort(out.indices))
    # an empty selection and an empty batch range
    from nvme_strom_amd.ops.colpred import P
    for kw in (dict(quals=[P("f64") > 2.0]), dict(quals=quals, batches=(2, 2))):
        out = host_scan_where(paths[codec], kw["quals"], project=["s", "i8"], order_by=["u8", "i8"],
                              batches=kw.get("batches"), limit=4)
        assert len(out.indices) == 0 and len(out.columns) == 2
        G.same_table(out.to_arrow(), ftbl.slice(0, 0).select(["s", "i8"]))


def test_host_scan_order_expression_and_attributes(files):
    from nvme_strom_amd.models.arrow_scan import Join, JoinTable, StarJoin, host_scan_where
    from nvme_strom_amd.ops.colexpr import E, name_of
    tbl, paths = files
    quals, mask_of = G.quals_and_mask()
    ftbl = pa.ipc.open_file(paths[None]).read_all()
    dims = G.dimensions()
    jt = {fk: JoinTable(keys, attrs=attrs) for fk, (keys, attrs) in dims.items()}
    expr, ratio = E("i64") * 2 + E("i8"), E("f64") / E("f32")
    sj = StarJoin(Join("fa", jt["fa"]), Join("fb", jt["fb"]))
    out = host_scan_where(paths[None], quals, project=[jt["fb"]["grp"], "s", expr, jt["fa"]["cat"]],
                          join=sj, order_by=[("u8", "descending"), (ratio, "ascending"), expr],
                          limit=40, offset=3)
    fa, fb = ftbl.column("fa"), ftbl.column("fb")
    mask = pc.and_kleene(mask_of(ftbl), pc.and_kleene(
        pc.is_in(fa, value_set=pa.array(dims["fa"][0], pa.int32())),
        pc.is_in(fb, value_set=pa.array(dims["fb"][0].astype(np.uint16)))))
    sel = ftbl.filter(mask)
    ev = pc.add(pc.multiply(sel.column("i64"), 2), pc.cast(sel.column("i8"), pa.int64()))
    rv = pc.divide(sel.column("f64"), pc.cast(sel.column("f32"), pa.float64()))
    sel = sel.append_column("e", ev).append_column("r", rv)
    idx = pc.sort_indices(sel, sort_keys=[("u8", "descending"), ("r", "ascending"),
                                          ("e", "ascending")])
    want = sel.take(idx).slice(3, 40)
    assert want.num_rows == 40
    got = out.to_arrow()
    assert got.schema.names == ["grp", "s", str(name_of(expr)), "cat"]
    assert got.column("s").equals(want.column("s"))
    assert got.column(str(name_of(expr))).equals(want.column("e"))
    cat = dict(zip(dims["fa"][0].tolist(), dims["fa"][1]["cat"]))
    grp = dict(zip(dims["fb"][0].tolist(), dims["fb"][1]["grp"]))
    assert got.column("cat").to_pylist() == [cat[k] for k in want.column("fa").to_pylist()]
    assert got.column("grp").to_pylist() == [grp[k] for k in want.column("fb").to_pylist()]
    assert out.order == [("u8", True), (str(name_of(ratio)), False), (str(name_of(expr)), False)]


def test_refusals(files):
    from nvme_strom_amd.models.arrow_scan import Join, JoinTable, host_scan_where
    from nvme_strom_amd.ops.colexpr import E
    tbl, paths = files
    path = paths[None]
    quals, _ = G.quals_and_mask()
    scan = lambda **kw: host_scan_where(path, quals, **kw)
    # kinds that are not ordered, named
    for name, kind in (("s", "utf8"), ("ls", "utf8"), ("bin", "binary"), ("b", "bool"),
                       ("dec", "decimal"), ("dict", "dictionary-encoded"),
                       ("idict", "dictionary-encoded")):
        with pytest.raises(NotImplementedError, match=f"ORDER BY {name}: {kind}"):
            scan(project=["i8"], order_by=name)
        with pytest.raises(NotImplementedError, match=f"ORDER BY {name}: {kind}"):
            scan(project=["i8", name], order_by=[("i8", "descending"), name])
    dims = G.dimensions()
    dim = JoinTable(dims["fa"][0], attrs=dims["fa"][1])
    for ob in (dim["cat"], [dim["cat"]], ["i8", (dim["cat"], "descending")]):
        with pytest.raises(NotImplementedError, match="dim\\[attr\\]"):
            scan(project=["i8", dim["cat"]], order_by=ob, join=Join("fa", dim))
    with pytest.raises(ValueError, match="twice"):
        scan(project=["i8"], order_by=["i8", ("i8", "descending")])
    with pytest.raises(ValueError, match="twice"):
        scan(project=["i8"], order_by=[E("i8") + 1, E("i8") + 1])
    with pytest.raises(ValueError, match="1 to 4"):
        scan(project=["i8"], order_by=["i8", "i16", "i32", "i64", "u8"])
    with pytest.raises(ValueError, match="1 to 4"):
        scan(project=["i8"], order_by=[])
    with pytest.raises(ValueError, match="'ascending' or 'descending'"):
        scan(project=["i8"], order_by=[("i8", "down")])
    with pytest.raises(TypeError):
        scan(project=["i8"], order_by=[5])
    with pytest.raises(ValueError, match="no column"):
        scan(project=["i8"], order_by="nope")
    # the list form of project
    for project in (None, "i8"):
        with pytest.raises(ValueError, match="list form of project"):
            scan(project=project, order_by="i8")
    # limit / offset
    for kw in (dict(limit=5), dict(offset=2), dict(limit=0)):
        with pytest.raises(ValueError, match="need order_by"):
            scan(project=["i8"], **kw)
    for kw in (dict(limit=-1), dict(offset=-1), dict(limit=1.5), dict(offset="3"),
               dict(limit=True)):
        with pytest.raises(ValueError, match="non-negative int"):
            scan(project=["i8"], order_by="i8", **kw)
    # visible and hidden items within 16, expressions within four
    names = [c for c in tbl.schema.names if c not in ("fa", "fb")][:16]
    hidden = [c for c in ("fa", "fb")]
    with pytest.raises(NotImplementedError, match="at most 16"):
        scan(project=names, order_by=hidden)
    out = scan(project=names[:15], order_by=["fa", names[0]], limit=3)
    assert len(out.columns) == 15 and len(out.indices) == 3
    with pytest.raises(ValueError, match="more than 4 computed"):
        scan(project=[E("i8") + k for k in range(3)], order_by=[E("i8") * 7, E("i16") * 7])
    # the multi-rank scan
    from nvme_strom_amd.parallel import scan as PS
    for kw in (dict(order_by="i8"), dict(limit=3), dict(offset=1)):
        with pytest.raises(NotImplementedError, match="merging sorted results"):
            PS.DistributedArrowScan.scan_where(object(), quals, project="i8", **kw)
    # gather descriptors
    with pytest.raises(ValueError):
        SO.sort_cols([(SO.FIXED, 8, 8, 8, 0, 0)] * 17)
    with pytest.raises(ValueError):
        SO.sort_cols([(SO.FIXED, 3, 8, 8, 0, 0)])
    with pytest.raises(ValueError):
        SO.sort_cols([(7, 8, 8, 8, 0, 0)])


# ----------------------------------------------------------------- fuzzer
def test_fuzzer_builds_and_runs():
    exe = os.path.join(ROOT, "build", "colsort_fuzz")
    subprocess.run(["make", "-C", ROOT, "build/colsort_fuzz"], check=True, capture_output=True)
    r = subprocess.run([exe, "600", "11"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "600 iterations ok" in r.stdout
