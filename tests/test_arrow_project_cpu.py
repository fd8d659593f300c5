"""The select list (``project=[...]``) without a GPU: the numpy twin of the
emit kernel against a per-row loop, the kernel's C++ host copy against the
twin on the GPU tests' cases, ``host_scan_where(project=[...])`` against
pyarrow's filtered select, every refusal, and the ASan/UBSan fuzzer of the
host copy."""
import os
import subprocess
import sys

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")

sys.path.insert(0, os.path.dirname(__file__))

import projgen as G  # noqa: E402
from nvme_strom_amd.ops import colproject as PJ  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------- twin
def _loop(case: G.Case):
    """The selection row by row, bit by bit."""
    ids = []
    outs = [dict(vals=[], valid=[], starts=[], chars=bytearray()) for _ in case.cols]
    bt = case.batches
    for w in range(case.nwords):
        b = -1
        for k in range(len(bt)):
            if bt[k][3] <= w:
                b = k
        if b < 0:
            continue
        word = int(case.bitmap[w])
        for bit in range(64):
            r = (w - int(bt[b][3])) * 64 + bit
            if not (word >> bit) & 1 or r >= bt[b][2]:
                continue
            ids.append(int(bt[b][4]) + r)
            for c, o in zip(case.cols, outs):
                vb = c.valid[b]
                o["valid"].append(1 if vb is None else (int(vb[r >> 3]) >> (r & 7)) & 1)
                v = c.values[b]
                if c.kind == PJ.FIXED:
                    o["vals"].append(bytes(v[r * c.width:(r + 1) * c.width]))
                elif c.kind == PJ.BOOL:
                    o["vals"].append(bytes([(int(v[r >> 3]) >> (r & 7)) & 1]))
                else:
                    ow = 8 if c.kind == PJ.STR64 else 4
                    a = int.from_bytes(bytes(v[r * ow:(r + 1) * ow]), "little", signed=True)
                    e = int.from_bytes(bytes(v[(r + 1) * ow:(r + 2) * ow]), "little", signed=True)
                    o["starts"].append(len(o["chars"]))
                    if 0 <= a <= e <= len(c.aux[b]):
                        o["chars"] += bytes(c.aux[b][a:e])
    return ids, outs


def test_twin_equals_row_loop():
    rng = np.random.default_rng(3)
    rows = (1, 65, 300, 0, 130)
    bt = G.batch_table(rows, gaps=[0, 1, 0, 0, 2])
    nw = G.nwords_of(bt) + 2
    for kind in G.BITMAPS:
        cols, want = G.mixed_cols(8, rows, rng)
        case = G.Case(kind, G.bitmap(kind, nw, rng), bt, cols, want)
        ids, outs = PJ.host_rows_multi(case.bitmap, case.batches, case.cols)
        lids, louts = _loop(case)
        assert ids.tolist() == lids, kind
        for c, o, lo in zip(cols, outs, louts):
            assert o.valid.tolist() == lo["valid"], kind
            if PJ.is_str(c.kind):
                assert o.values.tolist() == lo["starts"] and bytes(o.chars) == bytes(lo["chars"])
            else:
                assert bytes(np.ascontiguousarray(o.values)) == b"".join(lo["vals"]), kind
    # a string column's malformed pairs really are in the selection
    case = G.Case("all", G.bitmap("all", nw, rng), bt, [G.str_col(False, rows, rng)], [False])
    _, (o,) = PJ.host_rows_multi(case.bitmap, case.batches, case.cols)
    offs = case.cols[0].values[2].view("<i4").astype(np.int64)
    assert ((offs[:-1] < 0) | (offs[1:] < offs[:-1]) | (offs[1:] > len(case.cols[0].aux[2]))).any()
    assert len(o.values) == sum(rows)


# -------------------------------------------------------------- host copy
def test_host_copy_equals_twin():
    """The C++ walk, bit for bit, on the cases the kernel is tested with."""
    be = G.HostBackend()
    for case in G.kernel_cases(np.random.default_rng(7)):
        G.run_and_check(be, [case], total0=3, cur0=5)


def test_host_copy_appends_behind_odd_cursors():
    rng = np.random.default_rng(9)
    rows = G.ROWS3
    bt = G.batch_table(rows)
    nw = G.nwords_of(bt)
    cases = []
    for kind in ("d2", "one_per_word"):
        cols, want = G.mixed_cols(7, rows, rng)
        cases.append(G.Case(kind, G.bitmap(kind, nw, rng), bt, cols, want))
    t0 = 1 - len(PJ.host_rows_multi(cases[0].bitmap, cases[0].batches, cases[0].cols)[0]) % 2
    mid = G.run_and_check(G.HostBackend(), cases[:1], total0=t0, cur0=1)
    assert mid["rows"] % 2 == 1
    end = G.run_and_check(G.HostBackend(), cases, total0=t0, cur0=1)
    assert end["rows"] > mid["rows"]


def test_host_copy_refusals():
    one = np.ones(1, np.uint64)
    bt = G.batch_table((10,))
    out, tot = np.zeros(16, np.int64), np.zeros(1, np.int64)
    vals = np.zeros(16, np.int64)
    tabs = np.zeros((1, 1, 7), np.int64)
    col = (PJ.FIXED, 8, vals.ctypes.data, 0, 0, 0)

    def call(cols, tables=tabs, nwords=1):
        return PJ.rows_multi_host(one, nwords, bt, out, tot, cols, tables)
    assert call(PJ.proj_cols([col]), nwords=0) == 0
    assert call(np.zeros(0, PJ.PROJ_COL)) == -22
    many = np.zeros(17, PJ.PROJ_COL)
    many[:] = PJ.proj_cols([col])[0]
    assert call(many, np.zeros((17, 1, 7), np.int64)) == -22
    for kind, width in ((0, 8), (5, 8), (PJ.FIXED, 3), (PJ.FIXED, 0), (PJ.FIXED, 32)):
        bad = PJ.proj_cols([col])
        bad["kind"], bad["width"] = kind, width
        assert call(bad) == -22, (kind, width)
    bad = PJ.proj_cols([col])
    bad["out"] += 4                                  # an 8-byte column at an odd word
    assert call(bad) == -22
    bad = PJ.proj_cols([col])
    bad["kind"] = PJ.STR32                           # no character output, no cursor
    assert call(bad) == -22
    assert tot[0] == 0
    with pytest.raises(ValueError):
        PJ.proj_cols([])
    with pytest.raises(ValueError):
        PJ.proj_cols([col] * 17)
    with pytest.raises(ValueError):
        PJ.proj_cols([(PJ.FIXED, 3, 8, 0, 0, 0)])


# ------------------------------------------------------------ whole scans
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from arrowgen import write
    tbl = G.table(3000)
    d = tmp_path_factory.mktemp("proj")
    paths = {}
    for codec in (None, "lz4", "zstd"):
        paths[codec] = str(d / f"proj_{codec}.arrow")
        write(paths[codec], tbl, codec, batch_rows=700)
    return tbl, paths


@pytest.mark.parametrize("codec", [None, "lz4", "zstd"])
def test_host_scan_select_equals_pyarrow(files, codec):
    from nvme_strom_amd.models.arrow_scan import host_scan_where
    tbl, paths = files
    quals, mask_of = G.quals_and_mask()
    ftbl = pa.ipc.open_file(paths[codec]).read_all()
    mask = mask_of(ftbl)
    for names in G.SELECTS:
        out = host_scan_where(paths[codec], quals, project=names)
        want = G.reference(ftbl, mask, names)
        assert 0 < want.num_rows < tbl.num_rows
        assert [c.name for c in out.columns] == names
        assert out.values is None and out.valid is None
        G.same_table(out.to_arrow(), want)
        assert np.array_equal(out.indices, np.flatnonzero(np.asarray(mask.combine_chunks()
                                                                     .fill_null(False))))
    # a tuple is the list form; a list of one is still a list
    out = host_scan_where(paths[codec], quals, project=("u16",))
    assert len(out.columns) == 1 and out.columns[0].values.dtype == np.uint16
    # an empty selection and an empty batch range
    from nvme_strom_amd.ops.colpred import P
    for kw in (dict(quals=[P("f64") > 2.0]), dict(quals=quals, batches=(2, 2))):
        out = host_scan_where(paths[codec], kw["quals"], project=G.SELECTS[1],
                              batches=kw.get("batches"))
        assert len(out.indices) == 0
        G.same_table(out.to_arrow(), ftbl.slice(0, 0).select(G.SELECTS[1]))


def test_host_scan_select_expression_and_attributes(files):
    import pyarrow.compute as pc
    from nvme_strom_amd.models.arrow_scan import Join, JoinTable, StarJoin, host_scan_where
    from nvme_strom_amd.ops.colexpr import E, name_of
    tbl, paths = files
    quals, mask_of = G.quals_and_mask()
    ftbl = pa.ipc.open_file(paths[None]).read_all()
    dims = G.dimensions()
    jt = {fk: JoinTable(keys, attrs=attrs) for fk, (keys, attrs) in dims.items()}
    expr = E("i64") * 2 + E("i8")
    ename = str(name_of(expr))
    sj = StarJoin(Join("fa", jt["fa"]), Join("fb", jt["fb"]))
    out = host_scan_where(paths[None], quals, project=[jt["fb"]["grp"], "s", expr,
                                                       jt["fa"]["cat"]], join=sj)
    fa, fb = ftbl.column("fa"), ftbl.column("fb")
    mask = pc.and_kleene(mask_of(ftbl), pc.and_kleene(
        pc.is_in(fa, value_set=pa.array(dims["fa"][0], pa.int32())),
        pc.is_in(fb, value_set=pa.array(dims["fb"][0].astype(np.uint16)))))
    want = ftbl.filter(mask)
    assert 0 < want.num_rows < tbl.num_rows
    got = out.to_arrow()
    assert got.schema.names == ["grp", "s", ename, "cat"]
    assert got.column("s").equals(want.column("s"))
    ev = pc.add(pc.multiply(want.column("i64"), 2), pc.cast(want.column("i8"), pa.int64()))
    assert got.column(ename).type == pa.int64() and got.column(ename).equals(ev)
    cat = dict(zip(dims["fa"][0].tolist(), dims["fa"][1]["cat"]))
    grp = dict(zip(dims["fb"][0].tolist(), dims["fb"][1]["grp"]))
    assert pa.types.is_dictionary(got.column("cat").type)
    assert got.column("cat").to_pylist() == [cat[k] for k in want.column("fa").to_pylist()]
    assert got.column("grp").to_pylist() == [grp[k] for k in want.column("fb").to_pylist()]


def test_refusals(files):
    from nvme_strom_amd.models.arrow_scan import (Join, JoinTable, StarJoin, host_scan_where)
    from nvme_strom_amd.ops.colexpr import E
    tbl, paths = files
    path = paths[None]
    quals, _ = G.quals_and_mask()
    names = [c for c in tbl.schema.names if c not in ("fa", "fb")]
    with pytest.raises(NotImplementedError, match="at most 16"):
        host_scan_where(path, quals, project=(names * 2)[:17])
    with pytest.raises(ValueError, match="twice"):
        host_scan_where(path, quals, project=["i8", "s", "i8"])
    with pytest.raises(ValueError, match="twice"):
        host_scan_where(path, quals, project=[E("i8") + 1, E("i8") + 1])
    with pytest.raises(ValueError, match="empty select list"):
        host_scan_where(path, quals, project=[])
    with pytest.raises(ValueError, match="no column"):
        host_scan_where(path, quals, project=["i8", "nope"])
    with pytest.raises(TypeError):
        host_scan_where(path, quals, project=["i8", 5])
    dims = G.dimensions()
    ka, attrs = dims["fa"]
    two = JoinTable(ka, attrs={"cat": attrs["cat"], "other": list(range(len(ka)))})
    with pytest.raises(NotImplementedError, match="one attribute per JoinTable"):
        host_scan_where(path, quals, project=[two["cat"], two["other"]], join=Join("fa", two))
    with pytest.raises(ValueError, match="needs join="):
        host_scan_where(path, quals, project=["i8", two["cat"]])
    with pytest.raises(ValueError, match="anti"):
        host_scan_where(path, quals, project=[two["cat"]], join=Join("fa", two, "anti"))
    with pytest.raises(ValueError, match="more than 4 computed"):
        host_scan_where(path, quals, project=[E("i8") + k for k in range(5)])
    # a kind the single form refuses too: float16 is not scanned
    f16 = pa.table({"h": pa.array(np.arange(8, dtype=np.float16)), "k": pa.array(np.arange(8))})
    from arrowgen import write
    p16 = os.path.join(os.path.dirname(path), "f16.arrow")
    write(p16, f16)
    with pytest.raises(NotImplementedError, match="projection of h"):
        host_scan_where(p16, [("k", 0, 5)], project=["k", "h"])
    # the multi-rank scan takes no list
    from nvme_strom_amd.parallel import scan as PS
    with pytest.raises(NotImplementedError, match="select list"):
        PS.DistributedArrowScan.scan_where(object(), quals, project=["i8"])
    # the single form is what it was
    out = host_scan_where(path, quals, project="i8")
    assert out.columns is None and out.values is not None
    with pytest.raises(NotImplementedError):
        _ = StarJoin(*[Join("fa", two)] * 5)


# ----------------------------------------------------------------- fuzzer
def test_fuzzer_builds_and_runs():
    exe = os.path.join(ROOT, "build", "colproject_fuzz")
    subprocess.run(["make", "-C", ROOT, "build/colproject_fuzz"], check=True,
                   capture_output=True)
    r = subprocess.run([exe, "2000", "11"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "2000 iterations ok" in r.stdout
