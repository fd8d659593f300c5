"""The select list on the GPU (strom_bitmap_to_rows_multi,
csrc/kernels/colproject.hip): the kernel alone on hand-built batch tables
against its numpy twin, bit for bit, with sentinels before and past the
cursors; and whole scans with ``project=[...]`` against pyarrow's filtered
select and against the single-column projection of the same query."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pa = pytest.importorskip("pyarrow")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))

import projgen as G  # noqa: E402
from nvme_strom_amd.ops import colproject as PJ  # noqa: E402


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nvme_strom_amd as S
    S.configure(gpu_emulation=0)
    return S


# ------------------------------------------------------------ kernel alone
@pytest.fixture(scope="module")
def cases():
    return G.kernel_cases(np.random.default_rng(7))


@pytest.mark.parametrize("kind", G.BITMAPS)
def test_kernel_equals_twin_bitmaps(S, cases, kind):
    """Every bitmap shape at nwords 1 / 255 / 256 / 257 / 600, one batch and
    three of 1 / 65 / 4,097 rows; the cursors start at 3 rows and 5
    characters."""
    be = G.DeviceBackend()
    mine = [c for c in cases if c.name.startswith(kind + "/") and c.name.endswith("b")]
    assert len(mine) == 2 * len(G.NWORDS)
    for case in mine:
        G.run_and_check(be, [case], total0=3, cur0=5)


@pytest.mark.parametrize("ncols", [1, 2, 7, 16])
def test_kernel_equals_twin_columns(S, cases, ncols):
    """ncols columns of every kind and width on about 40,000 rows in 29
    batches: densities 1/2 and 1/1000, whole empty blocks between full ones."""
    be = G.DeviceBackend()
    mine = [c for c in cases if c.name.endswith(f"/{ncols}c")]
    assert len(mine) == 3
    for case in mine:
        G.run_and_check(be, [case])


def test_kernel_appends_behind_odd_cursors(S):
    rng = np.random.default_rng(9)
    rows = G.ROWS3
    bt = G.batch_table(rows)
    nw = G.nwords_of(bt)
    cs = []
    for kind in ("d2", "one_per_word"):
        cols, want = G.mixed_cols(7, rows, rng)
        cs.append(G.Case(kind, G.bitmap(kind, nw, rng), bt, cols, want))
    be = G.DeviceBackend()
    # the first call leaves the row cursor odd: the second starts at an odd
    # row and, per string column, wherever the characters ended
    t0 = 1 - len(PJ.host_rows_multi(cs[0].bitmap, cs[0].batches, cs[0].cols)[0]) % 2
    mid = G.run_and_check(be, cs[:1], total0=t0, cur0=1)
    strs = [k for k, c in enumerate(cs[0].cols) if PJ.is_str(c.kind)]
    assert mid["rows"] % 2 == 1 and len(strs) == 2 and any(mid["chars"][k] % 4 for k in strs)
    end = G.run_and_check(be, cs, total0=t0, cur0=1)
    assert end["rows"] > mid["rows"]


def test_kernel_entry_refusals(S):
    dev = torch.device("cuda")
    bm = torch.ones(1, dtype=torch.int64, device=dev)
    bt = torch.from_numpy(G.batch_table((10,))).to(dev)
    out = torch.zeros(16, dtype=torch.int64, device=dev)
    tot = torch.zeros(1, dtype=torch.int64, device=dev)
    vals = torch.zeros(16, dtype=torch.int64, device=dev)
    tabs = torch.zeros((1, 1, 7), dtype=torch.int64, device=dev)
    col = (PJ.FIXED, 8, vals.data_ptr(), 0, 0, 0)
    from nvme_strom_amd import _native as N
    lib = N.lib()

    def call(cols, ncols=None, nwords=1):
        c = PJ.with_tables(cols, tabs.data_ptr(), 1) if len(cols) else cols
        return lib.strom_bitmap_to_rows_multi(bm.data_ptr(), nwords, bt.data_ptr(), 1,
                                              out.data_ptr(), tot.data_ptr(),
                                              c.ctypes.data if len(c) else 0,
                                              len(c) if ncols is None else ncols, 0)
    good = PJ.proj_cols([col])
    assert call(good, nwords=0) == 0
    assert call(good, ncols=0) == -22 and call(good, ncols=17) == -22
    for kind, width in ((0, 8), (5, 8), (PJ.FIXED, 3), (PJ.FIXED, 32)):
        bad = good.copy()
        bad["kind"], bad["width"] = kind, width
        assert call(bad) == -22, (kind, width)
    bad = good.copy()
    bad["kind"] = PJ.STR32
    assert call(bad) == -22
    torch.cuda.synchronize()
    assert int(tot.item()) == 0


# ------------------------------------------------------------ whole scans
@pytest.fixture(scope="module")
def files(S, tmp_path_factory):
    from arrowgen import write
    tbl = G.table(50_000, seed=6)
    d = tmp_path_factory.mktemp("projgpu")
    paths = {}
    for codec in (None, "lz4", "zstd"):
        paths[codec] = str(d / f"proj_{codec}.arrow")
        write(paths[codec], tbl, codec, batch_rows=7001)
    return tbl, paths


def _scan(path):
    """The ring held at its minimum and slots of 1 MiB whatever the codec:
    the long select lists take more groups than there are slots, so every
    slot's buffers and tables are reused."""
    from nvme_strom_amd.models.arrow_scan import ArrowScan
    sc = ArrowScan(path, "cuda", chunk_sz=64 << 10, slot_bytes=1 << 20, max_slot_bytes=1 << 20,
                   nslots=2)
    sc.MAX_SLOTS = 2
    return sc


def _same(a, b, what=None):
    """Bit for bit (NaNs included; the unsigned dtypes compare on the host)."""
    if a is None or b is None:
        assert a is None and b is None, what
    else:
        x, y = a.cpu().numpy(), b.cpu().numpy()
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), what


@pytest.mark.parametrize("codec", [None, "lz4", "zstd"])
def test_scan_select(S, files, codec):
    """to_arrow() equals pyarrow's filtered select; every list-form column
    equals the single-form projection of the same query, bit for bit."""
    tbl, paths = files
    quals, mask_of = G.quals_and_mask()
    ftbl = pa.ipc.open_file(paths[codec]).read_all()
    mask = mask_of(ftbl)
    sc = _scan(paths[codec])
    try:
        for names in G.SELECTS:
            out = sc.scan_where(quals, project=names)
            assert out.groups > len(sc._slots) or len(names) < 8
            assert out.values is None and out.valid is None and out.offsets is None
            assert [c.name for c in out.columns] == names
            want = G.reference(ftbl, mask, names)
            assert out.selected == want.num_rows and 0 < want.num_rows < tbl.num_rows
            G.same_table(out.to_arrow(), want)
            h = sc.host_scan_where(quals, project=names)
            assert np.array_equal(out.indices.cpu().numpy(), h.indices)
            for name, col in zip(names, out.columns):
                if name == "b":
                    # bools are new in the list form: uint8 0/1
                    assert col.values.dtype == torch.uint8 and int(col.values.max()) == 1
                    continue
                one = sc.scan_where(quals, project=name)
                _same(one.indices, out.indices, name)
                _same(one.values, col.values, name)
                _same(one.valid, col.valid, name)
                _same(one.offsets, col.offsets, name)
                assert one.column == col.column
    finally:
        sc.close()


def test_scan_select_star_join(S, files):
    """Two legs' attributes and an expression in the list."""
    import pyarrow.compute as pc
    from nvme_strom_amd.models.arrow_scan import Join, JoinTable, StarJoin
    from nvme_strom_amd.ops.colexpr import E, name_of
    tbl, paths = files
    quals, mask_of = G.quals_and_mask()
    ftbl = pa.ipc.open_file(paths[None]).read_all()
    dims = G.dimensions()
    jt = {fk: JoinTable(keys, attrs=attrs, device="cuda") for fk, (keys, attrs) in dims.items()}
    expr = E("i64") * 2 + E("i8")
    sj = StarJoin(Join("fa", jt["fa"]), Join("fb", jt["fb"]))
    proj = [jt["fb"]["grp"], "s", expr, jt["fa"]["cat"], "u16"]
    sc = _scan(paths[None])
    try:
        out = sc.scan_where(quals, project=proj, join=sj)
        h = sc.host_scan_where(quals, project=proj, join=sj)
        assert out.selected == len(h.indices) > 100 and out.groups >= len(sc._slots)
        assert np.array_equal(out.indices.cpu().numpy(), h.indices)
        got, want = out.to_arrow(), h.to_arrow()
        assert got.schema.names == ["grp", "s", str(name_of(expr)), "cat", "u16"]
        assert got.equals(want)
        # and against pyarrow
        ref = ftbl.take(pa.array(h.indices))
        assert got.column("s").equals(ref.column("s"))
        assert got.column("u16").equals(ref.column("u16"))
        ev = pc.add(pc.multiply(ref.column("i64"), 2), pc.cast(ref.column("i8"), pa.int64()))
        assert got.column(str(name_of(expr))).equals(ev)
        cat = dict(zip(dims["fa"][0].tolist(), dims["fa"][1]["cat"]))
        grp = dict(zip(dims["fb"][0].tolist(), dims["fb"][1]["grp"]))
        assert got.column("cat").to_pylist() == [cat[k] for k in ref.column("fa").to_pylist()]
        assert got.column("grp").to_pylist() == [grp[k] for k in ref.column("fb").to_pylist()]
        # each attribute alone, single form
        for attr, col in ((jt["fb"]["grp"], out.columns[0]), (jt["fa"]["cat"], out.columns[3])):
            one = sc.scan_where(quals, project=attr, join=sj)
            _same(one.values, col.values)
            assert one.dictionary == col.dictionary
        # one leg, join=Join: the attribute comes from the slot's key buffer
        one = sc.scan_where(quals, project=[jt["fa"]["cat"], "i32"], join=Join("fa", jt["fa"]))
        ref1 = sc.scan_where(quals, project=jt["fa"]["cat"], join=Join("fa", jt["fa"]))
        _same(one.columns[0].values, ref1.values)
        _same(one.indices, ref1.indices)
    finally:
        sc.close()
        for t in jt.values():
            t.close()


def test_scan_select_nothing_selected(S, files):
    from nvme_strom_amd.ops.colpred import P
    tbl, paths = files
    quals, _ = G.quals_and_mask()
    ftbl = pa.ipc.open_file(paths[None]).read_all()
    names = G.SELECTS[1]
    sc = _scan(paths[None])
    try:
        for kw in (dict(quals=[P("f64") > 2.0]), dict(quals=quals, batches=(3, 3))):
            out = sc.scan_where(kw["quals"], project=names, batches=kw.get("batches"))
            assert out.selected == 0 and out.indices.numel() == 0
            assert all(c.values.numel() == 0 for c in out.columns)
            G.same_table(out.to_arrow(), ftbl.slice(0, 0).select(names))
    finally:
        sc.close()
