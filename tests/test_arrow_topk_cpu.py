"""ORDER BY ... LIMIT k of the Arrow scan on the CPU: the key encoding and
the coltopk twin against plain Python comparison, the library's CPU copy of
the kernels' phases against the twin word for word, host_top against
pyarrow's sort_indices, and the phases under ASan + UBSan."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")

sys.path.insert(0, os.path.dirname(__file__))

import topkgen as TG  # noqa: E402
from nvme_strom_amd.ops import coltopk as T  # noqa: E402


# ------------------------------------------------------------------ the twin
def test_geometry_and_limits():
    assert T.MAX_K >= 1024
    assert (T.state_words(1), T.state_words(100)) == (11, 308)
    assert (T.slab_words(1), T.slab_words(100)) == (5, 302)
    # slabs x k stays bounded, a workgroup walks 16 words at least
    assert [T.grid(n, k) for n, k in ((0, 5), (1, 5), (16, 5), (17, 5), (10**6, 5), (10**6, 1024),
                                      (10**6, T.MAX_K))] == [0, 1, 1, 2, 1024, 256, 42]
    for k in (0, -1, T.MAX_K + 1, 2.5, True):
        with pytest.raises(ValueError):
            T.check_k(k)
    assert T.check_k(T.MAX_K) == T.MAX_K


@pytest.mark.parametrize("dtype", TG.DTYPES)
def test_key_order_and_round_trip(dtype):
    """Keys order as the values do (both directions), -0.0 == +0.0, and
    decode gives the values back bit for bit (the zero's sign included)."""
    v = np.unique(np.concatenate([TG.values(dtype, "random", 400, False, 3),
                                  TG._specials(np.dtype(dtype))]))
    v = v[~np.isnan(v)] if v.dtype.kind == "f" else v          # sorted, distinct, no NaN
    if v.dtype.kind == "f":
        v = np.concatenate([v[v < 0], [-0.0, 0.0], v[v > 0]]).astype(dtype)
    for desc in (False, True):
        key, cls, negz = T.encode(v, None, desc)
        assert (cls == 0).all()
        step = np.diff(key.astype(object))
        same = np.diff(v.astype(object)) == 0 if v.dtype.kind != "f" else (v[1:] == v[:-1])
        assert (step[same] == 0).all()
        assert ((step[~same] < 0) if desc else (step[~same] > 0)).all()
        ent = T.entries(v, None, np.arange(len(v)), desc)
        rows, vals, ok, pay, pok = T.decode(ent, dtype, desc)
        assert rows.tolist() == list(range(len(v))) and ok.all() and not pok.any()
        assert vals.dtype == v.dtype and vals.tobytes() == v.tobytes()
    if v.dtype.kind == "f":
        ent = T.entries(np.array([np.nan, 1.0, 2.0], dtype), np.array([True, True, False]),
                        [5, 6, 7], True)
        assert (ent[:, 1] >> np.uint64(62)).tolist() == [1, 0, 2] and ent[0, 0] == ent[2, 0] == 0
        rows, vals, ok, _, _ = T.decode(ent, dtype, True)
        assert np.isnan(vals[0]) and vals[1] == 1.0 and ok.tolist() == [True, True, False]


def _run_twin(select, merge, bl, pay, srcs, k, desc, prefill=True):
    """Select + merge per source bitmap against one state: (slabs of each
    round, the final state).  Words no phase writes keep the prefill."""
    st = np.full(T.state_words(k), TG.PREFILL, np.uint64)
    st[:T.HDR_WORDS] = T.host_init(k)[:T.HDR_WORDS]
    slabs = []
    for src in srcs:
        out = np.full((T.grid(len(src), k), T.slab_words(k)), TG.PREFILL, np.uint64)
        slabs.append(select(bl, src, k, desc, st, pay, out=out))
        st = merge(st, slabs[-1], k)
    return slabs, st


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("dtype", TG.DTYPES)
def test_twin_equals_plain_comparison(dtype, desc):
    """host_select + host_merge over hand-built batches against a Python
    sort by (class, value, row): every case x k, two rounds on one state."""
    for case in ("random", "equal", "worst", "best") + (("zeros",) if dtype[0] == "f" else ()):
        bl, pay = TG.batches(dtype, case, desc, seed=len(case))
        # the second round selects the rows the first did not
        srcs = [TG.bitmap(TG.ROWS, "random", 1), ~TG.bitmap(TG.ROWS, "random", 1)]
        for k in TG.KERNEL_KS:
            _, st = _run_twin(T.host_select, T.host_merge, bl, pay, srcs, k, desc)
            want = TG.expected(bl, TG.bitmap(TG.ROWS, "all"), k, desc, pay)
            rows, _, _, p, pv = T.decode(T.state_entries(st), dtype, desc)
            assert list(zip(rows.tolist(), T.payload_as(p, np.int32).tolist(),
                            pv.astype(int).tolist())) == want, (case, k)
            assert int(st[T.H_SEEN]) == sum(TG.ROWS) and int(st[T.H_MERGES]) == 2
    # one round, every row once: the state is exactly the expected rows
    bl, pay = TG.batches(dtype, "random", desc, seed=9)
    src = TG.bitmap(TG.ROWS, "random", 3)
    for k in TG.KERNEL_KS:
        _, st = _run_twin(T.host_select, T.host_merge, bl, pay, [src], k, desc)
        rows, _, _, p, pv = T.decode(T.state_entries(st), dtype, desc)
        assert list(zip(rows.tolist(), T.payload_as(p, np.int32).tolist(),
                        pv.astype(int).tolist())) == TG.expected(bl, src, k, desc, pay), k
        nsel = len(TG.expected(bl, src, 10**6, desc, pay))
        assert int(st[T.H_SEEN]) == nsel and int(st[T.H_COUNT]) == min(k, nsel)
        assert int(st[T.H_ERRORS]) == 0 and int(st[T.H_MERGES]) == 1
        assert (st[T.HDR_WORDS + 3 * min(k, nsel):] == TG.PREFILL).all()


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("dtype", TG.DTYPES)
def test_native_host_copy_equals_twin(dtype, desc):
    """The kernels' phases compiled for the CPU (strom_topk_host_select /
    _merge: the append, sort, cut and threshold code the GPU runs) against
    the numpy twin, slabs and state word for word, four rounds on one
    state, more than one workgroup, k up to MAX_K."""
    rows = TG.ROWS + [700, 1000, 0, 130]
    for case in ("random", "equal", "worst", "best"):
        bl, pay = TG.batches(dtype, case, desc, rows=rows, seed=4)
        srcs = [TG.bitmap(rows, kind, i) for i, kind in enumerate(("random", "all", "percent",
                                                                    "none"))]
        for k in TG.KERNEL_KS + [T.MAX_K]:
            assert T.grid(len(srcs[0]), k) > 1
            a, sa = _run_twin(T.host_select, T.host_merge, bl, pay, srcs, k, desc)
            b, sb = _run_twin(T.native_host_select, T.native_host_merge, bl, pay, srcs, k, desc)
            for x, y in zip(a, b):
                assert np.array_equal(x, y), (case, k)
            assert np.array_equal(sa, sb), (case, k)
    # without a carried column
    bl, _ = TG.batches(dtype, "random", desc, seed=5)
    src = TG.bitmap(TG.ROWS, "random", 5)
    a, sa = _run_twin(T.host_select, T.host_merge, bl, None, [src], 3, desc)
    b, sb = _run_twin(T.native_host_select, T.native_host_merge, bl, None, [src], 3, desc)
    assert np.array_equal(a[0], b[0]) and np.array_equal(sa, sb)


def test_stale_threshold_and_refused_slabs():
    """A select that read an older threshold leaves more candidates and the
    same result; a slab with a count above k and a state of another k are
    counted in ERRORS and not followed."""
    bl, pay = TG.batches("i4", "worst", False, seed=6)
    s1, s2 = TG.bitmap(TG.ROWS, "all", 0), TG.bitmap(TG.ROWS, "random", 7)
    k = 3
    st = T.host_merge(T.host_init(k), T.host_select(bl, s1, k, False, None, pay), k)
    assert st[T.H_THRESH] != T.PASS
    fresh = T.host_select(bl, s2, k, False, st, pay)
    stale = T.host_select(bl, s2, k, False, T.host_init(k), pay)
    assert fresh[:, 0].sum() < stale[:, 0].sum()
    assert np.array_equal(T.host_merge(st, fresh, k), T.host_merge(st, stale, k))
    for merge in (T.host_merge, T.native_host_merge):
        bad = stale.copy()
        bad[0, 0] = k + 1
        out = merge(st, bad, k)
        assert int(out[T.H_ERRORS]) == 1 and int(out[T.H_MERGES]) == 2
        other = merge(st, np.zeros((1, T.slab_words(2)), np.uint64), 2)
        assert int(other[T.H_ERRORS]) == 1 and np.array_equal(other[T.HDR_WORDS:],
                                                              st[T.HDR_WORDS:])


# ------------------------------------------------------------------ whole scans
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    import arrowgen
    d = tmp_path_factory.mktemp("topk")
    out = {}
    for codec in TG.CODECS:
        out[codec] = str(d / f"t_{codec}.arrow")
        arrowgen.write(out[codec], TG.table(), codec, batch_rows=TG.BATCH_ROWS)
    return out


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("codec", TG.CODECS)
def test_host_top_equals_sort_indices(files, codec, desc):
    """host_top == pc.sort_indices(...)[:k] over the selected rows: 9 order
    columns x 4 qualifier lists x k in {1, 7, 700, 5000}."""
    from nvme_strom_amd.models.arrow_scan import host_top
    from nvme_strom_amd.utils.arrow_ipc import read_metadata
    tbl = TG.table()
    meta, dicts = read_metadata(files[codec]), {}
    for label, quals, mask in TG.qual_lists():
        ids = TG.selected_ids(tbl, mask)
        assert (len(ids) == 0) == (label == "nothing")
        for col in TG.ORDER_COLS:
            nulls = tbl.column(col).null_count > 0
            for k in TG.KS:
                out = host_top(files[codec], quals, col, k, desc, meta=meta, dicts=dicts)
                want = TG.reference(tbl, ids, col, desc, k)
                TG.check_result(out, tbl, want, col, nulls, label=(label, col, k))
                assert out.nrows == 3000 and out.selected == len(ids)
                assert len(out.rows) == min(k, len(ids))


def test_carried_columns_and_join(files):
    """project= of a fixed-width column with nulls, of a dictionary-encoded
    column (its indices) and of the semi-join's attribute."""
    from nvme_strom_amd.models.arrow_scan import Join, JoinTable, host_top
    tbl = TG.table()
    path = files[None]
    label, quals, mask = TG.qual_lists()[3]
    ids = TG.selected_ids(tbl, mask)
    for col, proj, pnulls in (("f32", "i64", True), ("i64", "f64", False), ("ts", "dict", True),
                              ("u32", "i8", True), ("f64", "f64", False)):
        for desc in (False, True):
            out = host_top(path, quals, col, 50, desc, project=proj)
            want = TG.reference(tbl, ids, col, desc, 50)
            TG.check_result(out, tbl, want, col, tbl.column(col).null_count > 0, proj, pnulls,
                            label=(col, proj))
            if proj == "dict":
                assert out.dictionary is not None
    # a semi-join on i8 with an attribute of the dimension carried along
    keys = np.arange(-40, 40, 3, dtype=np.int64)
    dim = JoinTable(keys, {"name": [f"n{int(x) % 5}" for x in keys]})
    i8 = tbl.column("i8").combine_chunks()
    hit = np.isin(i8.fill_null(127).to_numpy(zero_copy_only=False), keys) & np.asarray(i8.is_valid())
    jids = np.flatnonzero(hit).astype(np.int64)
    for desc in (False, True):
        out = host_top(path, [], "f32", 100, desc, project=dim["name"], join=Join("i8", dim))
        want = TG.reference(tbl, jids, "f32", desc, 100)
        assert out.rows.tolist() == want.tolist() and out.selected == len(jids)
        names = [out.dictionary[c] for c in out.projected.tolist()]
        fk = i8.take(pa.array(want)).to_pylist()
        assert names == [f"n{x % 5}" for x in fk] and out.projected_valid is None
        # the anti-join keeps the other rows (no attribute there)
        out = host_top(path, [], "i64", 20, desc, join=Join("i8", dim, how="anti"))
        rest = np.flatnonzero(~hit).astype(np.int64)
        assert out.rows.tolist() == TG.reference(tbl, rest, "i64", desc, 20).tolist()


def test_merged_batch_ranges(files):
    """batches= halves merged with TopOut.merge equal the whole file's
    result; results of another query do not merge."""
    from nvme_strom_amd.models.arrow_scan import host_top
    tbl = TG.table()
    path = files["lz4"]
    _, quals, mask = TG.qual_lists()[2]
    for col, desc, k, proj in (("f32", True, 40, "i64"), ("i64", False, 700, None),
                               ("t32", True, 5000, "dict")):
        whole = host_top(path, quals, col, k, desc, project=proj)
        a = host_top(path, quals, col, k, desc, project=proj, batches=(0, 2))
        b = host_top(path, quals, col, k, desc, project=proj, batches=(2, 5))
        assert a.nrows == 1400 and b.nrows == 1600
        assert a.rows.tolist() == TG.reference(tbl, TG.selected_ids(tbl, mask, 0, 1400), col, desc,
                                               k).tolist()
        for m in (a.merge(b), b.merge(a)):
            assert m.rows.tolist() == whole.rows.tolist() and m.nrows == 3000
            assert m.selected == whole.selected
            assert np.array_equal(m.values, whole.values, equal_nan=True)
            assert np.array_equal(m._entries, whole._entries)
        for other in (host_top(path, quals, col, k, not desc, project=proj),
                      host_top(path, quals, col, k + 1, desc, project=proj),
                      host_top(path, quals, "u32", k, desc, project=proj),
                      host_top(path, quals, col, k, desc, project="i8")):
            with pytest.raises(ValueError):
                a.merge(other)
    # an empty batch range
    e = host_top(path, [], "i64", 5, batches=(3, 3))
    assert e.nrows == 0 and len(e.rows) == 0 and e.values.dtype == np.int64
    assert e.merge(whole_i64 := host_top(path, [], "i64", 5)).rows.tolist() == \
        whole_i64.rows.tolist()


def test_refusals(files, tmp_path):
    from nvme_strom_amd.models.arrow_scan import Join, JoinTable, host_top
    path = files[None]
    for k in (0, -3, T.MAX_K + 1):
        with pytest.raises(ValueError):
            host_top(path, [], "i64", k)
    with pytest.raises(ValueError):
        host_top(path, [], "nope", 3)
    with pytest.raises(ValueError):
        host_top(path, [], "i64", 3, project="nope")
    for col, kind in (("dec", "decimal"), ("b", "bool"), ("s", "utf8"), ("bin", "binary"),
                      ("ls", "utf8"), ("dict", "dictionary-encoded"),
                      ("idict", "dictionary-encoded")):
        with pytest.raises(NotImplementedError, match=kind):
            host_top(path, [], col, 3)
    for col, kind in (("s", "utf8"), ("dec", "decimal"), ("bin", "binary"), ("b", "bool")):
        with pytest.raises(NotImplementedError, match=kind):
            host_top(path, [], "i64", 3, project=col)
    with pytest.raises(NotImplementedError):
        host_top(path, [], ["i64", "f64"], 3)
    dim = JoinTable(np.arange(5), {"a": list("abcde")})
    with pytest.raises(ValueError):
        host_top(path, [], "i64", 3, project=dim["a"])                 # no join=
    with pytest.raises(ValueError):
        host_top(path, [], "i64", 3, project=dim["a"], join=Join("i8", dim, how="anti"))
    # an empty file
    import arrowgen
    empty = str(tmp_path / "empty.arrow")
    arrowgen.write(empty, TG.table().slice(0, 0), None)
    out = host_top(empty, [], "f32", 4, project="i64")
    assert out.nrows == 0 and out.selected == 0 and len(out.rows) == 0
    assert out.values.dtype == np.float32 and out.projected.dtype == np.int64


# ------------------------------------------------------------------ sanitizer
def test_coltopk_fuzz_asan():
    """Randomized tables and bitmaps of every storage type through the host
    copy of select + merge built with ASan + UBSan (csrc/tests/coltopk_fuzz.cc)
    against a plain std::sort: exits 0."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if shutil.which("make") is None or not (
            os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))):
        pytest.skip("no make / hipcc")
    r = subprocess.run(["make", "-s", "build/coltopk_fuzz"], cwd=root, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([os.path.join(root, "build", "coltopk_fuzz"), "1500"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "1500 cases ok" in r.stdout
