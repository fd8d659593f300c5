"""LIKE / contains / endswith on the GPU (csrc/kernels/collike.hip): the
kernel alone on hand-built batch tables, bit for bit against the `re`
reference of tests/likegen.py (all bitmap words, tail bits included, and the
accumulating count), and whole scans against pyarrow.compute and the host
twins."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))

import likegen as L  # noqa: E402
from nvme_strom_amd.ops import colpred as CP  # noqa: E402
from nvme_strom_amd.ops.colpred import Or, P, Pred  # noqa: E402

CODECS = [None, "lz4", "zstd"]
ALL4 = ((False, False), (True, False), (False, True), (True, True))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def _dev_words(w, dev):
    return torch.from_numpy(np.ascontiguousarray(w).view(np.int64).copy()).to(dev)


def _host_words(t):
    return t.cpu().numpy().view(np.uint64)


# the rows of a table depend on (utf8, malformed) alone: s4 and s8 share a reference
_TABLES, _REFS = {}, {}


def _table(dt, utf8, bad):
    if (dt, utf8, bad) not in _TABLES:
        _TABLES[dt, utf8, bad] = L.like_table(dt, utf8, np.random.default_rng(50 + bad), bad)
    return _TABLES[dt, utf8, bad]


def _ref(t, utf8, bad, name, op, v, neg):
    key = (utf8, bad, name, neg)
    if key not in _REFS:
        _REFS[key] = L.pack_words(t, L.like_ref(t, op, v, utf8, neg))
    return _REFS[key]


def _launches(dev, t, dtab, c, pred, combos, what, seed=0):
    """kernel == reference in each combination mode; one count accumulates."""
    rng = np.random.default_rng(seed)
    nw = t.nwords
    old = rng.integers(0, 1 << 64, nw + 1, dtype=np.uint64, endpoint=False)
    orw = rng.integers(0, 1 << 64, nw, dtype=np.uint64, endpoint=False)
    or_t = _dev_words(orw, dev)
    cnt = torch.full((1,), 7, dtype=torch.int64, device=dev)
    total = 7
    for use_or, and_dst in combos:
        bm = _dev_words(old, dev)                       # the last word is a guard
        CP.qual_batched(c, dtab.qtab, nw, bm, cnt, or_src=or_t if use_or else None, and_dst=and_dst)
        exp = L.expected_words(pred, orw if use_or else None, and_dst, old[:nw])
        got = _host_words(bm)
        bad = np.flatnonzero(got[:nw] != exp)
        assert not len(bad), (what, use_or, and_dst, bad[:8], [hex(x) for x in got[bad[:4]]],
                              [hex(x) for x in exp[bad[:4]]])
        assert got[nw] == old[nw], what
        total += L.popcount(exp)
        assert int(cnt.item()) == total, (what, use_or, and_dst)


# ------------------------------------------------------------ the kernel alone
@pytest.mark.parametrize("utf8", [True, False], ids=["utf8", "binary"])
@pytest.mark.parametrize("dt", ["s4", "s8"])
def test_like_kernel(dev, dt, utf8):
    """Every pattern class over qualgen's batch geometry (rows of 0 to 5,000
    bytes at every alignment, short and long ones in the same words), plain
    and NEGATE, the four or_src / and_dst combinations."""
    t = _table(dt, utf8, False)
    dtab = L.DeviceTable(t, dev)
    for name, op, v in L.like_preds(utf8):
        for neg in (False, True):
            c = L.compile_like(op, v, dt, utf8, neg)
            _launches(dev, t, dtab, c, _ref(t, utf8, False, name, op, v, neg), ALL4,
                      (dt, utf8, name, neg), len(name))


@pytest.mark.parametrize("utf8", [True, False], ids=["utf8", "binary"])
@pytest.mark.parametrize("dt", ["s4", "s8"])
def test_like_kernel_malformed_offsets(dev, dt, utf8):
    """The same with three malformed offsets per batch: those rows are
    selected by no pattern, NEGATE or not, and never followed."""
    t = _table(dt, utf8, True)
    assert sum(L.row_bytes(b, i) is None for b in t.batches for i in range(b.nrows)) >= 18
    dtab = L.DeviceTable(t, dev)
    for name, op, v in L.like_preds(utf8):
        for neg in (False, True):
            c = L.compile_like(op, v, dt, utf8, neg)
            _launches(dev, t, dtab, c, _ref(t, utf8, True, name, op, v, neg), ALL4,
                      (dt, utf8, name, neg, "bad"), len(name))


def _long_case(utf8):
    """(table, [(op, value)]): long rows with the needle at the start, deep
    inside and at the end, dealt among short rows."""
    rows = []
    for n in (255, 256, 257, 1000, 5000):
        src = ("é€" * n).encode() if utf8 else bytes([0xC3, 0xA9, 0x80]) * n
        fill = L._cut(src, 0, n - 12, utf8)
        half = L._cut(src, 0, n // 2, utf8)
        rows += [b"needle" + fill + b"haytai", fill + b"needle" + b"haytai",
                 half + b"need\xc3\xa9e" + half[:n - n // 2 - 13] + b"tail..",
                 b"a" * (n - 1) + b"b", b"a" * n, fill + b"needl" + b"e" * 7]
    rows += [b"needle", b"", b"tail", b"ab", b"a" * 40 + b"b", b"need\xc3\xa9e tail", b"x"] * 4
    t = L.like_table("s4", utf8, np.random.default_rng(61), False, [64, 130, 257],
                     [None, "dirty", "clean"], rows=rows)
    v = (lambda s: s) if utf8 else (lambda s: s.encode())
    preds = [("contains", v("needle")), ("like", v("needle%")), ("like", v("%haytai")),
             ("like", "%need_e%tail%" if utf8 else b"%need__e%tail%"), ("like", v("%need__e%")),
             ("like", v("%" + "a" * 40 + "b")), ("like", v("%" + "a" * 300 + "b%")),
             ("like", v("_%needle%hay_ai")), ("like", v("%needl%eeeeee")),
             ("suffix", [v("tail.."), v("b")]), ("not like", v("%e%"))]
    if utf8:
        preds += [("like", "%é€é_é%needle_aytai"), ("like", "%€_€%_______")]
    else:
        preds += [("like", b"%\xa9_\xc3%needle_aytai"), ("like", b"%\x80\xc3__\xc3%_______")]
    return t, preds


def test_like_long_and_short_rows_in_one_word(dev):
    """Rows of 255 / 256 / 257 / 1,000 / 5,000 bytes next to short ones in
    the same bitmap words: the row-per-lane and the row-per-wave path give
    the reference's bits, the needle at the start, deep inside and at the end."""
    for utf8 in (True, False):
        t, preds = _long_case(utf8)
        dtab = L.DeviceTable(t, dev)
        for op, val in preds:
            c = L.compile_like(op, val, "s4", utf8)
            pred = L.pack_words(t, L.like_ref(t, op, val, utf8))
            assert 0 < L.popcount(pred) < t.nrows, (op, val)
            _launches(dev, t, dtab, c, pred, ((False, False), (True, True)), (utf8, op, val))


def test_like_grid_stride(dev):
    """nwords just above 8192 blocks x 4 words: the grid-stride loop takes a
    second trip.  The reference is the regular expression per distinct word."""
    rng = np.random.default_rng(23)
    vocab = [b"", b"a", b"ab", b"abc", b"xabc", b"a\xc3\xa9c", b"abcabc", b"ba", b"cab", b"aXbYc",
             b"\xe2\x82\xacabc", b"abd"]
    geo = [64 * 12000 + 1, 64 * 20000 + 63, 64 * 775 + 5]
    lens = np.array([len(w) for w in vocab])
    batches, ids = [], []
    for n, mode in zip(geo, [None, "dirty", None]):
        k = rng.integers(0, len(vocab), n)
        offs = np.concatenate([[0], np.cumsum(lens[k])]).astype(np.int64)
        chars = np.frombuffer(b"".join(vocab[i] for i in k), np.uint8)
        batches.append(L.Batch(n, (offs, chars), L.make_valid(n, mode, rng), mode))
        ids.append(k)
    t = L.Table("s4", batches)
    assert t.nwords == 8192 * 4 + 10
    dtab = L.DeviceTable(t, dev)
    old = rng.integers(0, 1 << 64, t.nwords + 1, dtype=np.uint64, endpoint=False)
    for op, val in (("contains", "abc"), ("like", "a_c%")):
        rxs = [L.like_regex(p, True) for p in L.ref_patterns(op, val)]
        by_word = np.array([any(rx.fullmatch(w) for rx in rxs) for w in vocab], bool)
        bits = [by_word[k] & (b.valid if b.valid is not None else True)
                for k, b in zip(ids, t.batches)]
        pred = L.pack_words(t, bits)
        c = L.compile_like(op, val, "s4", True)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        total = 0
        for and_dst in (False, True):
            bm = _dev_words(old, dev)
            CP.qual_batched(c, dtab.qtab, t.nwords, bm, cnt, and_dst=and_dst)
            exp = L.expected_words(pred, None, and_dst, old[:t.nwords])
            got = _host_words(bm)
            assert np.array_equal(got[:t.nwords], exp) and got[t.nwords] == old[t.nwords]
            total += L.popcount(exp)
            assert int(cnt.item()) == total


def test_like_kernel_equals_twin_on_bytes_that_are_no_utf8(dev):
    """On a utf8 column holding other bytes the kernel's bits are the numpy
    twin's (and the host copy's: tests/test_arrow_like_cpu.py)."""
    rng = np.random.default_rng(78)
    alpha = np.array([0x61, 0x62, 0x80, 0xA9, 0xBF, 0xC3, 0xE2, 0xF0, 0x5F], np.uint8)
    junk = [bytes(rng.choice(alpha, int(n))) for n in rng.integers(0, 24, 300)]
    junk += [bytes(rng.integers(0x80, 0xC0, 300, dtype=np.uint8)), b"a" + bytes([0x80]) * 299 + b"b",
             bytes(rng.choice(alpha, 700))]
    t = L.like_table("s4", True, rng, False, [64, 2600, 1], [None, "dirty", None], rows=junk)
    dtab = L.DeviceTable(t, dev)
    for pat in ("_", "__", "%_", "_%", "a_b", "%a_", "_a%", "%_b_%", "%a__b%", "a%_", "%__", "___%",
                "%b_a%_", "%_é%", "é_%", "%_é", "%a_b%_a_"):
        c = L.compile_like("like", pat, "s4", True)
        twin = [CP.evaluate(c, L.host_values(t, b), b.valid, b.nrows) for b in t.batches]
        _launches(dev, t, dtab, c, L.pack_words(t, twin), ((False, False),), pat)


# ------------------------------------------------------------------ whole scans
@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nvme_strom_amd as S
    S.configure(gpu_emulation=0)
    return S


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    pytest.importorskip("pyarrow")
    import arrowgen
    d = tmp_path_factory.mktemp("like")
    out = {}
    for codec in CODECS:
        out[codec] = str(d / f"like_{codec}.arrow")
        arrowgen.write(out[codec], L.arrow_table(), codec, batch_rows=1000)
    return out


@pytest.mark.parametrize("codec", CODECS)
def test_scans_equal_pyarrow_and_host(S, files, codec):
    """scan_where with like / contains / endswith / not_like and an Or of
    them over a 6,000-row file in 1,000-row batches, on string, large_string,
    binary and dictionary columns: row ids == pyarrow.compute ==
    host_scan_where; an aggregate and a top under a like qualifier."""
    from nvme_strom_amd.models.arrow_scan import ArrowScan
    tbl = L.arrow_table()
    v = tbl.column("v").to_numpy()
    sc = ArrowScan(files[codec], "cuda")
    try:
        nsel = 0
        for col in ("s", "ls", "bin", "dict"):
            for label, op, val in L.SCAN_PREDS:
                want = np.flatnonzero(L.pc_mask(tbl, col, op, val))
                q = [Pred(col, op, val)]
                got = sc.scan_where(q).indices.cpu().numpy()
                assert np.array_equal(got, want), (col, label)
                assert np.array_equal(sc.host_scan_where(q).indices, want), (col, label)
                nsel += len(want)
        assert nsel > 10000
        q = [Or(P("s").like("%green"), P("bin").contains(b"special"), P("dict").endswith("o")),
             P("ls").not_like("a%"), P("v") < 700]
        m = (L.pc_mask(tbl, "s", "like", "%green") | L.pc_mask(tbl, "bin", "contains", "special") |
             L.pc_mask(tbl, "dict", "suffix", "o")) & L.pc_mask(tbl, "ls", "not like", "a%") & \
            (v < 700)
        assert np.array_equal(sc.scan_where(q).indices.cpu().numpy(), np.flatnonzero(m))
        part = sc.scan_where(q, batches=(2, 5)).indices.cpu().numpy()
        ids = np.flatnonzero(m)
        assert np.array_equal(part, ids[(ids >= 2000) & (ids < 5000)])
        # aggregate and top
        ql = [P("s").like("%special%requests%")]
        ml = L.pc_mask(tbl, "s", "like", "%special%requests%")
        aggs = [("count", None), ("sum", "v")]
        out, host = sc.aggregate(ql, aggs), sc.host_aggregate(ql, aggs)
        assert out.selected == host.selected == int(ml.sum()) > 0
        for i in range(len(aggs)):
            assert np.array_equal(np.asarray(out.values[i]), np.asarray(host.values[i]))
        assert int(np.asarray(out.values[1]).ravel()[0]) == int(v[ml].sum())
        top, htop = sc.top(ql, "v", 25), sc.host_top(ql, "v", 25)
        assert np.array_equal(top._entries, htop._entries)
        assert np.array_equal(np.asarray(top.values), np.sort(v[ml])[:25])
        assert ml[np.asarray(top.rows)].all()
    finally:
        sc.close()
    # the multi-rank driver (one rank here) takes predicates and Or as it takes tuples
    from nvme_strom_amd.parallel.scan import DistributedArrowScan
    ds = DistributedArrowScan(files[codec], torch.device("cuda"))
    try:
        out = ds.scan_where(q)
        assert np.array_equal(out.indices.cpu().numpy(), np.flatnonzero(m))
        assert out.ranges == [(0, 6)] and out.per_rank == [int(m.sum())]
    finally:
        ds.close()
