"""LIKE / contains / endswith on the CPU: the numpy twin of the kernel
(colpred.evaluate) against the `re` reference of tests/likegen.py on generated
tables and against pyarrow.compute on an Arrow file through host_scan_where,
the library's host copy of the kernel against the twin word for word (bytes
that are not UTF-8 included), the compiler's refusals, and the host copy under
ASan + UBSan (csrc/tests/collike_fuzz.cc)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

import likegen as L  # noqa: E402
from nvme_strom_amd.ops import colpred as CP  # noqa: E402
from nvme_strom_amd.ops.colpred import Or, P, Pred  # noqa: E402

CODECS = [None, "lz4", "zstd"]
STR_COLS = ["s", "ls", "bin", "dict"]


def _twin(t, c):
    return [CP.evaluate(c, L.host_values(t, b), b.valid, b.nrows) for b in t.batches]


@pytest.fixture(scope="module")
def tables():
    """(dt, utf8, malformed) -> Table, built once."""
    out = {}
    for dt in ("s4", "s8"):
        for utf8 in (True, False):
            for bad in (False, True):
                out[dt, utf8, bad] = L.like_table(dt, utf8, np.random.default_rng(40 + bad), bad)
    return out


# ------------------------------------------------------------------ the twin
@pytest.mark.parametrize("utf8", [True, False], ids=["utf8", "binary"])
@pytest.mark.parametrize("dt", ["s4", "s8"])
def test_twin_equals_re_reference(tables, dt, utf8):
    """evaluate == fullmatch of the translated regular expression, every
    pattern class, plain and negated, with and without malformed offsets."""
    for bad in (False, True):
        t = tables[dt, utf8, bad]
        assert max(len(L.row_bytes(b, b.nrows - 1) or b"") for b in t.batches if b.nrows) > 0
        for name, op, v in L.like_preds(utf8):
            for neg in (False, True):
                c = L.compile_like(op, v, dt, utf8, neg)
                assert c.op == CP.QOP_STR_LIKE and c.type == (CP.COL_STR64 if dt == "s8"
                                                              else CP.COL_STR32)
                want = L.like_ref(t, op, v, utf8, neg)
                for k, (g, w) in enumerate(zip(_twin(t, c), want)):
                    assert np.array_equal(g, w), (name, neg, bad, k, np.flatnonzero(g != w)[:5])


def test_table_covers_what_it_claims():
    t = L.like_table("s4", True, np.random.default_rng(1))
    assert [b.nrows for b in t.batches] == L.GEOMETRY
    seen = set()
    for b in t.batches:
        offs, chars = b.values
        if b.nrows:
            assert offs[-1] == len(chars)            # the last row ends at aux_len
        for i in range(b.nrows):
            seen.add((offs[i + 1] - offs[i], offs[i] % 4))
    for n in (0, 1, 9, 17, 40, 255, 256, 257, 1000, 5000):
        for a in range(4):
            assert (n, a) in seen, (n, a)


def test_malformed_offsets_never_select(tables):
    for dt in ("s4", "s8"):
        t = tables[dt, True, True]
        for op, v in (("like", "%"), ("not like", "%"), ("contains", ""), ("not suffix", "zz")):
            c = CP.compile_pred(Pred("c", op, v), L.column(dt, True))
            nbad = 0
            for b, g in zip(t.batches, _twin(t, c)):
                bad = np.array([L.row_bytes(b, i) is None for i in range(b.nrows)], bool)
                nbad += int(bad.sum())
                assert not g[bad].any(), (dt, op)
            assert nbad >= 3 * 6


def test_compiled_form():
    col = L.column("s4", True)
    c = CP.compile_pred(P("c").like("ab%c_d%_"), col)
    assert c.flags == CP.FLAG_LIKE_WILD | CP.FLAG_LIKE_UTF8 and c.nconst == 1
    head, tail, segs = c.patterns[0]
    assert head and tail and segs == [([(0, b"ab")], 0, 2), ([(0, b"c"), (1, b"d")], 0, 3),
                                      ([], 1, 1)]
    w = np.frombuffer(c.offs, np.uint32)
    assert w[0] == 1 and list(w[1:4]) == [CP.LIKE_HEAD | CP.LIKE_TAIL, 6, 3]
    assert len(c.consts) % 4 == 0 and len(c.offs) % 4 == 0
    # contains / endswith are %x% / %x with the specials literal; no wildcard flag
    c = CP.compile_pred(P("c").contains("a_%"), col)
    assert c.flags == 0 and c.patterns == [(False, False, [([(0, b"a_%")], 0, 3)])]
    c = CP.compile_pred(P("c").endswith(["x", "x", "\\"]), col)
    assert c.nconst == 2 and c.patterns[0] == (False, True, [([(0, b"\\")], 0, 1)])
    c = CP.compile_pred(P("c").not_like("%%a%%"), col)
    assert c.flags == CP.FLAG_NEGATE and c.patterns == [(False, False, [([(0, b"a")], 0, 1)])]
    # on a binary column _ is one byte: no utf8 flag
    c = CP.compile_pred(P("c").like(b"a_"), L.column("s8", False))
    assert c.flags == CP.FLAG_LIKE_WILD and c.type == CP.COL_STR64
    assert CP.compile_pred(P("c").like(""), col).patterns == [(True, True, [])]
    assert CP.compile_pred(P("c").like("%"), col).patterns == [(False, False, [])]


# ----------------------------------------------------------------- refusals
def test_compile_time_refusals():
    from nvme_strom_amd.utils.arrow_ipc import Column
    col = L.column("s4", True)
    for bad in ("a\\b", "abc\\", "\\", "%\\x%"):
        with pytest.raises(ValueError, match="backslash"):
            CP.compile_pred(P("c").like(bad), col)
    with pytest.raises(ValueError, match="MAX_LIKE_BYTES"):
        CP.compile_pred(P("c").like("a" * (CP.MAX_LIKE_BYTES + 1)), col)
    with pytest.raises(ValueError, match="MAX_LIKE_SEGMENTS"):
        CP.compile_pred(P("c").like("%".join("ab" for _ in range(CP.MAX_LIKE_SEGMENTS + 1))), col)
    with pytest.raises(ValueError, match="MAX_LIKE_PATTERNS"):
        CP.compile_pred(P("c").contains(["k%d" % k for k in range(CP.MAX_LIKE_PATTERNS + 1)]), col)
    with pytest.raises(ValueError, match="MAX_QUAL_BYTES"):
        CP.compile_pred(P("c").endswith([("%03d" % k) * 1300 for k in range(20)]), col)
    with pytest.raises(ValueError, match="one pattern"):
        CP.compile_pred(P("c").like(["a", "b"]), col)
    for p in (P("c").like("a%"), P("c").contains("a"), P("c").endswith("a"), P("c").not_like("a")):
        with pytest.raises(ValueError, match=r"\(int\).*needs utf8/binary"):
            CP.compile_pred(p, Column("c", "int", 32, True))
    with pytest.raises(TypeError):
        CP.compile_pred(P("c").like(5), col)
    # the limits themselves compile
    assert CP.compile_pred(P("c").like("a" * CP.MAX_LIKE_BYTES), col).nconst == 1


# ------------------------------------------------------- the library's host copy
def _host_copy(t, c):
    h = L.HostTable(t)
    bm = np.zeros(t.nwords, np.uint64)
    n = CP.like_host(c, h.qtab, t.nwords, bm)
    assert n == L.popcount(bm)
    return bm


@pytest.mark.parametrize("utf8", [True, False], ids=["utf8", "binary"])
def test_host_copy_equals_twin(tables, utf8):
    """strom_column_like_host == evaluate, word for word, on the generated
    tables (malformed offsets too) and on rows of random bytes, where a utf8
    column's `_` is defined by these two and the kernel alone."""
    rng = np.random.default_rng(77)
    junk = [bytes(rng.choice(np.array([0x61, 0x62, 0x80, 0xA9, 0xBF, 0xC3, 0xE2, 0xF0, 0x5F], np.uint8),
                             int(n))) for n in rng.integers(0, 24, 400)]
    junk += [bytes(rng.integers(0x80, 0xC0, 300, dtype=np.uint8)), b"a" + bytes([0x80]) * 299 + b"b"]
    jt = L.like_table("s4", utf8, rng, False, [64, 3400, 1], [None, "dirty", None], rows=junk)
    jpreds = [("like", x) for x in ("_", "__", "%_", "_%", "a_b", "%a_", "_a%", "%_b_%", "%a__b%", "a%_",
                                    "%__", "___%", "%b_a%_", "%_é%", "é_%", "%_é")]
    enc = (lambda s: s) if utf8 else (lambda s: s.encode())
    for t, preds in ((tables["s4", utf8, True], [(op, v) for _, op, v in L.like_preds(utf8)]),
                     (tables["s8", utf8, False], [(op, v) for _, op, v in L.like_preds(utf8)][::3]),
                     (jt, [(op, enc(v)) for op, v in jpreds])):
        for op, v in preds:
            for neg in (False, True):
                c = L.compile_like(op, v, t.dt, utf8, neg)
                want = L.pack_words(t, _twin(t, c))
                got = _host_copy(t, c)
                assert np.array_equal(got, want), (t.dt, op, v, neg, np.flatnonzero(got != want)[:4])
    # the combination modes and the count
    t = tables["s4", utf8, False]
    c = L.compile_like("contains", enc("a"), "s4", utf8)
    pred = L.pack_words(t, _twin(t, c))
    old = rng.integers(0, 1 << 64, t.nwords, dtype=np.uint64, endpoint=False)
    orw = rng.integers(0, 1 << 64, t.nwords, dtype=np.uint64, endpoint=False)
    h = L.HostTable(t)
    for use_or, and_dst in ((False, True), (True, False), (True, True)):
        bm = old.copy()
        n = CP.like_host(c, h.qtab, t.nwords, bm, orw if use_or else None, and_dst)
        exp = L.expected_words(pred, orw if use_or else None, and_dst, old)
        assert np.array_equal(bm, exp) and n == L.popcount(exp)


def test_host_copy_refuses_bad_operands():
    import dataclasses
    t = L.like_table("s4", True, np.random.default_rng(3), geometry=[40], validity=[None],
                     rows=[b"abxc", b"ab", b"", b"xabyc", b"abc"])
    h = L.HostTable(t)
    c = L.compile_like("like", "%ab_c%", "s4", True)
    w = np.frombuffer(c.offs, np.uint32).copy()
    for at, val in ((0, len(w)), (3, 1 << 20), (4, len(w) - 1), (len(w) - 2, len(c.consts)),
                    (len(w) - 1, 0), (len(w) - 2, 2)):
        x = w.copy()
        x[at] = val
        bad = dataclasses.replace(c, offs=x.tobytes(), _dev={})
        with pytest.raises(RuntimeError, match="rc=-22"):
            CP.like_host(bad, h.qtab, t.nwords, np.zeros(t.nwords, np.uint64))


# ----------------------------------------------------------------- pyarrow
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
def test_host_scan_where_equals_pyarrow(files, codec):
    """Row ids of host_scan_where == pc.match_like / match_substring /
    ends_with on string, large_string, binary and dictionary columns (the
    dictionary decoded for pyarrow), nulls never selected."""
    from nvme_strom_amd.models import arrow_scan as S
    tbl = L.arrow_table()
    nsel = 0
    for col in STR_COLS:
        for label, op, v in L.SCAN_PREDS:
            want = np.flatnonzero(L.pc_mask(tbl, col, op, v))
            got = S.host_scan_where(files[codec], [Pred(col, op, v)]).indices
            assert np.array_equal(got, want), (col, label)
            nsel += len(want)
    assert nsel > 10000
    # in an Or, in a conjunction, with batches=
    q = [Or(P("s").like("%green"), P("bin").contains(b"special"), P("dict").endswith("o")),
         P("ls").not_like("a%"), P("v") < 700]
    m = (L.pc_mask(tbl, "s", "like", "%green") | L.pc_mask(tbl, "bin", "contains", "special") |
         L.pc_mask(tbl, "dict", "suffix", "o")) & L.pc_mask(tbl, "ls", "not like", "a%") & \
        (tbl.column("v").to_numpy() < 700)
    assert np.array_equal(S.host_scan_where(files[codec], q).indices, np.flatnonzero(m))
    part = S.host_scan_where(files[codec], q, batches=(2, 5)).indices
    assert np.array_equal(part, np.flatnonzero(m)[(np.flatnonzero(m) >= 2000) &
                                                  (np.flatnonzero(m) < 5000)])
    agg = S.host_aggregate(files[codec], [P("s").like("%green%")], [("count", None), ("sum", "v")])
    mg = L.pc_mask(tbl, "s", "like", "%green%")
    assert agg.selected == int(mg.sum())
    with pytest.raises(ValueError, match=r"\(int\)"):
        S.host_scan_where(files[codec], [P("v").like("1%")])


def test_dictionary_of_the_largest_size_is_fast():
    """A MAX_LUT_BITS-entry dictionary goes through the twin in seconds (no
    Python loop per byte), and its LUT is right."""
    import time
    from nvme_strom_amd.utils.arrow_ipc import Column, DictEncoding
    n = CP.MAX_LUT_BITS
    words = [b"w%07d-%s" % (k, b"green" if k % 3 == 0 else b"gr\xc3\xa9y") for k in range(n)]
    offs = np.concatenate([[0], np.cumsum([len(w) for w in words])]).astype(np.int64)
    chars = np.frombuffer(b"".join(words), np.uint8)
    col = Column("c", "utf8", nbuffers=3, dictionary=DictEncoding(1, 32, True))
    k = np.arange(n)
    t0 = time.time()
    for p, want in ((P("c").like("w%5-gr_y"), (k % 10 == 5) & (k % 3 != 0)),
                    (P("c").contains("00-green"), (k % 100 == 0) & (k % 3 == 0)),
                    (P("c").like("w____1__%n"), (k // 100 % 10 == 1) & (k % 3 == 0)),
                    (P("c").not_like("%y"), k % 3 == 0)):
        c = CP.compile_pred(p, col, dictionary=((offs, chars), None))
        assert c.op == CP.QOP_LUT and c.nconst == n
        assert np.array_equal(c.lut, want), p
    assert time.time() - t0 < 30


# --------------------------------------------------------------- multi-rank
def test_distributed_scan_takes_every_spelling(files, monkeypatch):
    """DistributedArrowScan (one rank) plans its record-batch ranges from the
    columns of P(...) predicates and Or clauses as from tuples, and hands
    the list on unchanged."""
    torch = pytest.importorskip("torch")
    from nvme_strom_amd.models import arrow_scan as S
    from nvme_strom_amd.parallel import scan as PS
    from nvme_strom_amd.utils.arrow_ipc import read_metadata

    class _HostScan:
        def __init__(self, path, device, **kw):
            self.path, self.meta = path, read_metadata(path)

        def scan_where(self, quals, project=None, batches=None):
            out = S.host_scan_where(self.path, quals, project, batches, meta=self.meta)
            return S.ScanOut(out.rows, len(out.indices), torch.from_numpy(out.indices), {})

        def close(self):
            pass
    monkeypatch.setattr(PS, "ArrowScan", _HostScan)
    tbl = L.arrow_table()
    ds = PS.DistributedArrowScan(files["lz4"], torch.device("cpu"))
    seen = []
    plan = ds.ranges
    monkeypatch.setattr(ds, "ranges", lambda names: seen.append(list(names)) or plan(names))
    q = [Or(P("s").like("%green"), P("bin").contains(b"special")), P("ls").not_like("a%"),
         ("dict", "suffix", "o"), ("v", 0, 700)]
    m = (L.pc_mask(tbl, "s", "like", "%green") | L.pc_mask(tbl, "bin", "contains", "special")) & \
        L.pc_mask(tbl, "ls", "not like", "a%") & L.pc_mask(tbl, "dict", "suffix", "o") & \
        (tbl.column("v").to_numpy() <= 700)
    out = ds.scan_where(q)
    assert seen == [["s", "bin", "ls", "dict", "v"]] and out.ranges == [(0, 6)]
    assert np.array_equal(out.indices.numpy(), np.flatnonzero(m)) and out.selected == int(m.sum())
    ds.close()


# ---------------------------------------------------------------- sanitizer
def test_collike_fuzz_asan():
    """The host copy of the kernel built with ASan + UBSan
    (csrc/tests/collike_fuzz.cc): random valid-UTF-8 and binary rows x random
    patterns against a backtracking matcher written there, random malformed
    bytes and offsets against a second evaluation: exits 0."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if shutil.which("make") is None or not (
            os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))):
        pytest.skip("no make / hipcc")
    r = subprocess.run(["make", "-s", "build/collike_fuzz"], cwd=root, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([os.path.join(root, "build", "collike_fuzz"), "3000"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "3000 cases ok" in r.stdout
