"""Generators for the select-list tests (tests/test_arrow_project_cpu.py,
tests/test_gpu_arrow_project.py): hand-built batch tables, bitmaps and
column buffers for strom_bitmap_to_rows_multi, one runner for its host copy
and its kernel that checks every output byte against the numpy twin
(ops/colproject.host_rows_multi) — sentinels before and past the cursors
included — and the table, qualifiers and pyarrow references of whole scans."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from nvme_strom_amd.ops import colproject as PJ

SENTINEL = 0xA5
GUARD = 72                      # sentinel elements kept behind every output


# ------------------------------------------------------------ kernel cases
@dataclass
class Case:
    name: str
    bitmap: np.ndarray          # uint64[nwords]
    batches: np.ndarray         # (n, 5) int64: 0, 0, nrows, word_base, row_base
    cols: List[PJ.TwinCol]
    want_valid: List[bool]      # the column's validity is asked for

    @property
    def nwords(self) -> int:
        return len(self.bitmap)


def batch_table(rows: Sequence[int], gaps: Optional[Sequence[int]] = None,
                row0: int = 0) -> np.ndarray:
    """Every batch on fresh words; ``gaps[b]``: unused words behind batch b."""
    t = np.zeros((len(rows), 5), np.int64)
    w, r = 0, row0
    for b, n in enumerate(rows):
        t[b] = (0, 0, n, w, r)
        w += (n + 63) // 64 + (gaps[b] if gaps else 0)
        r += n
    return t


def nwords_of(bt: np.ndarray) -> int:
    return int(bt[-1, 3] + (bt[-1, 2] + 63) // 64) if len(bt) else 0


BITMAPS = ("empty", "all", "one_per_word", "top_of_tail", "alternating", "d1000", "d2", "blocks")


def bitmap(kind: str, nwords: int, rng) -> np.ndarray:
    """The bitmap shapes of the kernel tests.  Bits past a batch's rows are
    left set where the shape sets them: the walk ignores them."""
    full = np.uint64(0xFFFFFFFFFFFFFFFF)
    bm = np.zeros(nwords, np.uint64)
    if kind == "all":
        bm[:] = full
    elif kind == "one_per_word":
        bm[:] = np.uint64(1) << rng.integers(0, 64, nwords).astype(np.uint64)
    elif kind == "top_of_tail":
        if nwords:
            bm[-1] = np.uint64(1) << np.uint64(63)
    elif kind == "alternating":
        bm[1::2] = full
    elif kind in ("d1000", "d2"):
        p = 0.001 if kind == "d1000" else 0.5
        bits = (rng.random(nwords * 64) < p).astype(np.uint8)
        bm = np.packbits(bits, bitorder="little").view(np.uint64).copy()
    elif kind == "blocks":
        # whole 256-word blocks: full, empty, empty, full, ...
        for b0 in range(0, nwords, 256):
            if (b0 // 256) % 3 == 0:
                bm[b0:b0 + 256] = full
    elif kind != "empty":
        raise ValueError(kind)
    return bm


def _valid(mode: Optional[str], rows: Sequence[int], rng) -> list:
    """None: no batch has validity; "all": every batch; "some": every other."""
    out = []
    for b, n in enumerate(rows):
        if mode is None or (mode == "some" and b % 2 == 0):
            out.append(None)
        else:
            out.append(rng.integers(0, 256, (n + 7) // 8).astype(np.uint8))
    return out


def fixed_col(width: int, rows: Sequence[int], rng, valid: Optional[str] = None) -> PJ.TwinCol:
    return PJ.TwinCol(PJ.FIXED, width,
                      [rng.integers(0, 256, n * width).astype(np.uint8) for n in rows],
                      _valid(valid, rows, rng))


def bool_col(rows: Sequence[int], rng, valid: Optional[str] = None) -> PJ.TwinCol:
    return PJ.TwinCol(PJ.BOOL, 0, [rng.integers(0, 256, (n + 7) // 8).astype(np.uint8)
                                   for n in rows], _valid(valid, rows, rng))


def str_col(wide: bool, rows: Sequence[int], rng, valid: Optional[str] = None,
            long_row: bool = True, malformed: bool = True) -> PJ.TwinCol:
    """Strings of 3-20 bytes, a fifth of them empty, one 5,000-byte row in
    the largest batch, and (``malformed``) a few offset pairs that are
    negative, decreasing or past the characters."""
    dt = np.int64 if wide else np.int32
    values, aux = [], []
    big = int(np.argmax(rows)) if len(rows) else -1
    for b, n in enumerate(rows):
        ln = np.where(rng.random(n) < 0.2, 0, rng.integers(3, 21, n))
        if long_row and b == big and n > 2:
            ln[n // 2] = 5000
        offs = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
        chars = rng.integers(97, 123, int(offs[-1])).astype(np.uint8)
        if malformed and n > 8:
            for k, r in enumerate(rng.choice(n + 1, 4, replace=False)):
                offs[r] = (-5, int(offs[-1]) + 9, np.iinfo(dt).max, np.iinfo(dt).min)[k]
        values.append(offs.astype(dt).view(np.uint8) if n else np.zeros(0, np.uint8))
        aux.append(chars)
    return PJ.TwinCol(PJ.STR64 if wide else PJ.STR32, 0, values, _valid(valid, rows, rng), aux)


def mixed_cols(ncols: int, rows: Sequence[int], rng) -> tuple:
    """``ncols`` columns cycling through every kind and width, validity on
    some columns and, of those, on some batches only.  Returns (columns,
    want_valid)."""
    makers = [lambda v: fixed_col(8, rows, rng, v), lambda v: str_col(False, rows, rng, v),
              lambda v: fixed_col(1, rows, rng, v), lambda v: bool_col(rows, rng, v),
              lambda v: fixed_col(16, rows, rng, v), lambda v: str_col(True, rows, rng, v),
              lambda v: fixed_col(2, rows, rng, v), lambda v: fixed_col(4, rows, rng, v)]
    modes = [None, "some", "all", "some"]
    cols, want = [], []
    for k in range(ncols):
        mode = modes[k % len(modes)]
        cols.append(makers[k % len(makers)](mode))
        # validity asked for where there is some, and once where there is none
        want.append(mode is not None or k % 5 == 4)
    return cols, want


# ---------------------------------------------------------------- backends
class HostBackend:
    """The C++ host copy over numpy memory."""

    def put(self, arr: np.ndarray):
        a = np.ascontiguousarray(arr).copy()
        return a, a.ctypes.data

    def get(self, h) -> np.ndarray:
        return h

    def call(self, bm, nwords, bt, out, total, cols, tables) -> None:
        rc = PJ.rows_multi_host(bm, nwords, bt, out, total, cols, tables)
        assert rc == 0, rc


class DeviceBackend:
    """The kernel, on the current stream."""

    def __init__(self, device="cuda"):
        import torch
        self.torch, self.device = torch, torch.device(device)

    def put(self, arr: np.ndarray):
        a = np.ascontiguousarray(arr)
        if a.dtype == np.uint64:
            a = a.view(np.int64)
        t = self.torch.from_numpy(a.copy()).to(self.device)
        return t, t.data_ptr()

    def get(self, h) -> np.ndarray:
        return h.cpu().numpy()

    def call(self, bm, nwords, bt, out, total, cols, tables) -> None:
        PJ.bitmap_to_rows_multi(bm, nwords, bt, out, total, cols, tables)
        self.torch.cuda.synchronize(self.device)


def _pack(case: Case) -> tuple:
    """Every buffer of the case in one blob, each 64-byte aligned: (blob,
    (ncols, n, 7) tables with blob offsets in the pointer fields, the mask of
    the pointer fields that are set)."""
    n = len(case.batches)
    tabs = np.zeros((len(case.cols), n, 7), np.int64)
    isptr = np.zeros(tabs.shape, bool)
    chunks, off = [], 0

    def add(a: np.ndarray) -> int:
        nonlocal off
        a = np.asarray(a, np.uint8)
        at = off
        chunks.append(a)
        pad = -len(a) % 64
        chunks.append(np.zeros(pad + 64, np.uint8))
        off += len(a) + pad + 64
        return at

    for k, c in enumerate(case.cols):
        tabs[k, :, 2:5] = case.batches[:, 2:5]
        for b in range(n):
            tabs[k, b, 0], isptr[k, b, 0] = add(c.values[b]), True
            if c.valid[b] is not None:
                tabs[k, b, 1], isptr[k, b, 1] = add(c.valid[b]), True
            if PJ.is_str(c.kind):
                tabs[k, b, 5], isptr[k, b, 5] = add(c.aux[b]), True
                tabs[k, b, 6] = len(c.aux[b])
    blob = np.concatenate(chunks) if chunks else np.zeros(64, np.uint8)
    return blob, tabs, isptr


def _per_row(c: PJ.TwinCol) -> int:
    return 8 if PJ.is_str(c.kind) else (1 if c.kind == PJ.BOOL else c.width)


def run_and_check(be, cases: Sequence[Case], total0: int = 0, cur0: int = 0) -> dict:
    """The cases' calls one after the other into the same outputs, cursors
    starting at ``total0`` rows and ``cur0`` characters: every output byte
    equals the twin's, the cursors are the sums, and nothing before the
    starting positions or at and past the final ones was written.  Returns
    the final cursors."""
    first = cases[0]
    ncols = len(first.cols)
    want_ids, want = [], [dict(vals=[], valid=[], chars=[]) for _ in range(ncols)]
    nch = [cur0] * ncols
    for case in cases:
        ids, outs = PJ.host_rows_multi(case.bitmap, case.batches, case.cols)
        want_ids.append(ids)
        for k, o in enumerate(outs):
            if PJ.is_str(case.cols[k].kind):
                want[k]["vals"].append((o.values + nch[k]).astype("<i8").view(np.uint8))
                want[k]["chars"].append(o.chars)
                nch[k] += len(o.chars)
            else:
                want[k]["vals"].append(np.ascontiguousarray(o.values).reshape(-1))
            want[k]["valid"].append(o.valid)
    want_ids = np.concatenate(want_ids)
    nsel = len(want_ids)
    cap = total0 + nsel + GUARD
    h_out, _ = be.put(np.full(cap, -0x5A5A5A5A5A5A5A5B, np.int64))
    h_tot, _ = be.put(np.array([total0], np.int64))
    h_cur, a_cur = be.put(np.full(ncols, cur0, np.int64))
    h_vals, h_valid, h_chars, specs = [], [], [], []
    for k, c in enumerate(first.cols):
        per = _per_row(c)
        # 16-byte aligned whatever the width: the buffer starts a fresh allocation
        hv, av = be.put(np.full(cap * per, SENTINEL, np.uint8))
        hk, ak = be.put(np.full(cap, SENTINEL, np.uint8)) if first.want_valid[k] else (None, 0)
        hc, ac = (None, 0)
        if PJ.is_str(c.kind):
            hc, ac = be.put(np.full(nch[k] + GUARD, SENTINEL, np.uint8))
        h_vals.append(hv), h_valid.append(hk), h_chars.append(hc)
        specs.append((c.kind, c.width, av, ak, ac, a_cur + 8 * k if PJ.is_str(c.kind) else 0))
    cols = PJ.proj_cols(specs)
    keep = []
    for case in cases:
        assert [(_per_row(c), c.kind) for c in case.cols] == \
            [(_per_row(c), c.kind) for c in first.cols]
        blob, tabs, isptr = _pack(case)
        h_blob, base = be.put(blob)
        tabs = np.where(isptr, tabs + base, tabs)
        h_tabs, _ = be.put(tabs)
        h_bm, _ = be.put(case.bitmap if case.nwords else np.zeros(1, np.uint64))
        h_bt, _ = be.put(case.batches)
        keep += [h_blob, h_tabs, h_bm, h_bt]
        be.call(h_bm, case.nwords, h_bt, h_out, h_tot, cols, h_tabs)
    # ---- compare
    name = "+".join(c.name for c in cases)
    got = be.get(h_out)
    assert int(be.get(h_tot)[0]) == total0 + nsel, name
    assert np.array_equal(got[total0:total0 + nsel], want_ids), name
    assert (got[:total0] == got[-1]).all() and (got[total0 + nsel:] == got[-1]).all(), name
    curs = be.get(h_cur)
    for k, c in enumerate(first.cols):
        per = _per_row(c)
        v = be.get(h_vals[k]).view(np.uint8)
        exp = np.concatenate(want[k]["vals"]) if nsel else np.zeros(0, np.uint8)
        lo, hi = total0 * per, (total0 + nsel) * per
        bad = np.flatnonzero(v[lo:hi] != exp)
        assert not len(bad), (name, k, "values", bad[:8] // per)
        assert (v[:lo] == SENTINEL).all() and (v[hi:] == SENTINEL).all(), (name, k, "guard")
        if first.want_valid[k]:
            ok = be.get(h_valid[k])
            exp = np.concatenate(want[k]["valid"])
            assert np.array_equal(ok[total0:total0 + nsel], exp), (name, k, "validity")
            assert (ok[:total0] == SENTINEL).all() and (ok[total0 + nsel:] == SENTINEL).all(), \
                (name, k, "validity guard")
        if PJ.is_str(c.kind):
            ch = be.get(h_chars[k])
            exp = np.concatenate(want[k]["chars"])
            assert int(curs[k]) == nch[k], (name, k, "character cursor")
            bad = np.flatnonzero(ch[cur0:nch[k]] != exp)
            assert not len(bad), (name, k, "characters", bad[:8])
            assert (ch[:cur0] == SENTINEL).all() and (ch[nch[k]:] == SENTINEL).all(), \
                (name, k, "character guard")
        else:
            assert int(curs[k]) == cur0, (name, k, "cursor of a column without characters")
    return dict(rows=total0 + nsel, chars=nch)


ROWS3 = (1, 65, 4097)           # a batch boundary inside a block, tails no multiple of 64
NWORDS = (1, 255, 256, 257, 600)


def kernel_cases(rng) -> List[Case]:
    """Every bitmap shape at every word count on one batch and on the three
    batches, with two columns (8 bytes with validity on some batches, utf8);
    then ncols 1 / 2 / 7 / 16 of every kind on about 40,000 rows in batches
    of 1 / 65 / 4,097 rows repeated, at densities 1/2 and 1/1000 and with
    whole empty blocks."""
    out = []
    for nw in NWORDS:
        for rows in ((nw * 64 - 7,), ROWS3):
            bt = batch_table(rows)
            # the three batches take 68 words: at other word counts the
            # bitmap stops short of them or runs past them
            for kind in BITMAPS:
                cols = [fixed_col(8, rows, rng, "some"), str_col(False, rows, rng, None)]
                out.append(Case(f"{kind}/{nw}w/{len(rows)}b", bitmap(kind, nw, rng), bt, cols,
                                [True, False]))
    rows = ROWS3 * 9 + (1000, 2477)                 # 40,944 rows, 29 batches
    bt = batch_table(rows, gaps=[b % 7 == 3 for b in range(len(rows))])
    nw = nwords_of(bt)
    for ncols in (1, 2, 7, 16):
        for kind in ("d2", "d1000", "blocks"):
            cols, want = mixed_cols(ncols, rows, rng)
            out.append(Case(f"{kind}/{ncols}c", bitmap(kind, nw, rng), bt, cols, want))
    return out


# ------------------------------------------------------------- whole scans
def table(n: int = 3000, seed: int = 5):
    """arrowgen.table and the integer widths it lacks, a large_binary column
    and two foreign keys."""
    import pyarrow as pa
    import arrowgen
    t = arrowgen.table(n, seed)
    rng = np.random.default_rng(seed + 1)
    nulls = lambda p=0.07: rng.random(n) < p
    bins = [bytes(rng.integers(0, 256, int(k)).astype(np.uint8)) for k in rng.integers(0, 9, n)]
    more = {
        "i16": pa.array(rng.integers(-2**15, 2**15, n).astype(np.int16), mask=nulls()),
        "i32": pa.array(rng.integers(-2**31, 2**31, n).astype(np.int32)),
        "u8": pa.array(rng.integers(0, 256, n).astype(np.uint8), mask=nulls()),
        "u16": pa.array(rng.integers(0, 2**16, n).astype(np.uint16)),
        "u64": pa.array(rng.integers(0, 2**64, n, dtype=np.uint64), mask=nulls()),
        "f64n": pa.array(np.where(rng.random(n) < 0.1, np.nan, rng.normal(0, 1, n)),
                         mask=nulls()),
        "lbin": pa.array(bins, pa.large_binary(), mask=nulls()),
        "fa": pa.array(rng.integers(0, 400, n).astype(np.int32), mask=nulls(0.03)),
        "fb": pa.array(rng.integers(0, 50, n).astype(np.uint16)),
    }
    for k, v in more.items():
        t = t.append_column(k, v)
    return t


# every kind a select list takes, in chunks of at most 16
SELECTS = [["i8", "i16", "i32", "i64", "u8", "u16", "u32", "u64", "f32", "f64", "f64n", "b",
            "d32", "ts", "t32", "dur"],
           ["dec", "dict", "idict", "s", "ls", "bin", "lbin", "i64"],
           ["s"], ["b", "f64"]]


def dimensions():
    """(keys, attrs) of the two JoinTables of the scan tests."""
    ka = np.arange(0, 400, 3, dtype=np.int64)
    kb = np.arange(0, 50, 2, dtype=np.int64)
    return {"fa": (ka, {"cat": [None if k % 11 == 0 else f"c{k % 7}" for k in ka.tolist()]}),
            "fb": (kb, {"grp": [int(k % 4) for k in kb.tolist()]})}


def quals_and_mask():
    import pyarrow.compute as pc
    from nvme_strom_amd.ops.colpred import P
    return [P("f64") > 0.25, P("i64") < 5 * 10**11], \
        lambda t: pc.and_kleene(pc.greater(t.column("f64"), 0.25),
                                pc.less(t.column("i64"), 5 * 10**11))


def reference(tbl, mask, names: Sequence[str]):
    """pyarrow's filtered select: nulls of the mask select nothing."""
    return tbl.filter(mask).select(list(names))


def same_table(got, want) -> None:
    """Equal schemas and columns; NaNs equal NaNs, dictionary columns by
    their decoded values."""
    import pyarrow as pa
    assert got.schema.names == want.schema.names
    assert got.num_rows == want.num_rows, (got.num_rows, want.num_rows)
    for name in want.schema.names:
        a, b = got.column(name).combine_chunks(), want.column(name).combine_chunks()
        assert a.type == b.type or pa.types.is_dictionary(b.type), (name, a.type, b.type)
        if pa.types.is_dictionary(b.type):
            assert pa.types.is_dictionary(a.type) and a.type.index_type == b.type.index_type and \
                a.type.value_type == b.type.value_type, (name, a.type, b.type)
            a, b = a.cast(b.type.value_type), b.cast(b.type.value_type)
        if pa.types.is_floating(b.type):
            assert a.is_valid().equals(b.is_valid()), name
            x, y = (np.asarray(v.fill_null(0)) for v in (a, b))
            assert np.array_equal(x, y, equal_nan=True), name
        else:
            assert a.equals(b), name
