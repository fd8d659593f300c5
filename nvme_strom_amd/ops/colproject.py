"""A select list in one walk of the selection bitmap
(csrc/kernels/colproject.hip): the selected rows' ids and up to MAX_COLS
projected columns — fixed-width values, bools, utf8/binary characters —
written at the same output positions behind shared device cursors.

``bitmap_to_rows_multi`` launches the kernel, ``rows_multi_host`` its C++
host copy over numpy buffers, and ``host_rows_multi`` is the numpy twin, a
formulation of its own (``np.flatnonzero`` over the unpacked bits of each
batch's words, fancy indexing) that the tests hold both against."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .. import _native as N

MAX_COLS = 16                                   # STROM_PROJ_MAX_COLS
FIXED, BOOL, STR32, STR64 = 1, 2, 3, 4          # STROM_PROJ_*
WIDTHS = (1, 2, 4, 8, 16)
QUAL_BATCH_FIELDS = 7                           # struct strom_qual_batch, u64 each

# struct strom_proj_col
PROJ_COL = np.dtype([("kind", "<i4"), ("width", "<u4"), ("table", "<u8"), ("out", "<u8"),
                     ("out_valid", "<u8"), ("out_chars", "<u8"), ("char_cursor", "<u8")])
assert PROJ_COL.itemsize == 48


def is_str(kind: int) -> bool:
    return kind in (STR32, STR64)


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed (rc={rc})")


def proj_cols(specs: Sequence[tuple]) -> np.ndarray:
    """The descriptor array of a select list: per column (kind, width, out,
    out_valid, out_chars, char_cursor) as addresses (0: none); ``table`` is
    filled in per call by ``with_tables``."""
    if not 1 <= len(specs) <= MAX_COLS:
        raise ValueError(f"a select list holds 1 to {MAX_COLS} columns")
    a = np.zeros(len(specs), PROJ_COL)
    for i, (kind, width, out, out_valid, out_chars, cursor) in enumerate(specs):
        if kind not in (FIXED, BOOL, STR32, STR64) or (kind == FIXED and width not in WIDTHS):
            raise ValueError(f"column {i}: kind {kind} width {width}")
        a[i] = (kind, width, 0, out, out_valid or 0, out_chars or 0, cursor or 0)
    return a


def stack_tables(tables: Sequence[np.ndarray]) -> np.ndarray:
    """The columns' strom_qual_batch tables, each (nbatches, 7), as one
    (ncols, nbatches, 7) int64 array: one upload per group."""
    out = np.stack([np.ascontiguousarray(t, dtype=np.int64) for t in tables])
    if out.ndim != 3 or out.shape[2] != QUAL_BATCH_FIELDS:
        raise ValueError("tables: (nbatches, 7) strom_qual_batch rows per column")
    return out


def with_tables(cols: np.ndarray, base: int, nbatches: int) -> np.ndarray:
    """``cols`` with column i's table at ``base`` + i tables of ``nbatches``
    rows: the address of ``stack_tables``' array, wherever it lives."""
    c = cols.copy()
    c["table"] = base + np.arange(len(c), dtype=np.uint64) * np.uint64(
        nbatches * QUAL_BATCH_FIELDS * 8)
    return c


def bitmap_to_rows_multi(bitmap, nwords: int, batches, out, cursor, cols: np.ndarray,
                         tables, stream=None) -> None:
    """Append the global row ids (int64) of the set bits at ``out[cursor]``
    and each column's values at the same positions; ``cursor`` (int64[1],
    device) and the string columns' character cursors advance.  ``batches``:
    the (nbatches, 5) strom_filter_batch table on the device; ``tables``: the
    (ncols, nbatches, 7) device tensor of ``stack_tables``; ``cols``:
    ``proj_cols`` of device addresses."""
    from ._util import ptr, require_cuda, stream_handle
    require_cuda(bitmap, "bitmap")
    require_cuda(tables, "tables")
    if out.dtype.itemsize != 8:
        raise ValueError("out must be int64")
    nb = batches.shape[0]
    if tables.dim() != 3 or tuple(tables.shape) != (len(cols), nb, QUAL_BATCH_FIELDS) or \
            tables.element_size() != 8:
        raise ValueError("tables: (ncols, nbatches, 7) int64 of the same batches")
    if bitmap.numel() < nwords:
        raise ValueError("bitmap too small")
    c = with_tables(cols, ptr(tables), nb)
    _check(N.lib().strom_bitmap_to_rows_multi(ptr(bitmap), nwords, ptr(batches), nb, ptr(out),
                                              ptr(cursor), c.ctypes.data, len(c),
                                              stream_handle(stream)), "bitmap_to_rows_multi")


def rows_multi_host(bitmap: np.ndarray, nwords: int, batches: np.ndarray, out: np.ndarray,
                    cursor: np.ndarray, cols: np.ndarray, tables: np.ndarray) -> int:
    """The C++ host copy over numpy memory (every address in ``batches``,
    ``tables`` and ``cols`` a host address).  Returns the library's code."""
    b = np.ascontiguousarray(batches, dtype=np.int64)
    t = np.ascontiguousarray(tables, dtype=np.int64)
    c = with_tables(cols, t.ctypes.data, b.shape[0]) if len(cols) else cols
    return int(N.lib().strom_bitmap_to_rows_multi_host(
        bitmap.ctypes.data, nwords, b.ctypes.data, b.shape[0], out.ctypes.data,
        cursor.ctypes.data, c.ctypes.data if len(c) else 0, len(c)))


# ------------------------------------------------------------ numpy twin
@dataclass
class TwinCol:
    """One column of the twin's select list, per record batch: ``values``
    the data buffer as uint8 (FIXED: nrows * width bytes; BOOL: the packed
    bits; STR: nrows + 1 offsets of 4 / 8 bytes), ``valid`` the packed
    validity bits or None, ``aux`` the characters (STR)."""
    kind: int
    width: int
    values: List[np.ndarray]
    valid: List[Optional[np.ndarray]]
    aux: List[Optional[np.ndarray]] = field(default_factory=list)


@dataclass
class TwinOut:
    values: np.ndarray                  # FIXED (n, width) uint8; BOOL uint8; STR int64 starts
    valid: np.ndarray                   # uint8 0/1
    chars: Optional[np.ndarray] = None  # STR: the characters, starts relative to its first


def _bits(packed: np.ndarray, n: int) -> np.ndarray:
    return np.unpackbits(np.asarray(packed, np.uint8), bitorder="little")[:n]


def host_rows_multi(bitmap: np.ndarray, batches: np.ndarray,
                    cols: Sequence[TwinCol]) -> Tuple[np.ndarray, List[TwinOut]]:
    """(row ids, per column its TwinOut) of the bitmap's selection.
    ``batches``: (nbatches, >= 5) with nrows, word_base and row_base in
    fields 2-4.  A word belongs to the last batch that starts at or before
    it; its bits at or past that batch's rows select nothing."""
    bm = np.ascontiguousarray(bitmap).view(np.uint64)
    nb = len(batches)
    ids: List[np.ndarray] = []
    parts: List[List[tuple]] = [[] for _ in cols]
    for b in range(nb):
        nrows, w0 = int(batches[b][2]), int(batches[b][3])
        w1 = min(int(batches[b + 1][3]) if b + 1 < nb else len(bm), len(bm))
        if w1 <= w0:
            continue
        bits = np.unpackbits(bm[w0:w1].view(np.uint8), bitorder="little")[:nrows]
        sel = np.flatnonzero(bits)
        ids.append(sel.astype(np.int64) + int(batches[b][4]))
        for k, c in enumerate(cols):
            ok = np.ones(len(sel), np.uint8) if c.valid[b] is None else _bits(c.valid[b], nrows)[sel]
            v = np.asarray(c.values[b], np.uint8)
            if c.kind == FIXED:
                parts[k].append((v[:nrows * c.width].reshape(nrows, c.width)[sel], ok, None))
            elif c.kind == BOOL:
                parts[k].append((_bits(v, nrows)[sel], ok, None))
            else:
                ow = "<i8" if c.kind == STR64 else "<i4"
                offs = v[:(nrows + 1) * int(ow[-1])].view(ow).astype(np.int64) if nrows else \
                    np.zeros(1, np.int64)
                aux = np.asarray(c.aux[b], np.uint8)
                a, e = offs[sel], offs[sel + 1] if nrows else offs[:0]
                good = (a >= 0) & (e >= a) & (e <= len(aux))
                ln = np.where(good, e - a, 0)
                st = np.cumsum(ln) - ln
                idx = np.repeat(np.where(good, a, 0) - st, ln) + np.arange(int(ln.sum()))
                parts[k].append((ln, ok, aux[idx]))
    rows = np.concatenate(ids) if ids else np.zeros(0, np.int64)
    outs = []
    for c, p in zip(cols, parts):
        ok = np.concatenate([x[1] for x in p]) if p else np.zeros(0, np.uint8)
        if is_str(c.kind):
            ln = np.concatenate([x[0] for x in p]) if p else np.zeros(0, np.int64)
            chars = np.concatenate([x[2] for x in p]) if p else np.zeros(0, np.uint8)
            outs.append(TwinOut((np.cumsum(ln) - ln).astype(np.int64), ok, chars))
        else:
            shape = (0, c.width) if c.kind == FIXED else (0,)
            outs.append(TwinOut(np.concatenate([x[0] for x in p]) if p else
                                np.zeros(shape, np.uint8), ok))
    return rows, outs
