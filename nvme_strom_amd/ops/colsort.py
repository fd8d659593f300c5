"""ORDER BY on several columns over a scan's compacted outputs
(csrc/kernels/colsort.hip): the normalizer of ``order_by``, the wrappers of
the encode / radix pass / gather launches and of their C++ host copies, and a
numpy twin.

The order is ops/coltopk.py's, column by column: (class, key) ascending,
class 0 a value, 1 a NaN, 2 a null — in both directions —, ``key`` the
order-preserving key of the value (-0.0 taken as +0.0), every bit inverted
for a descending column, 0 for a NaN or a null; rows equal in every column
stay in the order they came in (file order).  It is total, so the kernels are
compared with the twin — coltopk's ``encode`` per column, then ``np.lexsort``,
a formulation that shares nothing with the passes — element for element.

Device state, all the caller's: two uint64 key arrays and two uint32
permutation arrays of n entries — 24 bytes per selected row — plus a work
table of ``work_bytes(n)`` (256 counts per tile of ``TILE`` keys and 256
totals, 4 bytes each).  n < 2**32.  A column costs one 8-bit pass per byte of
its storage type, and one more over its classes when it is a float type or
has a validity array; a pass is three launches (histogram, scan, scatter)."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import coltopk as T

MAX_KEYS = 4
MAX_COLS = 16                                   # STROM_SORT_MAX_COLS
TILE = 4096                                     # STROM_SORT_TILE
SCAN_THREADS = 256                              # STROM_SORT_SCAN_THREADS
DESC, CLASS, FIRST = 1, 2, 4                    # STROM_SORT_*
FIXED, LEN = 1, 2
WIDTHS = (1, 2, 4, 8, 16)
TYPE_CODE = T.TYPE_CODE
_WIDTH = {code: int(st[1:]) for st, code in TYPE_CODE.items()}
_FLOAT = (TYPE_CODE["f4"], TYPE_CODE["f8"])

# struct strom_sort_col
SORT_COL = np.dtype([("kind", "<u4"), ("width", "<u4"), ("in", "<u8"), ("out", "<u8"),
                     ("in_valid", "<u8"), ("out_valid", "<u8")])
assert SORT_COL.itemsize == 40


# ------------------------------------------------------------ order_by
def order_keys(order_by) -> List[Tuple[object, bool]]:
    """``order_by`` normalized to [(name, descending)]: one item or a list
    of 1 to MAX_KEYS, an item a column name or an E expression (as its
    ExprName), alone or in a pair with "ascending" / "descending"."""
    from .colexpr import E, name_of
    one = lambda x: isinstance(x, (str, E))
    pair = lambda x: isinstance(x, tuple) and len(x) == 2 and one(x[0]) and \
        x[1] in ("ascending", "descending")
    items = list(order_by) if isinstance(order_by, (list, tuple)) and not pair(order_by) \
        else [order_by]
    if not 1 <= len(items) <= MAX_KEYS:
        raise ValueError(f"order_by: 1 to {MAX_KEYS} order columns, not {len(items)}")
    out = []
    for it in items:
        what = it[0] if isinstance(it, tuple) and len(it) == 2 else it
        if type(what).__name__ == "JoinAttr":
            raise NotImplementedError(f"ORDER BY {what!r}: a joined attribute (dim[attr]) is not "
                                      "ordered on the GPU")
        if one(it):
            out.append((name_of(it), False))
        elif pair(it):
            out.append((name_of(it[0]), it[1] == "descending"))
        elif isinstance(it, tuple) and len(it) == 2 and one(it[0]):
            raise ValueError(f"order_by: direction {it[1]!r}: 'ascending' or 'descending'")
        else:
            raise TypeError(f"order_by: {it!r} is no column name or expression (dim[attr] and "
                            "other kinds are not ordered)")
    names = [str(n) for n, _ in out]
    for n in names:
        if names.count(n) > 1:
            raise ValueError(f"order_by: {n!r} appears twice")
    return out


def window(n: int, limit: Optional[int], offset: int) -> Tuple[int, int]:
    """(first, count) of LIMIT / OFFSET over n sorted rows."""
    for v, what in ((limit, "limit"), (offset, "offset")):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0):
            raise ValueError(f"{what}={v!r}: a non-negative int")
    first = min(int(offset), n)
    return first, n - first if limit is None else min(int(limit), n - first)


# ------------------------------------------------------------ numpy twin
def host_order(columns: Sequence[tuple], n: int) -> np.ndarray:
    """The permutation (int64) that sorts n rows by ``columns``, the most
    significant first: each (values, valid bool/uint8 array or None,
    descending)."""
    keys = []
    for values, valid, desc in reversed(list(columns)):
        key, cls, _ = T.encode(np.asarray(values)[:n],
                               None if valid is None else np.asarray(valid)[:n] != 0, bool(desc))
        keys += [key, cls]
    if not keys:
        return np.arange(n, dtype=np.int64)
    return np.lexsort(tuple(keys)).astype(np.int64)


def host_apply(perm: np.ndarray, first: int, count: int, values, valid=None, offsets=None):
    """(values, valid, offsets) of one column in the order ``perm[first :
    first + count]``: ``values`` per row ((n, 2) for decimal128), or with
    ``offsets`` (int64[n + 1]) a string column's characters."""
    idx = np.asarray(perm, np.int64)[first:first + count]
    ok = None if valid is None else np.asarray(valid)[idx]
    if offsets is None:
        return np.asarray(values)[idx], ok, None
    offs = np.asarray(offsets, np.int64)
    a = offs[idx]
    ln = offs[idx + 1] - a if len(idx) else a
    st = np.cumsum(ln) - ln
    src = np.repeat(a - st, ln) + np.arange(int(ln.sum()))
    return np.asarray(values, np.uint8)[src], ok, \
        np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)


# ------------------------------------------------------------ native host copy
def type_code(dtype) -> int:
    dt = np.dtype(dtype)
    return TYPE_CODE["i8" if dt.kind in "mM" else f"{dt.kind}{dt.itemsize}"]


def passes(code: int, classes: bool) -> int:
    """Radix passes of one order column."""
    return _WIDTH[code] + (1 if classes or code in _FLOAT else 0)


def native_host_order(columns: Sequence[tuple], n: int) -> np.ndarray:
    """host_order through the library's CPU copies of the kernels' steps
    (strom_sort_encode_host / strom_sort_pass_host), with the device's
    schedule of passes."""
    from .. import _native as N
    L = N.lib()
    key = [np.zeros(max(n, 1), np.uint64) for _ in range(2)]
    perm = [np.zeros(max(n, 1), np.uint32) for _ in range(2)]
    work = np.zeros(int(L.strom_sort_work_bytes(n)) // 4, np.uint32)
    cur, first = 0, FIRST

    def run(code, flags, v, ok, shifts):
        nonlocal cur
        rc = L.strom_sort_encode_host(code, flags, v.ctypes.data, ok.ctypes.data if ok is not None
                                      else 0, perm[cur].ctypes.data, n, key[cur].ctypes.data)
        for sh in shifts:
            rc = rc or L.strom_sort_pass_host(key[cur].ctypes.data, perm[cur].ctypes.data,
                                              key[1 - cur].ctypes.data, perm[1 - cur].ctypes.data,
                                              n, sh, work.ctypes.data)
            cur = 1 - cur
        if rc:
            raise RuntimeError(f"sort host copy failed (rc={rc})")
    for values, valid, desc in reversed(list(columns)):
        v = np.ascontiguousarray(np.asarray(values)[:n])
        if v.dtype.kind in "mM":
            v = v.view(np.int64)
        if not n:
            v = np.zeros(1, v.dtype)
        ok = None if valid is None else np.ascontiguousarray(np.asarray(valid)[:n] != 0, np.uint8)
        code = type_code(v.dtype)
        run(code, first | (DESC if desc else 0), v, ok, range(0, 8 * _WIDTH[code], 8))
        first = 0
        if ok is not None or code in _FLOAT:
            run(code, CLASS, v, ok, [0])
    if first:
        return np.arange(n, dtype=np.int64)
    return perm[cur][:n].astype(np.int64)


def sort_cols(specs: Sequence[tuple]) -> np.ndarray:
    """The descriptor array of a gather: per column (kind, width, in, out,
    in_valid, out_valid) as addresses (0: none)."""
    if len(specs) > MAX_COLS:
        raise ValueError(f"a gather takes at most {MAX_COLS} columns")
    a = np.zeros(len(specs), SORT_COL)
    for i, (kind, width, src, out, in_valid, out_valid) in enumerate(specs):
        if kind not in (FIXED, LEN) or (kind == FIXED and width not in WIDTHS):
            raise ValueError(f"column {i}: kind {kind} width {width}")
        a[i] = (kind, width, src, out, in_valid or 0, out_valid or 0)
    return a


# ------------------------------------------------------------ device
def work_bytes(n: int) -> int:
    from .. import _native as N
    return int(N.lib().strom_sort_work_bytes(n))


class State:
    """The sort's device memory for n rows: ``key`` and ``perm`` (two each,
    int64 / int32 tensors holding the uint64 keys and uint32 permutation
    entries), ``work`` the table, ``cur`` which pair holds the current order,
    ``err`` the gather's uint64 error word."""

    def __init__(self, n: int, device):
        import torch
        if not 0 <= n < 1 << 32:
            raise ValueError(f"n={n}: the permutation entries are 32 bits")
        self.n = int(n)
        m = max(self.n, 1)
        self.key = [torch.empty(m, dtype=torch.int64, device=device) for _ in range(2)]
        self.perm = [torch.empty(m, dtype=torch.int32, device=device) for _ in range(2)]
        self.work = torch.empty(work_bytes(self.n) // 4, dtype=torch.int32, device=device)
        self.err = torch.zeros(1, dtype=torch.int64, device=device)
        self.cur = 0
        self.fresh = True                       # no column yet: perm is not written

    @property
    def order(self):
        """The current permutation (int32 tensor of uint32 entries)."""
        return self.perm[self.cur][:self.n]


def encode(st: State, code: int, values, valid, descending: bool = False, classes: bool = False,
           stream=None) -> None:
    """strom_sort_encode into the current key array through the current
    permutation (the first call of a state writes the identity)."""
    from ._util import check, lib, ptr, require_cuda, stream_handle
    require_cuda(values, "values")
    if code not in _WIDTH:
        raise NotImplementedError(f"order by storage type {code}: integers and float32/64")
    if values.numel() * values.element_size() < st.n * _WIDTH[code] or \
            (valid is not None and valid.numel() < st.n):
        raise ValueError("values / valid: one entry per row")
    flags = (DESC if descending else 0) | (CLASS if classes else 0) | (FIRST if st.fresh else 0)
    check(lib().strom_sort_encode(code, flags, ptr(values), ptr(valid) if valid is not None else 0,
                                  ptr(st.perm[st.cur]), st.n, ptr(st.key[st.cur]),
                                  stream_handle(stream)), "sort_encode")
    st.fresh = False


def radix_pass(st: State, shift: int, stream=None) -> None:
    """strom_sort_pass: the current pair into the other one, which becomes
    the current."""
    from ._util import check, lib, ptr, stream_handle
    a, b = st.cur, 1 - st.cur
    check(lib().strom_sort_pass(ptr(st.key[a]), ptr(st.perm[a]), ptr(st.key[b]), ptr(st.perm[b]),
                                st.n, shift, ptr(st.work), stream_handle(stream)), "sort_pass")
    st.cur = b


def order(st: State, columns: Sequence[tuple], stream=None) -> int:
    """Sort the state's rows by ``columns``, the most significant first: each
    (STROM_COL_* code, values tensor, valid uint8 tensor or None,
    descending).  Returns the number of radix passes enqueued."""
    done = 0
    for code, values, valid, desc in reversed(list(columns)):
        encode(st, code, values, valid, desc, stream=stream)
        for sh in range(0, 8 * _WIDTH[code], 8):
            radix_pass(st, sh, stream)
        done += _WIDTH[code]
        if valid is not None or code in _FLOAT:
            encode(st, code, values, valid, classes=True, stream=stream)
            radix_pass(st, 0, stream)
            done += 1
    return done


def apply(perm, n: int, first: int, count: int, rows_in, rows_out, cols: np.ndarray, err,
          stream=None) -> None:
    """strom_sort_apply: the row ids and ``cols`` (``sort_cols`` of device
    addresses) in the order perm[first : first + count]."""
    from ._util import check, lib, ptr, stream_handle
    check(lib().strom_sort_apply(ptr(perm), n, first, count,
                                 ptr(rows_in) if rows_in is not None else 0,
                                 ptr(rows_out) if rows_out is not None else 0,
                                 cols.ctypes.data if len(cols) else 0, len(cols), ptr(err),
                                 stream_handle(stream)), "sort_apply")


def chars(perm, n: int, first: int, count: int, in_off, in_chars, in_len: int, out_off,
          out_chars, stream=None) -> None:
    """strom_sort_chars: a string column's characters in output order."""
    from ._util import check, lib, ptr, stream_handle
    check(lib().strom_sort_chars(ptr(perm), n, first, count, ptr(in_off), ptr(in_chars), in_len,
                                 ptr(out_off), ptr(out_chars), out_chars.numel(),
                                 stream_handle(stream)), "sort_chars")
