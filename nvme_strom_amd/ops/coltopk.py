"""ORDER BY one column LIMIT k over a scan's selection bitmap
(csrc/kernels/coltopk.hip): the device select and merge, the key encoding,
and a numpy twin with the same slabs and the same state.

The order is (class, key, row), all ascending: class 0 a value, 1 a NaN, 2
a null, in both directions; ``key`` the order-preserving 64-bit key of the
value (colagg's MIN / MAX encoding, -0.0 taken as +0.0), every bit inverted
for a descending query, 0 for a NaN or a null; ``row`` the file-global row
id.  It is total, so every result is unique and the kernels are compared
with the twin word for word.

A candidate is three uint64 words (strom.h): key, ``meta = class << 62 |
row << 2 | negzero << 1 | pvalid`` and the payload (the carried column's
value, zero-extended; 0 when null or absent).  A state is ``HDR_WORDS``
header words (K, COUNT, SEEN, THRESH, ERRORS, MERGES) and up to k sorted
candidates; a slab is (n, rows seen) and up to k sorted candidates, one slab
per workgroup of the select launch: workgroup g of ``grid(nwords, k)`` walks
the bitmap words 4 g + 4 grid t + (0 .. 3).

The threshold: once a state holds k candidates and the k-th is a value, its
key is THRESH; a select launch reads it once and drops rows behind it.  The
result does not depend on it — a select that read an older, larger THRESH
only leaves more candidates in its slabs.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

MAX_K = 6144
HDR_WORDS = 8
ENTRY_WORDS = 3
SLAB_HDR_WORDS = 2
H_K, H_COUNT, H_SEEN, H_THRESH, H_ERRORS, H_MERGES = range(6)
DESC = 1
PASS = np.uint64(0xFFFFFFFFFFFFFFFF)
# STROM_COL_* of the storage types an order column may have
TYPE_CODE = {"i4": 1, "i8": 2, "f4": 3, "f8": 4, "i1": 5, "i2": 6, "u1": 7, "u2": 8, "u4": 9,
             "u8": 10}
_SIGN = np.uint64(1 << 63)
_ROW_MASK = np.uint64((1 << 60) - 1)
_MIN_WORDS, _MAX_GRID, _SLAB_ENTRIES = 16, 1024, 1 << 18


def check_k(k) -> int:
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= MAX_K:
        raise ValueError(f"k={k!r}: 1 <= k <= {MAX_K} (STROM_TOPK_MAX_K)")
    return int(k)


def state_words(k: int) -> int:
    return HDR_WORDS + ENTRY_WORDS * k


def slab_words(k: int) -> int:
    return SLAB_HDR_WORDS + ENTRY_WORDS * k


def grid(nwords: int, k: int) -> int:
    """Workgroups (slabs) of a select launch: strom_column_topk_grid."""
    if not nwords or not k:
        return 0
    most = max(1, min(_MAX_GRID, _SLAB_ENTRIES // k))
    return min(most, (nwords + _MIN_WORDS - 1) // _MIN_WORDS)


# ------------------------------------------------------------ key encoding
def encode(values, valid=None, descending: bool = False) -> Tuple[np.ndarray, np.ndarray,
                                                                   np.ndarray]:
    """(key, class, negzero) per value, uint64 each.  ``values``: integers,
    floats, or datetime64 / timedelta64 (their ticks); ``valid`` a bool
    array or None."""
    v = np.asarray(values)
    if v.dtype.kind in "mM":
        v = v.view(np.int64)
    n = len(v)
    cls = np.zeros(n, np.uint64)
    negz = np.zeros(n, np.uint64)
    if v.dtype.kind == "f" and v.dtype.itemsize in (4, 8):
        d = v.astype(np.float64)
        bits = d.view(np.uint64).copy()
        zero = d == 0
        negz[zero & ((bits >> np.uint64(63)) == 1)] = 1
        bits[zero] = 0
        key = np.where(bits & _SIGN != 0, ~bits, bits | _SIGN)
        cls[np.isnan(d)] = 1
    elif v.dtype.kind == "i":
        key = v.astype(np.int64).view(np.uint64) ^ _SIGN
    elif v.dtype.kind == "u":
        key = v.astype(np.uint64)
    else:
        raise NotImplementedError(f"order key of dtype {v.dtype}: integers and float32/64")
    if descending:
        key = ~key
    if valid is not None:
        cls[~np.asarray(valid, bool)] = 2
    off = cls != 0
    key[off] = 0
    negz[off] = 0
    return key, cls, negz


def entries(values, valid, rows, descending: bool = False, pay=None, pay_valid=None) -> np.ndarray:
    """The candidates (n, 3) uint64 of ``values`` at the file-global ids
    ``rows``; ``pay`` the carried column's values (any fixed-width dtype of
    up to 8 bytes) with ``pay_valid`` (None: no nulls)."""
    key, cls, negz = encode(values, valid, descending)
    n = len(key)
    out = np.zeros((n, ENTRY_WORDS), np.uint64)
    pv = np.zeros(n, np.uint64)
    if pay is not None:
        p = np.ascontiguousarray(pay)
        width = p.dtype.itemsize
        p = p.view(f"u{width}").astype(np.uint64)
        pv[:] = 1
        if pay_valid is not None:
            pv[~np.asarray(pay_valid, bool)] = 0
        out[:, 2] = np.where(pv == 1, p, 0)
    out[:, 0] = key
    out[:, 1] = cls << np.uint64(62) | np.asarray(rows).astype(np.uint64) << np.uint64(2) | \
        negz << np.uint64(1) | pv
    return out


def order(ent: np.ndarray) -> np.ndarray:
    """The permutation that sorts candidates: lexsort on (class, key, meta)."""
    return np.lexsort((ent[:, 1], ent[:, 0], ent[:, 1] >> np.uint64(62)))


def best(ent: np.ndarray, k: int) -> np.ndarray:
    """The k first candidates, sorted."""
    return ent[order(ent)[:k]]


def decode(ent: np.ndarray, dtype, descending: bool = False):
    """(rows int64, values of ``dtype``, valid bool, payload words uint64,
    payload valid bool) of candidates."""
    ent = np.asarray(ent, np.uint64).reshape(-1, ENTRY_WORDS)
    dt = np.dtype(dtype)
    key, meta = ent[:, 0].copy(), ent[:, 1]
    cls = meta >> np.uint64(62)
    rows = ((meta >> np.uint64(2)) & _ROW_MASK).astype(np.int64)
    if descending:
        key = ~key
    if dt.kind == "f":
        bits = np.where(key & _SIGN != 0, key ^ _SIGN, ~key)
        d = bits.view(np.float64).copy()
        d[(meta >> np.uint64(1)) & np.uint64(1) == 1] = -0.0
        d[cls == 1] = np.nan
        d[cls == 2] = 0
        vals = d.astype(dt)
    elif dt.kind == "i":
        vals = (key ^ _SIGN).view(np.int64)
        vals = np.where(cls == 0, vals, 0).astype(dt)
    else:
        vals = np.where(cls == 0, key, 0).astype(dt)
    return rows, vals, cls != 2, ent[:, 2].copy(), (meta & np.uint64(1)) == 1


def payload_as(words: np.ndarray, dtype) -> np.ndarray:
    """The payload words back in the carried column's dtype."""
    dt = np.dtype(dtype)
    return np.asarray(words, np.uint64).astype(f"u{dt.itemsize}").view(dt)


# ------------------------------------------------------------ numpy twin
def host_init(k: int) -> np.ndarray:
    """strom_topk_init: an empty state."""
    st = np.zeros(state_words(check_k(k)), np.uint64)
    st[H_K], st[H_THRESH] = k, PASS
    return st


def state_entries(state: np.ndarray) -> np.ndarray:
    n = int(state[H_COUNT])
    return np.asarray(state[HDR_WORDS:HDR_WORDS + ENTRY_WORDS * n]).reshape(n, ENTRY_WORDS)


def host_select(batches: Sequence[tuple], src, k: int, descending: bool = False,
                state: Optional[np.ndarray] = None, pay: Optional[Sequence[tuple]] = None,
                out: Optional[np.ndarray] = None) -> np.ndarray:
    """What strom_column_topk leaves: ``batches`` a list of (values, valid
    bool or None, row_base), batch b on fresh bitmap words; ``src`` the
    selection words (bits beyond a batch's rows are ignored); ``pay`` per
    batch (values, valid or None) of the carried column.  Returns the slabs
    (grid, slab_words) uint64, written into ``out`` when given (the words a
    launch does not write stay)."""
    src = np.asarray(src).view(np.uint64)
    thresh = PASS if state is None else np.uint64(state[H_THRESH])
    g = grid(len(src), k)
    slabs = np.zeros((g, slab_words(k)), np.uint64) if out is None else \
        np.asarray(out).view(np.uint64).reshape(g, slab_words(k))
    ents, wgs = [], []
    w0 = 0
    for b, (v, ok, row_base) in enumerate(batches):
        n = len(v)
        nw = (n + 63) // 64
        sel = np.flatnonzero(np.unpackbits(src[w0:w0 + nw].view(np.uint8),
                                           bitorder="little")[:n])
        pv = pok = None
        if pay is not None:
            pv = np.asarray(pay[b][0])[sel]
            pok = None if pay[b][1] is None else np.asarray(pay[b][1], bool)[sel]
        ents.append(entries(np.asarray(v)[sel], None if ok is None else np.asarray(ok, bool)[sel],
                            sel + int(row_base), descending, pv, pok))
        wgs.append(((w0 + sel // 64) // 4) % max(g, 1))
        w0 += nw
    ent = np.concatenate(ents) if ents else np.zeros((0, ENTRY_WORDS), np.uint64)
    wg = np.concatenate(wgs) if wgs else np.zeros(0, np.int64)
    ok = (thresh == PASS) | ((ent[:, 1] >> np.uint64(62) == 0) & (ent[:, 0] <= thresh))
    for i in range(g):
        mine = wg == i
        top = best(ent[mine & ok], k)
        slabs[i, 0], slabs[i, 1] = len(top), int(mine.sum())
        slabs[i, SLAB_HDR_WORDS:SLAB_HDR_WORDS + ENTRY_WORDS * len(top)] = top.reshape(-1)
    return slabs


def host_merge(state: np.ndarray, slabs, k: int) -> np.ndarray:
    """strom_topk_merge: the slabs and the state folded into a new state."""
    st = np.asarray(state, np.uint64).copy()
    slabs = np.asarray(slabs).view(np.uint64).reshape(-1, slab_words(k))
    if not len(slabs):
        return st
    if int(st[H_K]) != k or int(st[H_COUNT]) > k:
        st[H_ERRORS] += np.uint64(1)
        return st
    parts = [state_entries(st)]
    for s in slabs:
        n = int(s[0])
        if n > k:
            st[H_ERRORS] += np.uint64(1)
            continue
        st[H_SEEN] += s[1]
        e = s[SLAB_HDR_WORDS:SLAB_HDR_WORDS + ENTRY_WORDS * n].reshape(n, ENTRY_WORDS)
        parts.append(e[e[:, 1] >> np.uint64(62) < 3])
    top = best(np.concatenate(parts), k)
    st[HDR_WORDS:HDR_WORDS + top.size] = top.reshape(-1)
    st[H_COUNT] = len(top)
    st[H_MERGES] += np.uint64(1)
    if len(top) == k:
        st[H_THRESH] = top[-1, 0] if top[-1, 1] >> np.uint64(62) == 0 else PASS
    return st


# ------------------------------------------------------------ native host copy
def _batch_table(batches: Sequence[tuple], keep: list, width: Optional[int] = None) -> np.ndarray:
    """A strom_filter_batch table over host arrays (kept alive in ``keep``)."""
    tab = np.zeros((len(batches), 5), np.int64)
    wb = 0
    for b, bt in enumerate(batches):
        v, ok = np.ascontiguousarray(bt[0]), bt[1]
        if v.dtype.kind in "mM":
            v = v.view(np.int64)
        n = len(v)
        nw = (n + 63) // 64
        # one element at least, so that an empty batch has an address too
        data = np.zeros(max(n, 1), v.dtype)
        data[:n] = v
        keep.append(data)
        vptr = 0
        if ok is not None:
            bits = np.zeros(max(nw, 1) * 64, np.uint8)
            bits[:n] = np.asarray(ok, bool)
            vb = np.packbits(bits, bitorder="little")
            keep.append(vb)
            vptr = vb.ctypes.data
        tab[b] = (data.ctypes.data, vptr, n, wb, bt[2] if len(bt) > 2 else 0)
        wb += nw
    return tab


def native_host_select(batches: Sequence[tuple], src, k: int, descending: bool = False,
                       state: Optional[np.ndarray] = None, pay: Optional[Sequence[tuple]] = None,
                       out: Optional[np.ndarray] = None) -> np.ndarray:
    """host_select through the library's CPU copy of the kernel's phases
    (strom_topk_host_select): the arguments of host_select."""
    from .. import _native as N
    src = np.ascontiguousarray(np.asarray(src).view(np.uint64))
    st = host_init(k) if state is None else np.ascontiguousarray(state, np.uint64)
    keep: list = []
    dt = np.asarray(batches[0][0]).dtype
    code = TYPE_CODE["i8" if dt.kind in "mM" else f"{dt.kind}{dt.itemsize}"]
    tab = _batch_table(batches, keep)
    ptab, width = None, 0
    if pay is not None:
        ptab = _batch_table([(p[0], p[1], 0) for p in pay], keep)
        width = np.asarray(pay[0][0]).dtype.itemsize
    g = grid(len(src), k)
    slabs = np.zeros((g, slab_words(k)), np.uint64) if out is None else \
        np.asarray(out).view(np.uint64).reshape(g, slab_words(k))
    rc = N.lib().strom_topk_host_select(code, DESC if descending else 0, k, src.ctypes.data,
                                        len(src), tab.ctypes.data,
                                        ptab.ctypes.data if ptab is not None else 0, width,
                                        len(batches), st.ctypes.data,
                                        slabs.ctypes.data if g else st.ctypes.data)
    if rc:
        raise RuntimeError(f"topk_host_select failed (rc={rc})")
    return slabs


def native_host_merge(state: np.ndarray, slabs, k: int) -> np.ndarray:
    """host_merge through the library's CPU copy (strom_topk_host_merge)."""
    from .. import _native as N
    st = np.ascontiguousarray(state, np.uint64).copy()
    slabs = np.ascontiguousarray(np.asarray(slabs).view(np.uint64)).reshape(-1, slab_words(k))
    rc = N.lib().strom_topk_host_merge(k, slabs.ctypes.data if len(slabs) else 0, len(slabs),
                                       st.ctypes.data)
    if rc:
        raise RuntimeError(f"topk_host_merge failed (rc={rc})")
    return st


# ------------------------------------------------------------ device
class State:
    """A top-k state on the device: ``words`` the int64 tensor of header and
    candidates."""

    def __init__(self, words, k: int):
        self.words, self.k = words, int(k)

    def to_host(self) -> np.ndarray:
        """The state's words on the host (synchronizes)."""
        return self.words.cpu().numpy().view(np.uint64).copy()


def init(k: int, device, stream=None, words=None) -> State:
    """strom_topk_init: a new empty state on ``device`` (in ``words``, an
    int64 tensor of state_words(k), when given)."""
    import torch
    from ._util import check, lib, ptr, require_cuda, stream_handle
    k = check_k(k)
    if words is None:
        words = torch.empty(state_words(k), dtype=torch.int64, device=device)
    else:
        require_cuda(words, "words")
        if words.dtype != torch.int64 or words.numel() != state_words(k):
            raise ValueError("words: int64, state_words(k)")
    check(lib().strom_topk_init(ptr(words), k, stream_handle(stream)), "topk_init")
    return State(words, k)


def select(state: State, code: int, vals, nwords: int, bitmap, descending: bool = False,
           pay=None, pay_width: int = 0, slabs=None, stream=None):
    """strom_column_topk over a group: ``vals`` the (nbatches, 5)
    strom_filter_batch table of the order column, ``pay`` that of the
    carried column (``pay_width`` bytes per row) or None.  Returns (slabs
    int64 tensor, how many): ``slabs`` is allocated unless given."""
    import torch
    from ._util import check, lib, ptr, require_cuda, stream_handle
    from .colfilter import BATCH_FIELDS
    for t, name in ((vals, "vals"), (bitmap, "bitmap")) + (((pay, "pay"),) if pay is not None
                                                          else ()):
        require_cuda(t, name)
    if vals.dtype != torch.int64 or vals.dim() != 2 or vals.shape[1] != BATCH_FIELDS:
        raise ValueError("vals: int64 (n, 5)")
    if pay is not None and (pay.shape != vals.shape or pay.dtype != torch.int64):
        raise ValueError("pay: a table of the same batches")
    if (pay_width not in (1, 2, 4, 8)) if pay is not None else pay_width:
        raise ValueError("pay_width: 1, 2, 4 or 8 bytes with pay, else 0")
    if bitmap.numel() < nwords:
        raise ValueError("bitmap too small")
    if code not in TYPE_CODE.values():
        raise NotImplementedError(f"order by storage type {code}: integers and float32/64")
    n = grid(nwords if vals.shape[0] else 0, state.k)
    need = n * slab_words(state.k)
    if slabs is None:
        slabs = torch.empty(max(need, 1), dtype=torch.int64, device=bitmap.device)
    elif slabs.numel() < need or slabs.dtype != torch.int64:
        raise ValueError("slabs: int64, grid * slab_words")
    if n:
        check(lib().strom_column_topk(code, DESC if descending else 0, state.k, ptr(bitmap), nwords,
                                      ptr(vals), ptr(pay) if pay is not None else 0, pay_width,
                                      vals.shape[0], ptr(state.words), ptr(slabs),
                                      stream_handle(stream)), "column_topk")
    return slabs, n


def merge(state: State, slabs, nslabs: int, stream=None) -> None:
    """strom_topk_merge: fold ``nslabs`` slabs into the state."""
    from ._util import check, lib, ptr, stream_handle
    if not nslabs:
        return
    if slabs.numel() < nslabs * slab_words(state.k):
        raise ValueError("slabs too small")
    check(lib().strom_topk_merge(state.k, ptr(slabs), nslabs, ptr(state.words),
                                 stream_handle(stream)), "topk_merge")
