"""Aggregates over a scan's selection bitmap (csrc/kernels/colagg.hip):
COUNT / SUM / MIN / MAX of the selected valid rows of a column, per key slot
when a small-domain key column is given — and a numpy twin of the kernels.

The accumulator block is an array of 64-bit words, the same on the device
and in the twin: word 0 counts malformed keys, then one *entry* per
aggregated column, each ``popcount(ops)`` arrays of ``nslots`` words in the
order COUNT, SUM, MIN, MAX (strom.h).  SUM holds the bits of an int64 /
uint64 (wrapping, like ``pyarrow.compute.sum``) or of a float64 (float32
included); MIN / MAX hold order-preserving keys that NaN never enters.
``entry_arrays`` turns an entry back into typed numpy arrays.

Semantics (pinned to pyarrow.compute): nulls of the aggregated column are
skipped; NaN propagates into a float sum; min / max ignore NaN and are NaN
only when every counted value is; a slot that counted nothing has no sum,
min or max.  Slot ``nslots - 1`` of a keyed block collects the null keys.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

COUNT, SUM, MIN, MAX, ALL = 1, 2, 4, 8, 16
COL_NONE = 0
COL_BOOL = 11
# a launch keeps popcount(ops) * nslots 8-byte accumulators in LDS
# (STROM_AGG_LDS_BYTES); larger integer key domains go through the hash table
# and HBM accumulators of ops/colgroup.py
LDS_BYTES = 64 << 10
_SIGN = np.uint64(1 << 63)
_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
# STROM_COL_* of the storage types whose values the kernels read
VALUE_CODE = {"i4": 1, "i8": 2, "f4": 3, "f8": 4, "i1": 5, "i2": 6, "u1": 7, "u2": 8, "u4": 9,
              "u8": 10}


def nacc(ops: int) -> int:
    return bin(ops & 15).count("1")


def max_slots(ops: int) -> int:
    """Key slots (the null slot included) one launch with ``ops`` can hold."""
    return LDS_BYTES // (8 * max(1, nacc(ops)))


@dataclass
class Entry:
    """One aggregated column: ``dtype`` is its storage dtype ("i8", "f4", ...;
    None with COL_NONE: only validity is read, or nothing with ALL)."""
    ops: int
    dtype: Optional[str] = None
    name: Optional[str] = None

    @property
    def code(self) -> int:
        return VALUE_CODE[self.dtype] if self.dtype is not None else COL_NONE

    @property
    def is_float(self) -> bool:
        return self.dtype in ("f4", "f8")


class Layout:
    """Where each entry lives in the block; refuses what the kernel's LDS
    cannot hold."""

    def __init__(self, entries: Sequence[Entry], nslots: int = 1, key_code: int = 0):
        self.entries = list(entries)
        self.nslots = int(nslots)
        self.key_code = int(key_code)
        self.off: List[int] = []
        o = 1
        for e in self.entries:
            if not nacc(e.ops):
                raise ValueError("an entry needs COUNT, SUM, MIN or MAX")
            if e.dtype is None and e.ops & (SUM | MIN | MAX):
                raise ValueError("SUM / MIN / MAX need a value type")
            if nacc(e.ops) * self.nslots * 8 > LDS_BYTES:
                raise NotImplementedError(
                    f"{self.nslots} key slots x {nacc(e.ops)} accumulators exceed the kernel's "
                    f"{LDS_BYTES >> 10} KiB of LDS (at most {max_slots(e.ops)} slots, the null "
                    "slot included); larger key domains are not aggregated on the GPU")
            self.off.append(o)
            o += nacc(e.ops) * self.nslots
        self.words = o

    def pos(self, e: int, op: int) -> Optional[slice]:
        """Words of accumulator ``op`` of entry ``e`` (None: not requested)."""
        ent = self.entries[e]
        if not ent.ops & op:
            return None
        j = bin(ent.ops & (op - 1) & 15).count("1")
        a = self.off[e] + j * self.nslots
        return slice(a, a + self.nslots)


# ------------------------------------------------------------ numpy twin
def new_block(layout: Layout) -> np.ndarray:
    """A host block at its identities (what strom_column_agg_init writes)."""
    b = np.zeros(layout.words, np.uint64)
    for e in range(len(layout.entries)):
        s = layout.pos(e, MIN)
        if s is not None:
            b[s] = _ONES
    return b


def order_keys(x: np.ndarray) -> np.ndarray:
    """The kernels' order-preserving uint64 keys of values (floats as
    float64: sign bit set for x >= 0, all bits flipped for x < 0)."""
    x = np.asarray(x)
    if x.dtype.kind == "f":
        b = x.astype(np.float64).view(np.uint64)
        return np.where(b & _SIGN != 0, ~b, b | _SIGN)
    if x.dtype.kind == "u":
        return x.astype(np.uint64)
    return x.astype(np.int64).view(np.uint64) ^ _SIGN


def key_values(keys: np.ndarray, dtype: str) -> np.ndarray:
    """Inverse of order_keys, in the storage dtype."""
    keys = np.asarray(keys, np.uint64)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        b = np.where(keys & _SIGN != 0, keys & ~_SIGN, ~keys)
        return b.view(np.float64).astype(dt)
    if dt.kind == "u":
        return keys.astype(dt)
    return (keys ^ _SIGN).view(np.int64).astype(dt)


def key_slots(key_values_, key_valid, nslots: int):
    """(slot per row, bad-key mask): the slot is the key value (a dictionary
    index, a bool, the byte of an int8 / uint8 key), ``nslots - 1`` for a
    null key; a value outside [0, nslots - 1) is malformed."""
    k = np.asarray(key_values_)
    k = k.astype(np.int64) if k.dtype != np.uint64 else \
        np.where(k > np.uint64(1 << 62), -1, k.astype(np.int64))
    null = np.zeros(len(k), bool) if key_valid is None else ~np.asarray(key_valid, bool)
    bad = ~null & ((k < 0) | (k >= nslots - 1))
    return np.where(null, nslots - 1, np.where(bad, 0, k)), bad


def host_agg(layout: Layout, block: np.ndarray, e: int, sel: np.ndarray, values=None, valid=None,
             key=None, count_bad: bool = True) -> None:
    """The kernels' result of one launch for entry ``e`` folded into
    ``block``: ``sel`` the selected rows (bool), ``values`` / ``valid`` the
    aggregated column's rows, ``key`` = (values, valid) of the key column."""
    ent = layout.entries[e]
    sel = np.asarray(sel, bool)
    n = len(sel)
    if key is not None:
        slots, bad = key_slots(key[0][:n], None if key[1] is None else key[1][:n], layout.nslots)
        if count_bad:
            block[0] += np.uint64(int((sel & bad).sum()))
        sel = sel & ~bad
    else:
        slots = np.zeros(n, np.int64)
    use = sel if (ent.ops & ALL or valid is None) else sel & np.asarray(valid[:n], bool)
    idx = np.flatnonzero(use)
    sl = slots[idx]
    G = layout.nslots
    s = layout.pos(e, COUNT)
    if s is not None:
        block[s] += np.bincount(sl, minlength=G).astype(np.uint64)
    if ent.dtype is None:
        return
    x = np.asarray(values)[:n][idx]
    s = layout.pos(e, SUM)
    if s is not None:
        if ent.is_float:
            acc = block[s].view(np.float64)
            np.add.at(acc, sl, x.astype(np.float64))
            block[s] = acc.view(np.uint64)
        else:
            w = x.astype(np.uint64) if x.dtype.kind == "u" else x.astype(np.int64).view(np.uint64)
            acc = block[s].copy()
            np.add.at(acc, sl, w)                       # wraps, as the device's 64-bit add
            block[s] = acc
    keep = ~np.isnan(x) if ent.is_float else np.ones(len(x), bool)
    k = order_keys(x[keep])
    for op, fn in ((MIN, np.minimum), (MAX, np.maximum)):
        s = layout.pos(e, op)
        if s is not None:
            acc = block[s].copy()
            fn.at(acc, sl[keep], k)
            block[s] = acc


def merge_blocks(layout: Layout, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Two blocks of the same layout combined: counts and sums add, min and
    max combine (what the reduce kernel does with a slab)."""
    out = a.copy()
    out[0] = a[0] + b[0]
    for e, ent in enumerate(layout.entries):
        for op in (COUNT, SUM, MIN, MAX):
            s = layout.pos(e, op)
            if s is None:
                continue
            if op == MIN:
                out[s] = np.minimum(a[s], b[s])
            elif op == MAX:
                out[s] = np.maximum(a[s], b[s])
            elif op == SUM and ent.is_float:
                out[s] = (a[s].view(np.float64) + b[s].view(np.float64)).view(np.uint64)
            else:
                out[s] = a[s] + b[s]
    return out


def entry_arrays(layout: Layout, block: np.ndarray, e: int) -> dict:
    """Entry ``e`` as typed arrays over the slots: ``count`` (int64),
    ``sum`` (int64 / uint64 / float64), ``min`` / ``max`` (the storage dtype;
    NaN where every counted value was NaN).  A slot with count 0 has no sum,
    min or max — its words hold the identities."""
    ent = layout.entries[e]
    block = np.asarray(block).view(np.uint64)
    out = {}
    s = layout.pos(e, COUNT)
    if s is not None:
        out["count"] = block[s].astype(np.int64)
    s = layout.pos(e, SUM)
    if s is not None:
        w = block[s].copy()
        out["sum"] = w.view(np.float64) if ent.is_float else \
            (w if np.dtype(ent.dtype).kind == "u" else w.view(np.int64))
    for name, op, ident in (("min", MIN, _ONES), ("max", MAX, np.uint64(0))):
        s = layout.pos(e, op)
        if s is None:
            continue
        k = block[s]
        v = key_values(k, ent.dtype)
        if ent.is_float:
            v = v.copy()
            v[k == ident] = np.nan
        out[name] = v
    return out


# ------------------------------------------------------------ device launch
def alloc_block(layout: Layout, device, stream=None, guard: int = 0):
    """The device block (int64 tensor viewing the 64-bit words), at its
    identities; ``guard`` extra words before and after it (tests).  Returns
    the tensor of the block itself."""
    import torch
    from ._util import check, lib, ptr, stream_handle
    whole = torch.zeros(layout.words + 2 * guard, dtype=torch.int64, device=device)
    block = whole[guard:guard + layout.words]
    for e, ent in enumerate(layout.entries):
        check(lib().strom_column_agg_init(ent.ops, layout.nslots,
                                          ptr(block) + 8 * layout.off[e], stream_handle(stream)),
              "column_agg_init")
    block._whole = whole
    return block


def slab_words(layout: Layout, e: int, nwords: int) -> int:
    from ._util import lib
    ent = layout.entries[e]
    return int(lib().strom_column_agg_grid(nwords, ent.ops, layout.nslots)) * nacc(ent.ops) * \
        layout.nslots


def agg_launch(layout: Layout, e: int, block, bitmap, nwords: int, vals, keys=None,
               slabs=None, count_bad: bool = True, stream=None):
    """The aggregate kernel of entry ``e`` over a group: ``vals`` / ``keys``
    are (nbatches, 5) strom_filter_batch tables of the aggregated and the key
    column (the same batches).  Writes one slab per workgroup into ``slabs``
    (allocated when None) and returns (slabs, number of slabs); malformed
    keys are counted in the block's word 0 when ``count_bad``."""
    import torch
    from ._util import check, lib, ptr, require_cuda, stream_handle
    from .colfilter import BATCH_FIELDS
    require_cuda(bitmap, "bitmap")
    require_cuda(vals, "vals")
    if vals.dtype != torch.int64 or vals.dim() != 2 or vals.shape[1] != BATCH_FIELDS:
        raise ValueError("vals: int64 (n, 5)")
    if keys is not None and (keys.shape != vals.shape or keys.dtype != torch.int64):
        raise ValueError("keys: a table of the same batches")
    if (keys is None) != (layout.nslots == 1 and not layout.key_code):
        raise ValueError("a keyed layout needs the key table (and only it)")
    if bitmap.numel() < nwords:
        raise ValueError("bitmap too small")
    ent = layout.entries[e]
    nslabs = int(lib().strom_column_agg_grid(nwords, ent.ops, layout.nslots))
    need = nslabs * nacc(ent.ops) * layout.nslots
    if slabs is None:
        slabs = torch.empty(need, dtype=torch.int64, device=bitmap.device)
    if slabs.numel() < need:
        raise ValueError("slabs too small")
    if not nwords or not vals.shape[0]:
        return slabs, 0
    check(lib().strom_column_agg(ent.code, ent.ops, ptr(bitmap), nwords, ptr(vals),
                                 ptr(keys) if keys is not None else 0, layout.key_code,
                                 layout.nslots, vals.shape[0], ptr(slabs), slabs.numel(),
                                 ptr(block) if (keys is not None and count_bad) else 0,
                                 stream_handle(stream)), "column_agg")
    return slabs, nslabs


def agg_reduce(layout: Layout, e: int, block, slabs, nslabs: int, stream=None) -> None:
    """Fold the slabs of one agg_launch into entry ``e`` of the block, in a
    fixed order."""
    from ._util import check, lib, ptr, stream_handle
    ent = layout.entries[e]
    check(lib().strom_column_agg_reduce(ent.code, ent.ops, layout.nslots, ptr(slabs), nslabs,
                                        ptr(block) + 8 * layout.off[e], stream_handle(stream)),
          "column_agg_reduce")


def agg_batched(layout: Layout, e: int, block, bitmap, nwords: int, vals, keys=None,
                count_bad: bool = True, stream=None) -> None:
    """agg_launch + agg_reduce on one stream."""
    slabs, n = agg_launch(layout, e, block, bitmap, nwords, vals, keys, None, count_bad, stream)
    agg_reduce(layout, e, block, slabs, n, stream)


def block_to_host(block) -> np.ndarray:
    return block.cpu().numpy().view(np.uint64).copy()


# -------------------------------------------- every entry of a group at once
class AggEntryArg(C.Structure):
    """struct strom_agg_entry (strom.h)."""
    _fields_ = [("type", C.c_int32), ("ops", C.c_uint32), ("vals", C.c_uint64),
                ("slabs", C.c_uint64), ("acc", C.c_uint64)]


def entry_args(layout: Layout, block):
    """The strom_agg_entry array of a layout over ``block`` (``vals`` and
    ``slabs`` are filled per group)."""
    arr = (AggEntryArg * len(layout.entries))()
    for i, ent in enumerate(layout.entries):
        arr[i].type, arr[i].ops = ent.code, ent.ops
        arr[i].acc = int(block.data_ptr()) + 8 * layout.off[i]
    return arr


def agg_many(layout: Layout, args, block, bitmap, nwords: int, keys_ptr: int, nbatches: int,
             stream=None) -> None:
    """One launch per entry over a group, in one native call: ``args`` from
    entry_args with each entry's table and slab addresses set (slab_words of
    room each); ``keys_ptr`` the key column's table or 0."""
    from ._util import check, lib, ptr, stream_handle
    check(lib().strom_column_agg_many(C.byref(args), len(args), ptr(bitmap), nwords, keys_ptr,
                                      layout.key_code, layout.nslots, nbatches,
                                      ptr(block) if keys_ptr else 0, stream_handle(stream)),
          "column_agg")


def agg_reduce_many(layout: Layout, args, nwords: int, stream=None) -> None:
    """The slabs of one agg_many folded into the block, entry by entry."""
    from ._util import check, lib, stream_handle
    check(lib().strom_column_agg_reduce_many(C.byref(args), len(args), layout.nslots, nwords,
                                             stream_handle(stream)), "column_agg_reduce")
