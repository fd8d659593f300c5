"""Hash GROUP BY on an integer key column (csrc/kernels/colgroup.hip): the
device table, the find-or-insert and accumulate launches, the compaction of
the occupied slots — and a numpy twin that maps key -> accumulators.

Device side: ``HDR_WORDS`` header words (strom.h: capacity, distinct keys,
overflowed rows, whether the key ``EMPTY`` was met) and ``capacity`` key
words, then per entry ``popcount(ops)`` accumulator arrays of
``capacity + 2`` words indexed by *code*: a slot index, ``capacity`` for the
null keys, ``capacity + 1`` for the one key whose bit pattern is the free
slot's.  Which slot a key gets depends on which CAS wins, so a device table
and the twin agree key by key — never slot by slot.

Both sides end in a ``Groups``: the keys ascending by value (int64, or
uint64 for an unsigned column) and a colagg block (ops/colagg.py: the same
words, the same encodings) of ``len(keys) + 1`` slots, the last one the null
keys' group.  ``merge`` unites two of them by key.

Semantics are colagg's; float sums are added with global atomics on the
device, in the order the rows arrive: they are not bitwise reproducible from
run to run (the LDS path's keyed float sums are not either).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Sequence

import numpy as np

from . import colagg as A
from .coljoin import EMPTY, FK_CODE, hash64  # noqa: F401  (the table's hash)

HDR_WORDS = 8
H_CAPACITY, H_NKEYS, H_OVERFLOW, H_HAS_EMPTY = range(4)
MAX_GROUPS = 1 << 24
KEY_CODE = FK_CODE                        # the integer storage types, as the join's
# in a word of mixed codes, reduce the rows that share the first row's code
# before the atomics (profiles/r9/hashagg/SUMMARY.md)
COMBINE = 1


def capacity(groups: int) -> int:
    """Slots of a table for ``groups`` distinct keys: a power of two >= 2 * groups."""
    c = 2
    while c < 2 * int(groups):
        c <<= 1
    return c


def check_groups(groups) -> int:
    g = int(groups)
    if not 1 <= g <= MAX_GROUPS:
        raise ValueError(f"groups={groups}: 1 <= groups <= {MAX_GROUPS}")
    return g


class GroupLayout(A.Layout):
    """colagg's block layout for any number of slots (a host block or the
    compacted device result: nothing of it lives in LDS)."""

    def __init__(self, entries: Sequence[A.Entry], nslots: int):
        self.entries = list(entries)
        self.nslots = int(nslots)
        self.key_code = 1
        self.off: List[int] = []
        o = 1
        for e in self.entries:
            if not A.nacc(e.ops):
                raise ValueError("an entry needs COUNT, SUM, MIN or MAX")
            if e.dtype is None and e.ops & (A.SUM | A.MIN | A.MAX):
                raise ValueError("SUM / MIN / MAX need a value type")
            self.off.append(o)
            o += A.nacc(e.ops) * self.nslots
        self.words = o


def narrays(entries: Sequence[A.Entry]) -> int:
    return sum(A.nacc(e.ops) for e in entries)


def wide_keys(values) -> np.ndarray:
    """Key values of any integer dtype by value: int64, uint64 for unsigned."""
    v = np.asarray(values)
    if v.dtype.kind not in "iu":
        raise NotImplementedError(f"hash GROUP BY key of dtype {v.dtype}: integer columns")
    return v.astype(np.uint64 if v.dtype.kind == "u" else np.int64)


# ------------------------------------------------------------ numpy twin
@dataclass
class Groups:
    """key -> accumulators: ``keys`` ascending by value, ``block`` a colagg
    block of ``GroupLayout(entries, len(keys) + 1)`` (last slot: null keys)."""
    entries: List[A.Entry]
    keys: np.ndarray
    block: np.ndarray

    @property
    def layout(self) -> GroupLayout:
        return GroupLayout(self.entries, len(self.keys) + 1)

    def arrays(self, e: int) -> dict:
        return A.entry_arrays(self.layout, self.block, e)


def empty_groups(entries: Sequence[A.Entry], unsigned: bool = False) -> Groups:
    ents = list(entries)
    return Groups(ents, np.zeros(0, np.uint64 if unsigned else np.int64),
                  A.new_block(GroupLayout(ents, 1)))


def host_group_agg(entries: Sequence[A.Entry], sel, key_values, key_valid, cols) -> Groups:
    """One batch through the twin: ``sel`` the selected rows (bool),
    ``key_values`` / ``key_valid`` the key column, ``cols[e]`` = (values,
    valid) of entry ``e``'s column (None, None for count(*)).  The per-group
    arithmetic is ops/colagg.host_agg's."""
    ents = list(entries)
    sel = np.asarray(sel, bool)
    n = len(sel)
    k = wide_keys(np.asarray(key_values)[:n])
    ok = np.ones(n, bool) if key_valid is None else np.asarray(key_valid, bool)[:n]
    keys = np.unique(k[sel & ok])
    lay = GroupLayout(ents, len(keys) + 1)
    block = A.new_block(lay)
    slot = np.searchsorted(keys, k)
    slot = np.where(sel & ok, np.minimum(slot, max(len(keys) - 1, 0)), 0).astype(np.int64)
    for e, (v, vok) in enumerate(cols):
        A.host_agg(lay, block, e, sel, v, vok, (slot, ok), count_bad=False)
    return Groups(ents, keys, block)


def _spread(g: Groups, keys: np.ndarray) -> np.ndarray:
    """``g``'s block over the key set ``keys`` (a superset of its own)."""
    lay = GroupLayout(g.entries, len(keys) + 1)
    out = A.new_block(lay)
    at = np.concatenate([np.searchsorted(keys, g.keys), [len(keys)]]).astype(np.int64)
    src = g.layout
    for e, ent in enumerate(g.entries):
        for op in (A.COUNT, A.SUM, A.MIN, A.MAX):
            s, d = src.pos(e, op), lay.pos(e, op)
            if s is not None:
                out[d.start + at] = g.block[s]
    return out


def merge(a: Groups, b: Groups) -> Groups:
    """Two results over the same entries united by key: counts and sums add,
    min and max combine."""
    if [(e.ops, e.dtype) for e in a.entries] != [(e.ops, e.dtype) for e in b.entries] or \
            a.keys.dtype != b.keys.dtype:
        raise ValueError("merge: different entries or key types")
    keys = np.union1d(a.keys, b.keys)
    lay = GroupLayout(a.entries, len(keys) + 1)
    return Groups(a.entries, keys, A.merge_blocks(lay, _spread(a, keys), _spread(b, keys)))


# ------------------------------------------------------------ device
class DeviceGroups:
    """A table on the device: ``table`` int64[HDR_WORDS + capacity] (header,
    key words), ``acc`` int64[narrays, capacity + 2] — entry e's arrays are
    rows ``row[e] .. row[e] + popcount(ops)``."""

    def __init__(self, entries: Sequence[A.Entry], groups: int, device, unsigned: bool = False,
                 stream=None):
        import torch
        from ._util import check, lib, ptr, stream_handle
        self.entries = list(entries)
        for e in self.entries:
            if not A.nacc(e.ops):
                raise ValueError("an entry needs COUNT, SUM, MIN or MAX")
        self.groups = check_groups(groups)
        self.capacity = capacity(self.groups)
        self.unsigned = bool(unsigned)
        self.stride = self.capacity + 2
        self.row = np.concatenate([[0], np.cumsum([A.nacc(e.ops) for e in self.entries])])
        nbytes = 8 * (HDR_WORDS + self.capacity + int(self.row[-1]) * self.stride)
        try:
            self.table = torch.empty(HDR_WORDS + self.capacity, dtype=torch.int64, device=device)
            self.acc = torch.empty((int(self.row[-1]), self.stride), dtype=torch.int64,
                                   device=device)
        except RuntimeError as err:
            raise RuntimeError(f"hash GROUP BY table for groups={self.groups}: {nbytes} bytes "
                               f"({self.capacity} slots x {int(self.row[-1])} accumulator arrays) "
                               f"could not be allocated: {err}") from err
        self.args = (A.AggEntryArg * len(self.entries))()
        for i, ent in enumerate(self.entries):
            self.args[i].type, self.args[i].ops = ent.code, ent.ops
            self.args[i].acc = int(self.acc.data_ptr()) + 8 * int(self.row[i]) * self.stride
        check(lib().strom_group_init(ptr(self.table), self.capacity, C.byref(self.args),
                                     len(self.args), stream_handle(stream)), "group_init")

    def header(self) -> np.ndarray:
        """The header on the host (synchronizes)."""
        return self.table[:HDR_WORDS].cpu().numpy().view(np.uint64).copy()

    def slots(self) -> np.ndarray:
        """The key words on the host (uint64; EMPTY: free)."""
        return self.table[HDR_WORDS:].cpu().numpy().view(np.uint64).copy()


def group_codes(t: DeviceGroups, key_code: int, keys, nwords: int, src, dst, codes,
                stream=None) -> None:
    """strom_group_codes over a group: ``keys`` the (nbatches, 5)
    strom_filter_batch table of the key column, ``src`` / ``dst`` the bitmaps
    (may be the same tensor), ``codes`` a table of the same batches whose
    values point to int32 buffers."""
    import torch
    from ._util import check, lib, ptr, require_cuda, stream_handle
    from .colfilter import BATCH_FIELDS
    for x, name in ((keys, "keys"), (src, "src"), (dst, "dst"), (codes, "codes")):
        require_cuda(x, name)
    if keys.dtype != torch.int64 or keys.dim() != 2 or keys.shape[1] != BATCH_FIELDS:
        raise ValueError("keys: int64 (n, 5)")
    if codes.shape != keys.shape or codes.dtype != torch.int64:
        raise ValueError("codes: a table of the same batches")
    if src.numel() < nwords or dst.numel() < nwords:
        raise ValueError("bitmap too small")
    if key_code not in KEY_CODE.values():
        raise NotImplementedError(f"hash GROUP BY on storage type {key_code}: integer columns")
    if not nwords or not keys.shape[0]:
        return
    check(lib().strom_group_codes(key_code, ptr(t.table), t.capacity, ptr(keys), keys.shape[0],
                                  nwords, ptr(src), ptr(dst), ptr(codes), stream_handle(stream)),
          "group_codes")


def group_agg(t: DeviceGroups, e: int, bitmap, nwords: int, vals, codes, combine=None,
              stream=None) -> None:
    """strom_group_agg of entry ``e``: ``vals`` the aggregated column's batch
    table, ``codes`` the code buffers' (what group_codes wrote)."""
    import torch
    from ._util import check, lib, ptr, require_cuda, stream_handle
    from .colfilter import BATCH_FIELDS
    for x, name in ((bitmap, "bitmap"), (vals, "vals"), (codes, "codes")):
        require_cuda(x, name)
    if vals.dtype != torch.int64 or vals.dim() != 2 or vals.shape[1] != BATCH_FIELDS:
        raise ValueError("vals: int64 (n, 5)")
    if codes.shape != vals.shape or codes.dtype != torch.int64:
        raise ValueError("codes: a table of the same batches")
    if bitmap.numel() < nwords:
        raise ValueError("bitmap too small")
    if not nwords or not vals.shape[0]:
        return
    ent = t.entries[e]
    check(lib().strom_group_agg(ent.code, ent.ops, ptr(bitmap), nwords, ptr(vals), ptr(codes),
                                vals.shape[0], int(t.args[e].acc), t.capacity,
                                COMBINE if combine is None else int(combine),
                                stream_handle(stream)), "group_agg")


def group_agg_many(t: DeviceGroups, bitmap, nwords: int, codes_ptr: int, nbatches: int,
                   combine=None, stream=None) -> None:
    """One launch per entry over a group, in one native call: ``t.args[e].vals``
    set to each entry's batch table, ``codes_ptr`` the code buffers' table."""
    from ._util import check, lib, ptr, stream_handle
    if not nwords or not nbatches:
        return
    check(lib().strom_group_agg_many(C.byref(t.args), len(t.args), ptr(bitmap), nwords, codes_ptr,
                                     nbatches, t.capacity,
                                     COMBINE if combine is None else int(combine),
                                     stream_handle(stream)), "group_agg")


def compact(t: DeviceGroups):
    """(header uint64[HDR_WORDS], Groups) of a table, on the current stream:
    the occupied slots and the two reserved codes are gathered on the device
    (keys plus accumulator rows, a block of ngroups columns) and only that and
    the header cross to the host."""
    import torch
    C_ = t.capacity
    slots = t.table[HDR_WORDS:]
    idx = torch.nonzero(slots != -(1 << 63)).reshape(-1)
    # ascending by key value on the device (a million keys sort in well under
    # a millisecond there): unsigned order is signed order with the top bit flipped
    keys_d = slots[idx]
    keys_d, order = torch.sort(keys_d ^ -(1 << 63) if t.unsigned else keys_d)
    idx = torch.cat([idx[order], torch.tensor([C_, C_ + 1], dtype=torch.int64,
                                              device=idx.device)])
    keys = keys_d.cpu().numpy()
    rows = t.acc[:, idx].cpu().numpy().view(np.uint64)
    hdr = t.header()
    nk = len(keys)
    wide = np.uint64 if t.unsigned else np.int64
    keys = (keys.view(np.uint64) ^ EMPTY) if t.unsigned else keys
    cols = np.arange(nk + 1)                           # the null keys' row last
    if hdr[H_HAS_EMPTY]:
        # the free slot's pattern: INT64_MIN sorts first, 2^63 where it belongs
        e = np.array([EMPTY]).view(wide)[0]
        at = int(np.searchsorted(keys, e))
        keys = np.insert(keys, at, e)
        cols = np.insert(cols, at, nk + 1)
    lay = GroupLayout(t.entries, len(keys) + 1)
    block = np.zeros(lay.words, np.uint64)
    for e in range(len(t.entries)):
        n = A.nacc(t.entries[e].ops)
        block[lay.off[e]:lay.off[e] + n * lay.nslots] = \
            rows[int(t.row[e]):int(t.row[e]) + n][:, cols].reshape(-1)
    return hdr, Groups(t.entries, keys.astype(wide, copy=False), block)
