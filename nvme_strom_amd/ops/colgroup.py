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

GROUP BY several columns (``KeySpec``, ``group_codes_multi``,
``host_group_agg_multi``): the components are packed into the one key word,
so that unsigned order of the words is lexicographic order of the tuples;
everything above then holds with uint64 keys, and ``Groups.spec`` says how to
take them apart again.  A null component is a bit of the word: the null
keys' slot stays empty on that path.

Semantics are colagg's; float sums are added with global atomics on the
device, in the order the rows arrive: they are not bitwise reproducible from
run to run (the LDS path's keyed float sums are not either).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence

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


# ------------------------------------------------------------ composite keys
MAX_KEYS = 4
H_RANGE = 4                               # header words 4 .. 7: rows a component did not fit


@dataclass(frozen=True)
class KeyComp:
    """One component of a composite key: ``storage`` how its values are
    stored ("i1" .. "u8"), ``bits`` the value bits of its field, ``nullable``
    one more bit on top for a null, ``shift`` the field's lowest bit."""
    name: str
    storage: str
    bits: int
    nullable: bool
    shift: int

    @property
    def width(self) -> int:
        return self.bits + int(self.nullable)

    @property
    def signed(self) -> bool:
        return self.storage[0] == "i"


class KeySpec:
    """How the components of ``GROUP BY a, b, ...`` share the table's one
    64-bit key word (strom.h, strom_group_codes_multi): the first component
    in the most significant used bits, a signed value biased by
    2^(bits - 1), a null as the field's top bit alone — unsigned order of
    the word is lexicographic order of the tuples, nulls after all values.
    The kernel and the numpy twin both pack by this object, so they agree
    key by key.

    ``comps``: (name, storage, bits or None, nullable) per component, at most
    four; ``bits`` None is the storage width.  Field widths over 64 bits in
    all raise NotImplementedError."""

    def __init__(self, comps):
        comps = [(str(n), str(s), b, bool(nu)) for n, s, b, nu in comps]
        if not comps:
            raise ValueError("a composite key needs a component")
        if len(comps) > MAX_KEYS:
            raise NotImplementedError(f"GROUP BY {len(comps)} key columns: at most {MAX_KEYS} "
                                      "components are packed into the 64-bit key")
        for n, s, b, nu in comps:
            if s not in KEY_CODE:
                raise NotImplementedError(f"hash GROUP BY component {n} of storage {s}: integer "
                                          "columns")
            full = 8 * np.dtype(s).itemsize
            if b is not None and not 1 <= int(b) <= full:
                raise ValueError(f"bits={b} for {n}: 1 <= bits <= {full}, its storage width")
        widths = [(int(b) if b is not None else 8 * np.dtype(s).itemsize) + int(nu)
                  for _, s, b, nu in comps]
        if sum(widths) > 64:
            each = ", ".join(f"{n}: {w}" + (" (1 for nulls)" if nu else "")
                             for (n, _, _, nu), w in zip(comps, widths))
            raise NotImplementedError(
                f"GROUP BY key of {sum(widths)} bits ({each}): the packed key holds 64; declare "
                "narrower value ranges with bits={column: n}")
        out, top = [], sum(widths)
        for (n, s, b, nu), w in zip(comps, widths):
            top -= w
            out.append(KeyComp(n, s, w - int(nu), nu, top))
        self.comps: List[KeyComp] = out

    def __len__(self) -> int:
        return len(self.comps)

    def __eq__(self, other) -> bool:
        return isinstance(other, KeySpec) and self.comps == other.comps

    def __repr__(self) -> str:
        return "KeySpec(" + ", ".join(f"{c.name}:{c.storage}/{c.bits}" + ("?" if c.nullable else "")
                                      for c in self.comps) + ")"

    @property
    def names(self) -> List[str]:
        return [c.name for c in self.comps]

    def args(self):
        """The strom_group_keys argument."""
        from .._native import GroupKeys
        a = GroupKeys()
        a.nkeys = len(self.comps)
        for i, c in enumerate(self.comps):
            a.k[i].type, a.k[i].bits = KEY_CODE[c.storage], c.bits
            a.k[i].shift, a.k[i].nullable = c.shift, int(c.nullable)
        return a

    def pack_why(self, columns, valids):
        """(packed uint64, bad int8): ``bad`` is -1 for a row whose every
        component fits, else the first component that does not (a value
        outside its ``bits``, or a null in a component that is not
        nullable); such a row's packed word means nothing."""
        n = len(columns[0]) if len(columns) else 0
        packed = np.zeros(n, np.uint64)
        bad = np.full(n, -1, np.int8)
        for i, c in enumerate(self.comps):
            v = np.asarray(columns[i])[:n]
            if v.dtype.kind not in "iu":
                raise NotImplementedError(f"component {c.name} of dtype {v.dtype}: integer columns")
            if c.signed:
                u = v.astype(np.int64).view(np.uint64) + np.uint64(1 << (c.bits - 1))
            else:
                u = v.astype(np.uint64)
            fits = np.ones(n, bool) if c.bits == 64 else (u >> np.uint64(c.bits)) == 0
            ok = valids[i] if valids is not None else None
            if ok is not None:
                null = ~np.asarray(ok, bool)[:n]
                u = np.where(null, np.uint64((1 << c.bits) & (2**64 - 1)), u)
                fits = np.where(null, c.nullable, fits)
            bad = np.where((bad < 0) & ~fits, np.int8(i), bad)
            packed |= np.where(fits, u, np.uint64(0)) << np.uint64(c.shift)
        return packed, bad

    def pack(self, columns, valids=None):
        """(packed uint64, fits bool) of rows given per component as values
        (integer arrays) and validity (bool array or None)."""
        packed, bad = self.pack_why(columns, valids)
        return packed, bad < 0

    def unpack(self, packed):
        """([values per component, in its storage dtype], [valid bool per
        component]) of packed keys; a null's value is 0."""
        p = np.asarray(packed, np.uint64)
        vals, oks = [], []
        for c in self.comps:
            f = p >> np.uint64(c.shift)
            null = np.zeros(len(p), bool)
            if c.nullable:
                null = ((f >> np.uint64(c.bits)) & np.uint64(1)).astype(bool)
            if c.bits < 64:
                f = f & np.uint64((1 << c.bits) - 1)
            if c.signed:
                f = (f - np.uint64(1 << (c.bits - 1))).view(np.int64)
            v = f.astype(np.dtype(c.storage))
            v[null] = 0
            vals.append(v)
            oks.append(~null)
        return vals, oks


# ------------------------------------------------------------ numpy twin
@dataclass
class Groups:
    """key -> accumulators: ``keys`` ascending by value, ``block`` a colagg
    block of ``GroupLayout(entries, len(keys) + 1)`` (last slot: null keys).
    With a composite key ``keys`` are the packed words (uint64) and ``spec``
    the KeySpec that packed them; the null keys' slot stays empty."""
    entries: List[A.Entry]
    keys: np.ndarray
    block: np.ndarray
    spec: Optional[KeySpec] = None

    @property
    def layout(self) -> GroupLayout:
        return GroupLayout(self.entries, len(self.keys) + 1)

    def arrays(self, e: int) -> dict:
        return A.entry_arrays(self.layout, self.block, e)


def empty_groups(entries: Sequence[A.Entry], unsigned: bool = False,
                 spec: Optional[KeySpec] = None) -> Groups:
    ents = list(entries)
    return Groups(ents, np.zeros(0, np.uint64 if unsigned or spec is not None else np.int64),
                  A.new_block(GroupLayout(ents, 1)), spec)


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


def host_group_agg_multi(entries: Sequence[A.Entry], sel, spec: KeySpec, columns, valids, cols):
    """One batch through the composite-key twin: ``columns`` / ``valids`` the
    components (values, validity or None), packed by ``spec`` as the kernel
    packs them.  Returns (Groups with the packed keys ascending, the selected
    rows per component that did not fit it and were left out)."""
    sel = np.asarray(sel, bool)
    n = len(sel)
    packed, bad = spec.pack_why([np.asarray(c)[:n] for c in columns],
                                [None if v is None else np.asarray(v, bool)[:n] for v in valids])
    misfit = np.bincount(bad[sel & (bad >= 0)].astype(np.int64), minlength=len(spec))
    g = host_group_agg(entries, sel & (bad < 0), packed, None, cols)
    g.spec = spec
    return g, misfit.astype(np.int64)


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
    if a.spec != b.spec:
        raise ValueError(f"merge: keys packed differently ({a.spec} and {b.spec})")
    keys = np.union1d(a.keys, b.keys)
    lay = GroupLayout(a.entries, len(keys) + 1)
    return Groups(a.entries, keys, A.merge_blocks(lay, _spread(a, keys), _spread(b, keys)),
                  a.spec)


# ------------------------------------------------------------ device
class DeviceGroups:
    """A table on the device: ``table`` int64[HDR_WORDS + capacity] (header,
    key words), ``acc`` int64[narrays, capacity + 2] — entry e's arrays are
    rows ``row[e] .. row[e] + popcount(ops)``.  ``spec``: the table holds
    composite keys packed by that KeySpec (uint64 words)."""

    def __init__(self, entries: Sequence[A.Entry], groups: int, device, unsigned: bool = False,
                 stream=None, spec: Optional[KeySpec] = None):
        import torch
        from ._util import check, lib, ptr, stream_handle
        self.entries = list(entries)
        for e in self.entries:
            if not A.nacc(e.ops):
                raise ValueError("an entry needs COUNT, SUM, MIN or MAX")
        self.groups = check_groups(groups)
        self.capacity = capacity(self.groups)
        self.spec = spec
        self.unsigned = bool(unsigned) or spec is not None
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


def group_codes_multi(t: DeviceGroups, keys, nwords: int, src, dst, codes, stream=None) -> None:
    """strom_group_codes_multi over a group with the table's KeySpec:
    ``keys`` the components' strom_filter_batch tables, int64
    (len(spec), nbatches, 5), all over the same batches; the rest as
    group_codes.  A component's values may be the code buffers themselves."""
    import torch
    from ._util import check, lib, ptr, require_cuda, stream_handle
    from .colfilter import BATCH_FIELDS
    if t.spec is None:
        raise ValueError("group_codes_multi: the table was made without a KeySpec")
    for x, name in ((keys, "keys"), (src, "src"), (dst, "dst"), (codes, "codes")):
        require_cuda(x, name)
    if keys.dtype != torch.int64 or keys.dim() != 3 or keys.shape[0] != len(t.spec) or \
            keys.shape[2] != BATCH_FIELDS or not keys.is_contiguous():
        raise ValueError(f"keys: contiguous int64 ({len(t.spec)}, n, 5)")
    if codes.shape != keys.shape[1:] or codes.dtype != torch.int64:
        raise ValueError("codes: a table of the same batches")
    if src.numel() < nwords or dst.numel() < nwords:
        raise ValueError("bitmap too small")
    if not nwords or not keys.shape[1]:
        return
    check(lib().strom_group_codes_multi(t.spec.args(), ptr(t.table), t.capacity, ptr(keys),
                                        keys.shape[1], nwords, ptr(src), ptr(dst), ptr(codes),
                                        stream_handle(stream)), "group_codes_multi")


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
    return hdr, Groups(t.entries, keys.astype(wide, copy=False), block, t.spec)
