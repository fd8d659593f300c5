"""Hash join of a scan's foreign-key column with a dimension table
(csrc/kernels/coljoin.hip): the device build and probe, and a numpy twin
with the same hash, the same layout and the same displacement bound.

The table is an array of 64-bit words, the same on the device and in the
twin: ``HDR_WORDS`` header words (strom.h: capacity, keys, largest
displacement, duplicates, whether the key ``EMPTY`` is present, its
payload), then ``capacity`` slots of (key, payload).  Linear probing from
``hash64(key) & (capacity - 1)``; a free slot holds ``EMPTY``, and since
every int64 is a legal key that one key lives in the header.  A probe looks
at no more than ``MAXDISP + 1`` slots.

Where a key lands depends on the order of insertion (on the device: on
which thread's CAS came first), so two builds of the same keys agree in
membership, payloads, key and duplicate counts — not slot by slot, and the
displacement bound of either is valid for its own table only.

Semantics (pinned to ``pyarrow.Table.join``): a null foreign key matches
nothing, so a semi-join drops it and an anti-join keeps it.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

HDR_WORDS = 8
H_CAPACITY, H_NKEYS, H_MAXDISP, H_DUPS, H_HAS_EMPTY, H_EMPTY_PAYLOAD = range(6)
EMPTY = np.uint64(1 << 63)               # the bits of INT64_MIN
SEMI, ANTI = 0, 1
HOW = {"semi": SEMI, "anti": ANTI}
# STROM_COL_* of the foreign-key storage types the probe reads
FK_CODE = {"i4": 1, "i8": 2, "i1": 5, "i2": 6, "u1": 7, "u2": 8, "u4": 9, "u8": 10}
_M1 = np.uint64(0xFF51AFD7ED558CCD)
_M2 = np.uint64(0xC4CEB9FE1A85EC53)
_S33 = np.uint64(33)


def capacity(n: int) -> int:
    """Slots of a table of ``n`` keys: a power of two, >= 2n and >= 64."""
    c = 64
    while c < 2 * int(n):
        c <<= 1
    return c


def hash64(keys) -> np.ndarray:
    """murmur3's 64-bit finalizer of the keys' int64 bits (uint64 array)."""
    k = np.atleast_1d(np.asarray(keys)).astype(np.int64, copy=False).view(np.uint64).copy()
    k ^= k >> _S33
    k *= _M1
    k ^= k >> _S33
    k *= _M2
    k ^= k >> _S33
    return k


def widen(values) -> Tuple[np.ndarray, np.ndarray]:
    """(int64 keys, can match) of foreign-key values of any integer dtype:
    uint64 is compared by value, so values >= 2^63 match nothing."""
    v = np.asarray(values)
    if v.dtype.kind not in "iu":
        raise NotImplementedError(f"join key of dtype {v.dtype}: integer columns are joined")
    if v.dtype == np.uint64:
        return v.view(np.int64), v <= np.uint64((1 << 63) - 1)
    return v.astype(np.int64), np.ones(len(v), bool)


# ------------------------------------------------------------ numpy twin
@dataclass
class HostTable:
    words: np.ndarray                    # uint64[HDR_WORDS + 2 * capacity]

    @property
    def header(self) -> np.ndarray:
        return self.words[:HDR_WORDS]

    @property
    def capacity(self) -> int:
        return int(self.words[H_CAPACITY])

    @property
    def slots(self) -> np.ndarray:
        """(capacity, 2) view: key, payload."""
        return self.words[HDR_WORDS:].reshape(-1, 2)

    @property
    def nkeys(self) -> int:
        return int(self.words[H_NKEYS])

    @property
    def dups(self) -> int:
        return int(self.words[H_DUPS])

    @property
    def maxdisp(self) -> int:
        return int(self.words[H_MAXDISP])

    def items(self) -> dict:
        """{key: payload} of everything in the table (the payload as the
        int32 a lookup returns)."""
        s = self.slots
        used = s[:, 0] != EMPTY
        pay = s[used, 1].astype(np.uint32).view(np.int32)
        out = dict(zip(s[used, 0].view(np.int64).tolist(), pay.tolist()))
        if self.words[H_HAS_EMPTY]:
            out[-(1 << 63)] = int(self.words[H_EMPTY_PAYLOAD:H_EMPTY_PAYLOAD + 1]
                                  .astype(np.uint32).view(np.int32)[0])
        return out

    def true_maxdisp(self) -> int:
        """The largest distance of a stored key from its home slot."""
        s = self.slots
        at = np.flatnonzero(s[:, 0] != EMPTY)
        if not len(at):
            return 0
        cap = np.uint64(self.capacity)
        home = hash64(s[at, 0].view(np.int64)) & (cap - np.uint64(1))
        return int(((at.astype(np.uint64) - home) & (cap - np.uint64(1))).max())


def host_build(keys, payload=None, cap: Optional[int] = None) -> HostTable:
    """What strom_join_build leaves for one order of arrival: the keys are
    inserted in rounds, in each round every pending key tries its next slot
    and the first of the contenders for a free slot takes it.  ``payload``
    (int32 per key) defaults to the build row.  Returns the table; its
    header counts the keys and the duplicates (a key met again is dropped)."""
    keys = np.asarray(keys).astype(np.int64, copy=False).reshape(-1)
    n = len(keys)
    pay = (np.arange(n, dtype=np.int64) if payload is None
           else np.asarray(payload).astype(np.int64)).astype(np.uint32).astype(np.uint64)
    cap = capacity(n) if cap is None else int(cap)
    if cap < 64 or cap & (cap - 1) or cap < 2 * n:
        raise ValueError("capacity: a power of two >= 2n and >= 64")
    words = np.zeros(HDR_WORDS + 2 * cap, np.uint64)
    words[H_CAPACITY] = cap
    t = HostTable(words)
    slots = t.slots
    slots[:, 0] = EMPTY
    ku = keys.view(np.uint64)
    mask = np.uint64(cap - 1)
    nkeys = dups = maxd = 0
    emp = np.flatnonzero(ku == EMPTY)
    if len(emp):
        words[H_HAS_EMPTY], words[H_EMPTY_PAYLOAD] = 1, pay[emp[0]]
        nkeys, dups = 1, len(emp) - 1
    pend = np.flatnonzero(ku != EMPTY)
    at = hash64(keys[pend]) & mask
    disp = np.zeros(len(pend), np.int64)
    while len(pend):
        cur = slots[at.astype(np.int64), 0]
        same = cur == ku[pend]
        dups += int(same.sum())
        free = cur == EMPTY
        # one winner per free slot: the first contender in build order
        win = np.zeros(len(pend), bool)
        fi = np.flatnonzero(free)
        if len(fi):
            _, first = np.unique(at[fi], return_index=True)
            win[fi[first]] = True
            w = fi[first]
            slots[at[w].astype(np.int64), 0] = ku[pend[w]]
            slots[at[w].astype(np.int64), 1] = pay[pend[w]]
            nkeys += len(w)
            maxd = max(maxd, int(disp[w].max()))
        # a loser looks at the same slot again (the winner may hold its key);
        # a key that met another key moves on
        move = ~free & ~same
        keep = ~win & ~same
        at = np.where(move, (at + np.uint64(1)) & mask, at)[keep]
        disp = (disp + move)[keep]
        pend = pend[keep]
    words[H_NKEYS], words[H_DUPS], words[H_MAXDISP] = nkeys, dups, maxd
    return t


def host_lookup(t: HostTable, keys, active=None) -> Tuple[np.ndarray, np.ndarray]:
    """(match, payload) per int64 key, walking exactly as the probe kernel:
    from the home slot, until the key or a free slot is met, at most
    ``MAXDISP + 1`` slots.  ``active`` False: the row is not probed."""
    keys = np.asarray(keys).astype(np.int64, copy=False).reshape(-1)
    ku = keys.view(np.uint64)
    n = len(keys)
    match = np.zeros(n, bool)
    pay = np.zeros(n, np.int32)
    act = np.ones(n, bool) if active is None else np.asarray(active, bool).copy()
    emp = act & (ku == EMPTY)
    if emp.any():
        match[emp] = bool(t.words[H_HAS_EMPTY])
        pay[emp] = np.uint32(t.words[H_EMPTY_PAYLOAD]).astype(np.int32)
    idx = np.flatnonzero(act & ~emp)
    mask = np.uint64(t.capacity - 1)
    at = hash64(keys[idx]) & mask
    slots = t.slots
    for _ in range(min(t.maxdisp, t.capacity - 1) + 1):
        if not len(idx):
            break
        cur = slots[at.astype(np.int64)]
        hit = cur[:, 0] == ku[idx]
        match[idx[hit]] = True
        pay[idx[hit]] = cur[hit, 1].astype(np.uint32).view(np.int32)
        go = ~hit & (cur[:, 0] != EMPTY)
        idx, at = idx[go], (at[go] + np.uint64(1)) & mask
    return match, pay


def host_probe(t: HostTable, batches: Sequence[tuple], src: np.ndarray, how: str = "semi",
               key_out: Optional[List[np.ndarray]] = None):
    """The probe kernel's result over record batches: ``batches`` is a list
    of (fk values, valid bool or None), batch b on fresh bitmap words;
    ``src`` the source words (bits beyond a batch's rows are ignored).
    Returns (destination words uint64, key output): ``key_out`` (one int32
    array per batch, copied) gets the payload of each selected matched row
    and is otherwise left as it was."""
    anti = HOW[how] == ANTI
    if anti and key_out is not None:
        raise ValueError("an anti-join has no key output")
    src = np.asarray(src).view(np.uint64)
    dst = np.zeros(len(src), np.uint64)
    out = [k.copy() for k in key_out] if key_out is not None else None
    w0 = 0
    for b, (v, ok) in enumerate(batches):
        n = len(v)
        nw = (n + 63) // 64
        sel = np.unpackbits(src[w0:w0 + nw].view(np.uint8), bitorder="little")[:n].astype(bool)
        keys, can = widen(v)
        act = sel & can & (np.ones(n, bool) if ok is None else np.asarray(ok, bool)[:n])
        m, pay = host_lookup(t, keys, act)
        res = sel & ~m if anti else sel & m
        bits = np.zeros(nw * 64, np.uint8)
        bits[:n] = res
        dst[w0:w0 + nw] = np.packbits(bits, bitorder="little").view(np.uint64)
        if out is not None:
            out[b][:n][m & sel] = pay[m & sel]
        w0 += nw
    return dst, out


# ------------------------------------------------------------ device
class DeviceTable:
    """A table built on the device: ``words`` is the int64 tensor of header
    and slots (16-byte aligned)."""

    def __init__(self, words, cap: int):
        self.words = words
        self.capacity = int(cap)

    def header(self) -> np.ndarray:
        """The header on the host (synchronizes with the build)."""
        return self.words[:HDR_WORDS].cpu().numpy().view(np.uint64).copy()

    def to_host(self) -> HostTable:
        return HostTable(self.words.cpu().numpy().view(np.uint64).copy())


def build(keys, payload=None, cap: Optional[int] = None, stream=None) -> DeviceTable:
    """strom_join_build: ``keys`` an int64 device tensor, ``payload`` an
    int32 device tensor of the same length or None (the build row)."""
    import torch
    from ._util import check, lib, ptr, require_cuda, stream_handle
    require_cuda(keys, "keys")
    if keys.dtype != torch.int64 or keys.dim() != 1:
        raise ValueError("keys: int64 (n,)")
    n = keys.numel()
    if payload is not None:
        require_cuda(payload, "payload")
        if payload.dtype != torch.int32 or payload.numel() != n:
            raise ValueError("payload: int32, one per key")
    cap = capacity(n) if cap is None else int(cap)
    if cap < 64 or cap & (cap - 1) or cap < 2 * n:
        raise ValueError("capacity: a power of two >= 2n and >= 64")
    words = torch.empty(HDR_WORDS + 2 * cap, dtype=torch.int64, device=keys.device)
    check(lib().strom_join_build(ptr(keys) if n else 0, ptr(payload) if payload is not None else 0,
                                 n, ptr(words), cap, stream_handle(stream)), "join_build")
    return DeviceTable(words, cap)


def probe(table: DeviceTable, fk_code: int, fk, nwords: int, src, dst, count, how: int = SEMI,
          key_out=None, stream=None) -> None:
    """strom_column_join over a group: ``fk`` the (nbatches, 5)
    strom_filter_batch table of the foreign-key column, ``src`` / ``dst``
    the bitmaps (may be the same tensor), ``count`` int64[1] on the device
    (+= popcount of the words written), ``key_out`` a table of the same
    batches whose values point to int32 buffers (semi-join only)."""
    import torch
    from ._util import check, lib, ptr, require_cuda, stream_handle
    from .colfilter import BATCH_FIELDS
    for t, name in ((fk, "fk"), (src, "src"), (dst, "dst"), (count, "count")):
        require_cuda(t, name)
    if fk.dtype != torch.int64 or fk.dim() != 2 or fk.shape[1] != BATCH_FIELDS:
        raise ValueError("fk: int64 (n, 5)")
    if key_out is not None and (key_out.shape != fk.shape or key_out.dtype != torch.int64):
        raise ValueError("key_out: a table of the same batches")
    if src.numel() < nwords or dst.numel() < nwords:
        raise ValueError("bitmap too small")
    if fk_code not in FK_CODE.values():
        raise NotImplementedError(f"join on storage type {fk_code}: integer columns are joined")
    if not nwords or not fk.shape[0]:
        return
    check(lib().strom_column_join(fk_code, how, ptr(table.words), table.capacity, ptr(fk),
                                  fk.shape[0], nwords, ptr(src), ptr(dst),
                                  ptr(key_out) if key_out is not None else 0, ptr(count),
                                  stream_handle(stream)), "column_join")


# ------------------------------------------------------------ star join
MAX_LEGS = 4


def _how(how) -> int:
    """SEMI / ANTI of "semi" / "anti" or the code itself."""
    return HOW[how] if isinstance(how, str) and how in HOW else how


def _check_legs(legs, ntables: int) -> None:
    """The rules of strom_column_join_star's legs, for the wrapper and the twin:
    ``legs`` items are (table, ..., how, kout)."""
    if not 1 <= len(legs) <= MAX_LEGS:
        raise ValueError(f"a star join has 1 .. {MAX_LEGS} legs")
    seen = set()
    for leg in legs:
        how, kout = leg[-2], leg[-1]
        if how not in (SEMI, ANTI):
            raise ValueError(f"leg how={how!r}: SEMI or ANTI")
        if kout is None or kout < 0:
            continue
        if how == ANTI:
            raise ValueError("an anti-join leg has no key output")
        if kout >= ntables or kout in seen:
            raise ValueError("kout: the index of a code table, each used by one leg")
        seen.add(kout)


def host_probe_star(legs: Sequence[tuple], fk_batches: Sequence[Sequence[tuple]], src: np.ndarray,
                    key_out: Optional[List[List[np.ndarray]]] = None):
    """strom_column_join_star's result over record batches.  ``legs``: per
    leg (HostTable, how SEMI / ANTI or its name, kout: index into ``key_out`` or -1);
    ``fk_batches[i]``: leg i's list of (fk values, valid bool or None), one per
    batch, batch b on fresh bitmap words; ``src`` the source words (bits beyond
    a batch's rows are ignored); ``key_out[j]``: one int32 array per batch.
    Returns (destination words uint64, key output copied): a leg's payload is
    stored for exactly the rows of the destination, every other element of a
    code buffer is left as it was."""
    legs = [(t, _how(how), -1 if kout is None else int(kout)) for t, how, kout in legs]
    _check_legs(legs, len(key_out) if key_out is not None else 0)
    if len(fk_batches) != len(legs) or any(len(f) != len(fk_batches[0]) for f in fk_batches):
        raise ValueError("fk_batches: one list of the same batches per leg")
    src = np.asarray(src).view(np.uint64)
    dst = np.zeros(len(src), np.uint64)
    out = [[k.copy() for k in tab] for tab in key_out] if key_out is not None else None
    w0 = 0
    for b in range(len(fk_batches[0])):
        n = len(fk_batches[0][b][0])
        nw = (n + 63) // 64
        cur = np.unpackbits(src[w0:w0 + nw].view(np.uint8), bitorder="little")[:n].astype(bool)
        pays = []
        for (t, how, _), fks in zip(legs, fk_batches):
            v, ok = fks[b]
            if len(v) != n:
                raise ValueError("fk_batches: the legs' batches differ in rows")
            keys, can = widen(v)
            # a row an earlier leg dropped is not probed
            act = cur & can & (np.ones(n, bool) if ok is None else np.asarray(ok, bool)[:n])
            m, pay = host_lookup(t, keys, act)
            cur = cur & ~m if how == ANTI else cur & m
            pays.append(pay)
        bits = np.zeros(nw * 64, np.uint8)
        bits[:n] = cur
        dst[w0:w0 + nw] = np.packbits(bits, bitorder="little").view(np.uint64)
        for (_, _, kout), pay in zip(legs, pays):
            if kout >= 0:
                out[kout][b][:n][cur] = pay[cur]
        w0 += nw
    return dst, out


def probe_star(legs: Sequence[tuple], fk_tables, nwords: int, src, dst, count, key_out=None,
               stream=None) -> None:
    """strom_column_join_star over a group: every leg in one walk of the
    bitmap.  ``legs``: per leg (DeviceTable, fk storage code, how SEMI / ANTI,
    kout: index of its code table in ``key_out`` or -1), in probe order;
    ``fk_tables`` the legs' strom_filter_batch tables, contiguous int64
    (len(legs), nbatches, 5) over the same batches; ``src`` / ``dst`` /
    ``count`` as probe; ``key_out`` contiguous int64 (ntables, nbatches, 5),
    values pointing to int32 buffers (semi legs only)."""
    import torch
    from .._native import JoinLegs
    from ._util import check, lib, ptr, require_cuda, stream_handle
    from .colfilter import BATCH_FIELDS
    legs = [(t, int(code), _how(how), -1 if kout is None else int(kout))
            for t, code, how, kout in legs]
    _check_legs(legs, key_out.shape[0] if key_out is not None else 0)
    for t, name in ((fk_tables, "fk_tables"), (src, "src"), (dst, "dst"), (count, "count")):
        require_cuda(t, name)
    if fk_tables.dtype != torch.int64 or fk_tables.dim() != 3 or \
            fk_tables.shape[0] != len(legs) or fk_tables.shape[2] != BATCH_FIELDS or \
            not fk_tables.is_contiguous():
        raise ValueError(f"fk_tables: contiguous int64 ({len(legs)}, n, 5)")
    if key_out is not None:
        require_cuda(key_out, "key_out")
        if key_out.dtype != torch.int64 or key_out.dim() != 3 or \
                key_out.shape[1:] != fk_tables.shape[1:] or not key_out.is_contiguous():
            raise ValueError("key_out: contiguous int64 (tables, n, 5) of the same batches")
    if src.numel() < nwords or dst.numel() < nwords:
        raise ValueError("bitmap too small")
    a = JoinLegs()
    a.nlegs = len(legs)
    for i, (t, code, how, kout) in enumerate(legs):
        if code not in FK_CODE.values():
            raise NotImplementedError(f"join on storage type {code}: integer columns are joined")
        a.leg[i].table, a.leg[i].capacity = ptr(t.words), t.capacity
        a.leg[i].type, a.leg[i].how, a.leg[i].kout = code, how, kout
    if not nwords or not fk_tables.shape[1]:
        return
    check(lib().strom_column_join_star(a, ptr(fk_tables), fk_tables.shape[1], nwords, ptr(src),
                                       ptr(dst), ptr(key_out) if key_out is not None else 0,
                                       ptr(count), stream_handle(stream)), "column_join_star")
