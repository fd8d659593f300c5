"""Tables and a brute-force reference for the aggregate, group and join
kernels (csrc/kernels/colagg.hip, colgroup.hip, coljoin.hip), shared by
tests/test_kagg_cpu.py (the numpy twins) and tests/test_gpu_kagg.py (the
kernels).

Tables have the layout the kernels get: one strom_filter_batch row
(values, valid, nrows, word_base, row_base) per record batch, every batch on
fresh bitmap words.  The geometry is tests/qualgen.py's — one row, both sides
of a word, empty batches that share a word_base with their neighbour, several
trips of a wave — plus a leading empty batch and a trailing one whose
word_base is the number of words.  Validity buffers are dirty past nrows,
bitmaps carry garbage past each batch's rows.

The reference looks at one row at a time: the row counts if its bit is set
and it exists; its key is null, malformed or a group; its value is valid or
not.  Counts are Python ints, integer sums Python ints mod 2^64, float values
are kept per group for math.fsum, min and max are Python comparisons that
skip NaN.  It uses the constants, layout accessors and decoders of
ops/colagg.py, ops/colgroup.py and ops/coljoin.py and none of their host_*
twins.

Comparison rule (tests/agggen.py's, extended to non-finite values): counts,
integer sums and integer min / max are exact.  A float min or max must == the
reference's and be, bit for bit, one of the group's own values (the sign of
a zero is not pinned); a group whose counted values are all NaN has NaN min
and max.  A float sum is NaN if the group holds a NaN or both infinities, the
infinity if it holds one sign of it, and otherwise within
n * 2^-52 * sum|x| of math.fsum(x).  For a group of subnormals that bound is
below one ulp: the sum must be exact.  Finite pools keep sum|x| < 2^1000, so
no order of summation overflows.
"""
from __future__ import annotations

import math
import struct
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np

import qualgen as Q
from qualgen import GEOMETRY, VALIDITY, valid_words
from nvme_strom_amd.ops import colagg as A

M64 = (1 << 64) - 1
BAD = "bad"                              # the group id of a malformed key
PREFILL = -559038737                     # what a code / payload buffer holds before a launch

# value validity per batch is qualgen's; the key column gets its own modes so
# that the two differ in every batch that has rows (the 129-row batch: only
# null keys)
KEY_VALIDITY = ["dirty", None, "clean", None, "clean", "dirty", None, None, "null"]
GEOMETRIES = {
    "plain": (GEOMETRY, VALIDITY, KEY_VALIDITY),
    "lead": ([0] + GEOMETRY, ["clean"] + VALIDITY, [None] + KEY_VALIDITY),
    "trail": (GEOMETRY + [0], VALIDITY + ["clean"], KEY_VALIDITY + ["dirty"]),
}
BITMAPS = (1.0, 0.5, 0.0)                # dense, 50 %, all-zero

INTS = ["i1", "i2", "i4", "i8", "u1", "u2", "u4", "u8"]
FLOATS = ["f4", "f8"]
VALUE_TYPES = INTS + FLOATS              # the 10 storage types of 11 STROM_COL_* value codes
# key storage types of the LDS kernel and their STROM_COL_* codes
KEY_TYPES = {"i1": 5, "i2": 6, "i4": 1, "i8": 2, "u1": 7, "u2": 8, "u4": 9, "u8": 10,
             "b1": A.COL_BOOL}
POOLS = ["ints", "cancel", "subnormal", "inf", "infs", "nan", "negzero", "zeros", "nullrows"]
NPOOLS = len(POOLS)


def nwords_of(geometry) -> int:
    return sum((n + 63) // 64 for n in geometry)


# ------------------------------------------------------------------ values
def _nan(dt: str, payload: int, neg: bool = False):
    if dt == "f4":
        b = np.array([0x7FC00000 | (payload & 0x3FFFFF) | (0x80000000 if neg else 0)], "<u4")
        return b.view("<f4")[0]
    b = np.array([0x7FF8000000000000 | payload | ((1 << 63) if neg else 0)], "<u8")
    return b.view("<f8")[0]


def pool_values(dt: str, pool: str, n: int, rng) -> np.ndarray:
    """``n`` values of float type ``dt`` from one pool."""
    ints = rng.integers(-1000, 1000, n).astype(dt)
    if pool in ("ints", "nullrows"):
        return ints
    if pool == "cancel":
        # +-1e+-150 (f4: +-1e+-30) with random mantissas, every value next to
        # its negation somewhere: the sum is tiny against sum|x|
        big = 1e150 if dt == "f8" else 1e30
        half = (n + 1) // 2
        mag = np.where(rng.random(half) < 0.5, big, 1.0 / big) * rng.uniform(1, 2, half)
        v = np.concatenate([mag, -mag])[:n].astype(dt)
        rng.shuffle(v)
        return v
    if pool == "subnormal":
        k = rng.integers(1, 1 << 20, n)
        u = "<u8" if dt == "f8" else "<u4"
        sign = (rng.random(n) < 0.5).astype(u) << np.array(8 * np.dtype(u).itemsize - 1, u)
        v = (k.astype(u) | sign).view(dt)
        assert (np.abs(v) < np.finfo(dt).tiny).all() and (v != 0).all()
        return v
    if pool == "inf":
        ints[rng.random(n) < 0.15] = np.inf
        return ints
    if pool == "infs":
        r = rng.random(n)
        ints[r < 0.15] = np.inf
        ints[r > 0.85] = -np.inf
        return ints
    if pool == "nan":
        pick = np.array([_nan(dt, 0), _nan(dt, 1), _nan(dt, 0x1234, True)], dt)
        return pick[rng.integers(0, 3, n)]
    if pool == "negzero":
        return np.full(n, -0.0, dt)
    if pool == "zeros":
        return np.where(rng.random(n) < 0.5, 0.0, -0.0).astype(dt)
    raise KeyError(pool)


def int_values(dt: str, n: int, rng) -> np.ndarray:
    """The type's min and max, 0, -1 and random values over the full range."""
    info = np.iinfo(dt)
    v = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    edge = np.array([info.min, info.max, 0, -1 if info.min < 0 else 1], dtype=dt)
    at = rng.random(n) < 0.3
    v[at] = edge[rng.integers(0, 4, int(at.sum()))]
    return v


# ------------------------------------------------------------------ tables
def _valid(n: int, mode: Optional[str], rng, force_null=None) -> Optional[np.ndarray]:
    ok = Q.make_valid(n, mode, rng)
    if ok is not None and force_null is not None:
        ok = ok & ~force_null
    return ok


def make_table(dt: str, values: np.ndarray, geometry, modes, rng, force_null=None) -> Q.Table:
    """``values`` (one per row) split over the batches, validity by mode;
    ``force_null`` rows are null wherever their batch has a validity buffer."""
    bs, at = [], 0
    for n, mode in zip(geometry, modes):
        fn = None if force_null is None else force_null[at:at + n]
        bs.append(Q.Batch(n, values[at:at + n], _valid(n, mode, rng, fn), mode))
        at += n
    assert at == len(values)
    return Q.Table(dt, bs)


def bitmap(geometry, p: float, rng):
    """(selected rows per batch (bool), the words): bits past a batch's rows
    are random garbage; p == 0 is the all-zero bitmap."""
    words, bits = [], []
    for n in geometry:
        nw = (n + 63) // 64
        r = rng.random(nw * 64) < p
        bits.append(r[:n].copy())
        if p > 0:
            r[n:] = rng.random(nw * 64 - n) < 0.5
        words.append(np.packbits(r, bitorder="little").view(np.uint64))
    return bits, np.concatenate(words) if words else np.zeros(0, np.uint64)


def pack_bits(geometry, bits) -> np.ndarray:
    """Rows per batch as bitmap words, zero past each batch's rows."""
    out = []
    for n, b in zip(geometry, bits):
        pad = np.zeros(((n + 63) // 64) * 64, bool)
        pad[:n] = b
        out.append(np.packbits(pad, bitorder="little").view(np.uint64))
    return np.concatenate(out) if out else np.zeros(0, np.uint64)


def unpack_bits(geometry, words) -> List[np.ndarray]:
    out, w = [], 0
    words = np.asarray(words).view(np.uint64)
    for n in geometry:
        nw = (n + 63) // 64
        out.append(np.unpackbits(words[w:w + nw].view(np.uint8), bitorder="little")[:n]
                   .astype(bool))
        w += nw
    return out


def _values_raw(dt: str, b: Q.Batch) -> bytes:
    if dt == "b1":
        return np.packbits(np.asarray(b.values, bool), bitorder="little").tobytes()
    return np.ascontiguousarray(b.values).tobytes()


def upload(t: Q.Table, dev, keep: list, values: bool = True):
    """The (nbatches, 5) strom_filter_batch table of ``t`` on the device; an
    empty batch's pointers are 0, and so is the values pointer of a column
    the kernel must not read (``values`` False)."""
    import torch
    rows = []
    for k, b in enumerate(t.batches):
        vp = valp = 0
        if b.nrows:
            if values:
                raw = _values_raw(t.dt, b)
                raw += b"\0" * (-len(raw) % 8)
                v = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(dev)
                keep.append(v)
                vp = v.data_ptr()
            vw = valid_words(b)
            if vw is not None:
                vt = torch.from_numpy(vw.view(np.int64).copy()).to(dev)
                keep.append(vt)
                valp = vt.data_ptr()
        rows.append([vp, valp, b.nrows, t.word_base[k], t.row_base[k]])
    arr = np.array(rows, dtype=np.uint64).view(np.int64).reshape(-1, 5)
    tab = torch.from_numpy(arr.copy()).to(dev)
    keep.append(tab)
    return tab


def code_buffers(geometry, dev, keep: list):
    """(int32 buffer of 64 elements per bitmap word, prefilled; its batch
    table): batch b's codes start at its first word, an empty batch has no
    buffer."""
    import torch
    nw = nwords_of(geometry)
    buf = torch.full((max(nw, 1) * 64,), PREFILL, dtype=torch.int32, device=dev)
    rows, w = [], 0
    for n in geometry:
        rows.append([buf.data_ptr() + w * 256 if n else 0, 0, n, w, 0])
        w += (n + 63) // 64
    tab = torch.from_numpy(np.array(rows, np.int64)).to(dev)
    keep.extend([buf, tab])
    return buf, tab


def expected_buffer(geometry, per_batch) -> np.ndarray:
    """The whole code buffer: ``per_batch`` rows in place, PREFILL elsewhere."""
    out = np.full(max(nwords_of(geometry), 1) * 64, PREFILL, np.int32)
    w = 0
    for n, v in zip(geometry, per_batch):
        out[w * 64:w * 64 + n] = v
        w += (n + 63) // 64
    return out


# --------------------------------------------------------------- reference
@dataclass
class Acc:
    rows: int = 0                        # selected rows of the group (COUNT | ALL)
    count: int = 0                       # of those, the ones with a value
    vals: list = field(default_factory=list)   # Python ints / floats (f4 widened exactly)


def _pylist(t: Q.Table, b: Q.Batch) -> list:
    v = np.asarray(b.values)
    if t.dt == "b1":
        return [int(x) for x in v]
    return (v.astype(np.float64) if v.dtype.kind == "f" else v).tolist()


def reference(bits, val: Optional[Q.Table], gid_of=None, keys: Optional[List[Q.Table]] = None):
    """Row by row: ({group id: Acc}, malformed keys met, per bitmap word the
    list of (group id, has value, is NaN) of its rows that count).
    ``gid_of(k)`` maps the key columns' values of a row (a tuple, None for a
    null component) to a group id or BAD; without keys every row is group 0."""
    groups: Dict[object, Acc] = {}
    nbad, words = 0, []
    nb = len(bits)
    for b in range(nb):
        n = len(bits[b])
        vb = val.batches[b] if val is not None else None
        if vb is not None:
            assert vb.nrows == n
        vals = _pylist(val, vb) if vb is not None and val.dt != "none" else None
        kcols = []
        for kt in keys or []:
            kb = kt.batches[b]
            assert kb.nrows == n
            kcols.append((_pylist(kt, kb), kb.valid))
        log: List[list] = [[] for _ in range((n + 63) // 64)]
        for i in range(n):
            if not bits[b][i]:
                continue
            gid = 0
            if keys is not None:
                gid = gid_of(tuple(None if (ok is not None and not ok[i]) else kv[i]
                                   for kv, ok in kcols))
                if gid == BAD:
                    nbad += 1
                    continue
            acc = groups.setdefault(gid, Acc())
            acc.rows += 1
            has = vb is None or vb.valid is None or bool(vb.valid[i])
            x = None
            if has:
                acc.count += 1
                if vals is not None:
                    x = vals[i]
                    acc.vals.append(x)
            log[i // 64].append((gid, has, isinstance(x, float) and x != x))
        words.extend(log)
    return groups, nbad, words


def slot_gid(nslots: int):
    """colagg's key: a slot in [0, nslots - 1), the last slot for a null,
    malformed otherwise (a uint64 >= 2^63 among them: it is >= nslots - 1)."""
    def f(k):
        k = k[0]
        if k is None:
            return nslots - 1
        return k if 0 <= k < nslots - 1 else BAD
    return f


def value_gid(k):
    """colgroup's key: the key value itself, None for a null key."""
    return k[0]


def witnesses(words, val: Optional[Q.Table], geometry, bm_words) -> set:
    """What a case exercises, from the reference's word log."""
    out = set()
    one = []
    for log in words:
        gids = [g for g, _, _ in log]
        one.append(gids[0] if len(gids) > 1 and len(set(gids)) == 1 else None)
        if one[-1] is not None:
            out.add("run")
        if len(set(gids)) > 1 and gids.count(gids[0]) > 1:
            out.add("combine")
            if any(g == gids[0] and has and nan for g, has, nan in log):
                out.add("mine_nan")
    for w in range(len(one) - 1):
        if w // 4 == (w + 1) // 4 and one[w] is not None and one[w + 1] is not None and \
                one[w] != one[w + 1]:
            out.add("flush")
    if val is not None and any(b.nrows and b.valid is not None and not b.valid.any()
                               for b in val.batches):
        out.add("null_batch")
    w = 0
    for n in geometry:
        nw = (n + 63) // 64
        if n % 64:
            last = int(bm_words[w + nw - 1])
            rows = (1 << (n % 64)) - 1
            if last & rows and last & ~rows & M64:
                out.add("garbage")
        w += nw
    return out


# -------------------------------------------------------------- comparison
def _bits(x: float) -> bytes:
    return struct.pack("<d", x)


def check_float_sum(got: float, vals: list, what=None) -> None:
    """The rule for a float sum of ``vals`` (Python floats, n > 0)."""
    nan = any(x != x for x in vals)
    pinf, ninf = math.inf in vals, -math.inf in vals
    if nan or (pinf and ninf):
        assert math.isnan(got), (what, got)
        return
    if pinf or ninf:
        assert got == (math.inf if pinf else -math.inf), (what, got)
        return
    fs, sabs = math.fsum(vals), math.fsum(abs(x) for x in vals)
    assert sabs < 2.0 ** 1000
    bound = len(vals) * 2.0 ** -52 * sabs
    assert abs(got - fs) <= bound, (what, got, fs, bound)


def check_entry(lay, block, e: int, accs: List[Optional[Acc]], what=None) -> None:
    """Entry ``e`` of a colagg block against the reference's group per slot
    (None: the slot counted no row)."""
    ent = lay.entries[e]
    block = np.asarray(block).view(np.uint64)
    got = A.entry_arrays(lay, block, e)
    raw = {op: block[lay.pos(e, op)] for op in (A.COUNT, A.SUM, A.MIN, A.MAX)
           if lay.pos(e, op) is not None}
    assert len(accs) == lay.nslots
    for j, acc in enumerate(accs):
        w = (what, ent.ops, ent.dtype, j)
        if ent.ops & A.ALL:
            n = acc.rows if acc else 0
        else:
            n = acc.count if acc else 0
        if ent.ops & A.COUNT:
            assert int(got["count"][j]) == n, w + (int(got["count"][j]), n)
        if ent.dtype is None or ent.ops & A.ALL:
            continue
        vals = acc.vals if acc else []
        assert len(vals) == n
        if not n:
            # nothing counted: the identities
            assert A.SUM not in raw or int(raw[A.SUM][j]) == 0, w
            assert A.MIN not in raw or int(raw[A.MIN][j]) == M64, w
            assert A.MAX not in raw or int(raw[A.MAX][j]) == 0, w
            continue
        if not ent.is_float:
            if ent.ops & A.SUM:
                assert int(raw[A.SUM][j]) == sum(vals) & M64, w
            if ent.ops & A.MIN:
                assert int(got["min"][j]) == min(vals), w
            if ent.ops & A.MAX:
                assert int(got["max"][j]) == max(vals), w
            continue
        nn = [x for x in vals if x == x]
        own = {_bits(x) for x in nn}
        for name, op, fn in (("min", A.MIN, min), ("max", A.MAX, max)):
            if not ent.ops & op:
                continue
            g = float(got[name][j])
            if not nn:
                assert math.isnan(g), w + (name, g)
            else:
                assert g == fn(nn) and _bits(g) in own, w + (name, g, fn(nn))
        if ent.ops & A.SUM:
            check_float_sum(float(got["sum"][j]), vals, w)


def entries_of(dt: Optional[str]) -> List[A.Entry]:
    """Every ops mask 1 .. 15 of a value type and COUNT | ALL; without a
    value type COUNT with and without ALL."""
    if dt is None:
        return [A.Entry(A.COUNT, None), A.Entry(A.COUNT | A.ALL, None)]
    return [A.Entry(ops, dt) for ops in range(1, 16)] + [A.Entry(A.COUNT | A.ALL, dt)]


# ------------------------------------------------------------------- cases
@dataclass
class Case:
    """One value column (``val``; dt "none": only its validity exists) and
    the key columns over one geometry.  ``keyvals[j]``: the key value of
    group j (colagg: j itself)."""
    label: str
    geom: str
    dt: Optional[str]
    val: Q.Table
    key: Optional[Q.Table] = None
    key_dt: Optional[str] = None
    nslots: int = 1
    keyvals: Optional[list] = None
    pool_of: Optional[dict] = None       # {group id: float pool its values come from}
    null_gid: object = None              # the group that draws from all pools

    @property
    def geometry(self):
        return [b.nrows for b in self.val.batches]

    @property
    def nwords(self):
        return nwords_of(self.geometry)

    def entries(self):
        return entries_of(self.dt)


def _none_table(geom: str, rng) -> Q.Table:
    g, vm, _ = GEOMETRIES[geom]
    return make_table("none", np.zeros(sum(g), np.int8), g, vm, rng)


def flat_cases(geom: str, seed: int = 1) -> List[Case]:
    """Unkeyed: every integer type, every float pool as its own column (and
    one column that draws from all pools), and the validity-only column."""
    rng = np.random.default_rng(seed)
    g, vm, _ = GEOMETRIES[geom]
    n = sum(g)
    out = [Case(f"flat-{dt}", geom, dt, make_table(dt, int_values(dt, n, rng), g, vm, rng))
           for dt in INTS]
    for dt in FLOATS:
        for pool in POOLS:
            fn = np.ones(n, bool) if pool == "nullrows" else None
            # every row null needs a validity buffer in every batch
            modes = ["null" if pool == "nullrows" else m for m in vm]
            out.append(Case(f"flat-{dt}-{pool}", geom, dt,
                            make_table(dt, pool_values(dt, pool, n, rng), g, modes, rng, fn),
                            pool_of={0: pool}))
        pid = rng.integers(0, NPOOLS - 1, n)
        v = np.zeros(n, dt)
        for p in range(NPOOLS - 1):
            v[pid == p] = pool_values(dt, POOLS[p], int((pid == p).sum()), rng)
        out.append(Case(f"flat-{dt}-mixed", geom, dt, make_table(dt, v, g, vm, rng)))
    out.append(Case("flat-none", geom, None, _none_table(geom, rng)))
    return out


def plant_at(g) -> int:
    """The row at which the planted words of the 1000-row batch start: on a
    bitmap word that opens a wave's trip of four."""
    b = g.index(1000)
    return sum(g[:b]) + (-nwords_of(g[:b]) % 4) * 64


def _key_indices(g, nkeys: int, rng) -> np.ndarray:
    """Group index per row: random, and in the 1000-row batch, within one
    trip of a wave, two one-key words, a third on another key, and a word
    that opens with a stretch of the NaN pool's key among others."""
    n = sum(g)
    k = rng.integers(0, nkeys, n)
    at = plant_at(g)
    k[at:at + 128] = 3 % nkeys
    k[at + 128:at + 192] = 4 % nkeys
    k[at + 192:at + 216] = 5 % nkeys
    return k


def _typed_keys(key_dt: str, idx: np.ndarray, keyvals: list) -> np.ndarray:
    if key_dt == "b1":
        return np.array([bool(keyvals[i]) for i in idx], bool)
    return np.array([keyvals[i] for i in idx], dtype=key_dt)


def malformed_keys(key_dt: str, nslots: int) -> list:
    """Key values outside [0, nslots - 1) that ``key_dt`` can hold: negative
    ones, values >= nslots - 1, uint64 >= 2^63."""
    if key_dt == "b1":
        return [1] if nslots == 2 else []
    info = np.iinfo(key_dt)
    cand = [-1, -77, info.min, nslots - 1, nslots + 5, info.max]
    if key_dt == "u8":
        cand += [1 << 63, (1 << 63) + 12345]
    return sorted({c for c in cand if info.min <= c <= info.max and not 0 <= c < nslots - 1})


def keyed_case(geom: str, key_dt: str, dt: Optional[str], keyvals: list, rng, nslots: int = 0,
               malformed: Optional[list] = None, label: str = "") -> Case:
    """A key column of ``key_dt`` over the groups ``keyvals`` and one value
    column: an integer type, the validity-only column, or a float type whose
    group j draws from pool j % NPOOLS (the null keys' rows from all)."""
    g, vm, km = GEOMETRIES[geom]
    n = sum(g)
    idx = _key_indices(g, len(keyvals), rng)
    kv = _typed_keys(key_dt, idx, keyvals)
    if malformed:
        at = rng.random(n) < 0.04
        at[plant_at(g):][:216] = False                 # the planted words stay whole
        kv[at] = np.array(malformed, kv.dtype)[rng.integers(0, len(malformed), int(at.sum()))]
    key = make_table(key_dt, kv, g, km, rng)
    force, pool_of = None, None
    if dt is None:
        val = _none_table(geom, rng)
    elif dt in FLOATS:
        pool_of = {kv_: POOLS[j % NPOOLS] for j, kv_ in enumerate(keyvals)}
        knull = np.concatenate([np.zeros(b.nrows, bool) if b.valid is None else ~b.valid
                                for b in key.batches])
        pid = np.where(knull, rng.integers(0, NPOOLS, n), idx % NPOOLS)
        # "every row null" needs a validity buffer: elsewhere those rows are small integers
        has_valid = np.concatenate([np.full(c, m is not None) for c, m in zip(g, vm)])
        force = (pid == POOLS.index("nullrows")) & has_valid
        v = np.zeros(n, dt)
        for p in range(NPOOLS):
            v[pid == p] = pool_values(dt, POOLS[p], int((pid == p).sum()), rng)
        val = make_table(dt, v, g, vm, rng, force)
    else:
        val = make_table(dt, int_values(dt, n, rng), g, vm, rng)
    return Case(label or f"{key_dt}-{dt}", geom, dt, val, key, key_dt, nslots, list(keyvals),
                pool_of, nslots - 1 if nslots else None)


def assert_pools(case: Case, groups: Dict[object, Acc], full: bool) -> None:
    """The float groups hold what their pool promises (``full``: the bitmap
    is dense and the groups are few, so every property must show)."""
    if not case.pool_of:
        return
    sub = float(np.finfo(case.dt).tiny)
    big = 1e100 if case.dt == "f8" else 1e20
    for gid, pool in case.pool_of.items():
        acc = groups.get(gid)
        if acc is None:
            assert not full, (case.label, pool)
            continue
        v = acc.vals
        fin = [x for x in v if x == x and abs(x) != math.inf]
        sabs = math.fsum(abs(x) for x in fin)
        assert sabs < 2.0 ** 1000
        if pool == "nullrows":
            # null wherever the batch has a validity buffer
            assert all(x == int(x) for x in v) and (not full or acc.rows > len(v) + 1)
            continue
        assert not full or len(v) > 1, (case.label, pool)
        if pool == "ints":
            assert all(x == int(x) for x in v)
        elif pool == "cancel":
            assert len(fin) == len(v)
            if full:
                assert any(x > big for x in v) and any(x < -big for x in v) and \
                    any(0 < abs(x) < 1 / big for x in v) and abs(math.fsum(v)) < 0.5 * sabs
        elif pool == "subnormal":
            assert all(0 < abs(x) < sub for x in v)
            # float64 subnormals: the bound is below one ulp, the sum must be exact
            assert case.dt == "f4" or len(v) * 2.0 ** -52 * sabs < 5e-324
        elif pool == "inf":
            assert -math.inf not in v and all(x == x for x in v)
            assert not full or (math.inf in v and fin)
        elif pool == "infs":
            assert all(x == x for x in v)
            assert not full or (math.inf in v and -math.inf in v)
        elif pool == "nan":
            assert all(x != x for x in v)
            assert not full or len({_bits(x) for x in v}) == 3
        elif pool == "negzero":
            assert all(_bits(x) == _bits(-0.0) for x in v)
        elif pool == "zeros":
            assert all(x == 0 for x in v)
            assert not full or len({_bits(x) for x in v}) == 2
    if full and case.key is not None:
        # the null keys' rows (with several key columns: a null first component)
        nul = [x for g, a in groups.items()
               if g == case.null_gid or (isinstance(g, tuple) and g[0] is None) for x in a.vals]
        assert any(x != x for x in nul) and any(0 < abs(x) < sub for x in nul) and math.inf in nul


def assert_wraps(dt: str, groups: Dict[object, Acc]) -> None:
    """A 64-bit sum of the case left the type's range: the result wraps."""
    lo, hi = (0, 1 << 64) if dt == "u8" else (-(1 << 63), 1 << 63)
    assert any(not lo <= sum(a.vals) < hi for a in groups.values())


WITNESSES = {"run", "combine", "mine_nan", "flush", "null_batch", "garbage"}


def slots_of(case: Case, groups: Dict[object, Acc]) -> List[Optional[Acc]]:
    """colagg's slots in order (the null keys' last; one slot without key)."""
    return [groups.get(j) for j in range(case.nslots)]


# --------------------------------------------------- colagg's launch rule
def replicas(ops: int, nslots: int) -> int:
    """R of launch_agg: the largest power of two, at most 256, whose
    replicas of the accumulators fit LDS."""
    r = 256
    while r > 1 and A.nacc(ops) * nslots * r * 8 > A.LDS_BYTES:
        r >>= 1
    return r


def reduce_lanes(ops: int, nslots: int) -> int:
    """L of strom_column_agg_reduce: lanes per element."""
    lanes = 64
    while lanes > 1 and A.nacc(ops) * nslots * lanes > 16384:
        lanes >>= 1
    return lanes


# (ops, nslots) -> (R, L): every replica count class and reduce width
REPLICA_CASES = [((15, 3), (256, 64)), ((15, 40), (32, 64)), ((A.COUNT | A.MIN, 700), (4, 8)),
                 ((A.SUM | A.MAX, 2048), (2, 4)), ((15, 2048), (1, 2))]


# ------------------------------------------------------------ group keys
def group_keyvals(key_dt: str) -> list:
    """Ten key values of a hash GROUP BY column: the type's ends (INT64_MIN
    and 2^63 are the free slot's bit pattern), 0, -1 and a few more."""
    info = np.iinfo(key_dt)
    if info.min < 0:
        return [info.min, info.max, 0, -1, 2, 3, 5, 7, 11, 13]
    second = 1 << 63 if key_dt == "u8" else info.max - 1
    return [info.max, second, 0, 1, 2, 3, 5, 7, 11, 13]


def multi_case(geom: str, dt: Optional[str], rng):
    """GROUP BY a nullable int16 and a uint32: (Case whose key is component
    a, component b's table, {group id (a or None, b): group index})."""
    g, vm, km = GEOMETRIES[geom]
    a_vals, b_vals = [-32768, -1, 0, 32767], [0, 7, (1 << 32) - 1]
    combos = [(a, b) for a in a_vals for b in b_vals]
    case = keyed_case(geom, "i2", dt, list(range(len(combos))), rng, label=f"multi-{dt}")
    idx = np.concatenate([np.asarray(b.values) for b in case.key.batches]).astype(np.int64)
    ka = make_table("i2", np.array([combos[i][0] for i in idx], np.int16), g, km, rng)
    # the null pattern of component a as the first table made it
    for nb, ob in zip(ka.batches, case.key.batches):
        nb.valid, nb.vmode = ob.valid, ob.vmode
    kb = make_table("u4", np.array([combos[i][1] for i in idx], np.uint32), g, [None] * len(g), rng)
    case.key, case.keyvals, case.null_gid = ka, combos, None
    case.pool_of = {combos[j]: p for j, p in case.pool_of.items()} if case.pool_of else None
    return case, kb


# -------------------------------------------------------------------- join
def join_reference(bits, fks: List[Q.Table], dims: List[dict], hows: List[int]):
    """Per row: it stays if its bit is set, it exists and every leg agrees —
    a semi leg (0) wants a valid foreign key that is in the leg's dict, an
    anti leg (1) the opposite.  Returns (rows that stay per batch, per leg
    the payload per row or None where the leg did not match)."""
    keep, pays = [], [[] for _ in fks]
    for b in range(len(bits)):
        n = len(bits[b])
        cols = [(_pylist(t, t.batches[b]), t.batches[b].valid) for t in fks]
        kb = np.zeros(n, bool)
        pb = [[None] * n for _ in fks]
        for i in range(n):
            if not bits[b][i]:
                continue
            stay = True
            for leg, ((kv, ok), dim, how) in enumerate(zip(cols, dims, hows)):
                hit = (ok is None or bool(ok[i])) and kv[i] in dim
                if hit:
                    pb[leg][i] = dim[kv[i]]
                if hit == bool(how):
                    stay = False
                    break                # a row a leg dropped is not probed further
            kb[i] = stay
        keep.append(kb)
        for leg in range(len(fks)):
            pays[leg].append(pb[leg])
    return keep, pays


def join_dim(fk_dt: str, leg: int = 0) -> dict:
    """{key: payload} of a dimension table: about half of group_keyvals, the
    free slot's pattern INT64_MIN and keys no foreign key has."""
    kv = group_keyvals(fk_dt)
    keys = [k for k in kv[leg::2] if k < 1 << 63] + [-(1 << 63), 1 << 40, -(1 << 41)]
    keys = list(dict.fromkeys(keys))
    return {k: (7 * i + leg) % 1000 - 3 for i, k in enumerate(keys)}


def join_fk(geom: str, fk_dt: str, rng) -> Q.Table:
    g, _, km = GEOMETRIES[geom]
    kv = group_keyvals(fk_dt)
    return make_table(fk_dt, _typed_keys(fk_dt, _key_indices(g, len(kv), rng), kv), g, km, rng)


# ------------------------------------------------- case lists and checkers
def case_reference(case: Case, bits, keys: Optional[List[Q.Table]] = None, gid_of=None):
    """reference() of a case: colagg's slots unless ``gid_of`` says otherwise."""
    if case.key is None:
        return reference(bits, case.val)
    return reference(bits, case.val, gid_of or slot_gid(case.nslots), keys or [case.key])


def check_block(case: Case, lay, block, ref, what=None) -> None:
    """A colagg block (device or twin) against the reference: the malformed
    keys' counter and every entry, slot by slot."""
    groups, nbad, _ = ref
    block = np.asarray(block).view(np.uint64)
    assert int(block[0]) == nbad, (what, int(block[0]), nbad)
    accs = slots_of(case, groups)
    for e in range(len(lay.entries)):
        check_entry(lay, block, e, accs, what)


def check_groups(keys: list, lay, block, groups: Dict[object, Acc], what=None) -> None:
    """A hash GROUP BY result — ``keys`` the group ids in the order of the
    block's slots, the null keys' slot last — against the reference, key by key."""
    want = [k for k in groups if k is not None]
    assert len(keys) == len(set(keys)) and set(keys) == set(want), (what, keys, want)
    accs = [groups[k] for k in keys] + [groups.get(None)]
    for e in range(len(lay.entries)):
        check_entry(lay, block, e, accs, what)


def keyed_type_cases(geom: str, seed: int = 2) -> List[Case]:
    """colagg with a key: every key type with an int64, a float64 and the
    validity-only column and its malformed keys; every value type under an
    int32 key; a bool key in two slots (value 1 malformed)."""
    rng = np.random.default_rng(seed)
    out = []
    for key_dt in KEY_TYPES:
        nslots = 3 if key_dt == "b1" else 12
        for dt in (VALUE_TYPES + [None]) if key_dt == "i4" else ["i8", "f8", None]:
            out.append(keyed_case(geom, key_dt, dt, list(range(nslots - 1)), rng, nslots,
                                  malformed_keys(key_dt, nslots)))
    out.append(keyed_case(geom, "b1", "i8", [0, 1], rng, 2, [1], label="b1-2slots"))
    return out


def replica_case(ops: int, nslots: int, dt: str, seed: int = 3):
    """(Case, its single entry) of one REPLICA_CASES pair under an int32 key."""
    rng = np.random.default_rng(seed + nslots + ops)
    c = keyed_case("plain", "i4", dt, list(range(nslots - 1)), rng, nslots,
                   malformed_keys("i4", nslots), label=f"R-{ops}-{nslots}-{dt}")
    return c, A.Entry(ops, dt)


BIG_ROWS = [40_000, 0, 30_001]           # 1,094 words: 69 slabs, a lane of the reduce folds two


def big_case(dt: str, seed: int = 4) -> Case:
    rng = np.random.default_rng(seed)
    n = sum(BIG_ROWS)
    v = pool_values(dt, "cancel", n, rng) if dt in FLOATS else int_values(dt, n, rng)
    modes = ["dirty", None, "dirty"]
    bs, at = [], 0
    for c, m in zip(BIG_ROWS, modes):
        bs.append(Q.Batch(c, v[at:at + c], Q.make_valid(c, m, rng), m))
        at += c
    return Case(f"big-{dt}", "big", dt, Q.Table(dt, bs))


def group_cases(geom: str, seed: int = 5) -> List[Case]:
    """Hash GROUP BY: every key type with an int64, a float64 and the
    validity-only column; every value type under an int32 key."""
    rng = np.random.default_rng(seed)
    out = []
    for key_dt in INTS:
        for dt in (VALUE_TYPES + [None]) if key_dt == "i4" else ["i8", "f8", None]:
            out.append(keyed_case(geom, key_dt, dt, group_keyvals(key_dt), rng,
                                  label=f"group-{key_dt}-{dt}"))
    return out


MULTI_SPEC = [("a", "i2", None, True), ("b", "u4", None, False)]     # KeySpec of multi_case


def multi_keys(spec, packed) -> list:
    """Group ids (a or None, b) of the packed keys of a KeySpec(MULTI_SPEC)."""
    vals, oks = spec.unpack(packed)
    return [tuple(int(v[i]) if ok[i] else None for v, ok in zip(vals, oks))
            for i in range(len(packed))]
