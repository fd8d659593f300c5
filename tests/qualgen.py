"""Case generators and a brute-force reference for the column filter,
qualifier and row-emit kernels (csrc/kernels/colfilter.hip).

Tables are built directly, in the layout ArrowScan hands the kernels: one
buffer set per record batch, every batch starting on a fresh bitmap word,
``row_base`` cumulative.  The reference evaluates every row on its own with
Python ints (integers, decimal128), float64 (floats) and ``bytes``
(strings); it shares no code with ``colpred.evaluate``.
"""
from __future__ import annotations

import dataclasses
import math
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from nvme_strom_amd.ops import colpred as CP
from nvme_strom_amd.utils.arrow_ipc import Column, DictEncoding

# rows per batch: one row, both sides of a word, empty batches that share
# their word_base with the next one, several words, more than one trip of kU
GEOMETRY = [1, 63, 64, 65, 0, 257, 1000, 0, 129]
# validity per batch: None absent, "clean" zero bits past nrows, "dirty" every
# bit past nrows set, "null" no valid row (and a dirty tail)
VALIDITY = [None, "dirty", "clean", "dirty", None, "null", "dirty", "clean", None]

INT_TYPES = ["i1", "i2", "i4", "i8", "u1", "u2", "u4", "u8"]
M64 = (1 << 64) - 1


def int_domain(dt: str):
    if dt == "b1":
        return 0, 1
    if dt == "d16":
        return -(1 << 127), (1 << 127) - 1
    bits = 8 * int(dt[1:])
    return (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if dt[0] == "i" else (0, (1 << bits) - 1)


def column(dt: str, name: str = "c") -> Column:
    """The arrow_ipc.Column whose storage type is ``dt`` ("s4"/"s8": utf8
    with 32/64-bit offsets)."""
    if dt == "b1":
        return Column(name, "bool", 1)
    if dt == "d16":
        return Column(name, "decimal", 128, precision=38, scale=0)
    if dt in ("s4", "s8"):
        return Column(name, "binary", nbuffers=3, large=dt == "s8")
    if dt[0] == "f":
        return Column(name, "float", 8 * int(dt[1:]))
    return Column(name, "int", 8 * int(dt[1:]), dt[0] == "i")


# ------------------------------------------------------------------ tables
@dataclass
class Batch:
    nrows: int
    values: object                      # ndarray / list of ints (d16) / (offsets, chars)
    valid: Optional[np.ndarray]         # bool[nrows] or None
    vmode: Optional[str] = None


@dataclass
class Table:
    dt: str
    batches: List[Batch]
    row0: int = 0                       # row_base of the first batch
    word_base: List[int] = field(default_factory=list)
    row_base: List[int] = field(default_factory=list)
    nwords: int = 0

    def __post_init__(self):
        w, r = 0, self.row0
        for b in self.batches:
            self.word_base.append(w)
            self.row_base.append(r)
            w += (b.nrows + 63) // 64
            r += b.nrows
        self.nwords = w

    @property
    def nrows(self):
        return sum(b.nrows for b in self.batches)


def make_valid(n: int, mode: Optional[str], rng) -> Optional[np.ndarray]:
    if mode is None:
        return None
    if mode == "null":
        return np.zeros(n, bool)
    return rng.random(n) < 0.85


def valid_words(b: Batch) -> Optional[np.ndarray]:
    """The validity buffer of a batch as whole uint64 words."""
    if b.valid is None:
        return None
    nw = max((b.nrows + 63) // 64, 1)
    bits = np.zeros(nw * 64, bool)
    bits[:b.nrows] = b.valid
    if b.vmode in ("dirty", "null"):
        bits[b.nrows:] = True
    return np.packbits(bits, bitorder="little").view(np.uint64)


def table(dt: str, values, rng, geometry=GEOMETRY, validity=VALIDITY, row0: int = 0) -> Table:
    """Split ``values`` (one per row, sum(geometry) of them) over the batches."""
    bs, at = [], 0
    for n, mode in zip(geometry, validity):
        bs.append(Batch(n, values[at:at + n], make_valid(n, mode, rng), mode))
        at += n
    assert at == len(values)
    return Table(dt, bs, row0)


def _pad8(raw: bytes) -> np.ndarray:
    raw = raw + b"\0" * (-len(raw) % 8 or (8 if not raw else 0))
    return np.frombuffer(raw, np.uint8)


def values_bytes(dt: str, b: Batch) -> bytes:
    if dt == "b1":
        return np.packbits(np.asarray(b.values, bool), bitorder="little").tobytes()
    if dt == "d16":
        return b"".join(int(x).to_bytes(16, "little", signed=True) for x in b.values)
    if dt in ("s4", "s8"):
        return np.asarray(b.values[0], "<i4" if dt == "s4" else "<i8").tobytes()
    return np.ascontiguousarray(b.values).tobytes()


class DeviceTable:
    """The batches' buffers on the device and the two batch tables over
    them: ``qtab`` (n, 7) strom_qual_batch, ``ftab`` (n, 5)
    strom_filter_batch."""

    def __init__(self, t: Table, dev, with_values: bool = True):
        import torch
        self.keep, rows = [], []
        for k, b in enumerate(t.batches):
            vp = ap = alen = valp = 0
            if with_values:
                v = torch.from_numpy(_pad8(values_bytes(t.dt, b)).copy()).to(dev)
                self.keep.append(v)
                vp = v.data_ptr()
                if t.dt in ("s4", "s8"):
                    chars = np.asarray(b.values[1], np.uint8)
                    a = torch.from_numpy(_pad8(chars.tobytes()).copy()).to(dev)
                    self.keep.append(a)
                    ap, alen = a.data_ptr(), len(chars)
            vw = valid_words(b)
            if vw is not None:
                vt = torch.from_numpy(vw.view(np.int64).copy()).to(dev)
                self.keep.append(vt)
                valp = vt.data_ptr()
            rows.append([vp, valp, b.nrows, t.word_base[k], t.row_base[k], ap, alen])
        arr = np.array(rows, dtype=np.uint64).view(np.int64).reshape(-1, 7)
        self.qtab = torch.from_numpy(arr.copy()).to(dev)
        self.ftab = torch.from_numpy(arr[:, :5].copy()).to(dev)
        self.nwords = t.nwords


# --------------------------------------------------------------- reference
def row_bytes(b: Batch, i: int) -> Optional[bytes]:
    """Row i of a string batch; None for a malformed offset pair."""
    offs, chars = b.values
    a, e = int(offs[i]), int(offs[i + 1])
    if a < 0 or e < a or e > len(chars):
        return None
    return bytes(chars[a:e])


def _str_bound_ok(x: bytes, bound, mode: int, upper: bool) -> bool:
    if not mode:
        return True
    if upper:
        return x <= bound if mode == 1 else x < bound
    return x >= bound if mode == 1 else x > bound


def brute(t: Table, ref: dict) -> List[np.ndarray]:
    """Per batch: bool[nrows], the rows the predicate ``ref`` selects
    (nulls cleared).  ``ref``: kind "ranges" (ranges, nan, neg), "lut"
    (bits), "str_in" / "str_prefix" (consts, neg), "str_ranges" (ranges of
    (lo, lo_mode, hi, hi_mode), neg), "valid" (neg)."""
    kind, neg = ref["kind"], bool(ref.get("neg"))
    out = []
    for b in t.batches:
        ok = np.ones(b.nrows, bool) if b.valid is None else b.valid.copy()
        if kind == "valid":
            out.append(~ok if neg else ok)
            continue
        hit = np.zeros(b.nrows, bool)
        for i in range(b.nrows):
            if kind == "ranges":
                x = b.values[i]
                if t.dt[0] == "f":
                    x = np.float64(x)
                    h = any(lo <= x <= hi for lo, hi in ref["ranges"]) or \
                        (bool(ref.get("nan")) and math.isnan(x))
                else:
                    x = int(x)
                    h = any(lo <= x <= hi for lo, hi in ref["ranges"])
            elif kind == "lut":
                x, bits = int(b.values[i]), ref["bits"]
                h = 0 <= x < len(bits) and bool(bits[x])
            else:
                x = row_bytes(b, i)
                if x is None:               # malformed: selected by nothing
                    ok[i] = False
                    continue
                if kind == "str_in":
                    h = any(x == c for c in ref["consts"])
                elif kind == "str_prefix":
                    h = any(x[:len(c)] == c and len(x) >= len(c) for c in ref["consts"])
                else:
                    h = any(_str_bound_ok(x, lo, lm, False) and _str_bound_ok(x, hi, hm, True)
                            for lo, lm, hi, hm in ref["ranges"])
            hit[i] = h != neg
        out.append(hit & ok)
    return out


def pack_words(t: Table, bits: List[np.ndarray]) -> np.ndarray:
    """Per-batch row bits as the scan's bitmap words (zeros past nrows)."""
    w = np.zeros(t.nwords, np.uint64)
    for k, (b, h) in enumerate(zip(t.batches, bits)):
        nw = (b.nrows + 63) // 64
        if nw:
            full = np.zeros(nw * 64, bool)
            full[:b.nrows] = h
            w[t.word_base[k]:t.word_base[k] + nw] = np.packbits(full, bitorder="little").view(np.uint64)
    return w


def expected_words(pred: np.ndarray, or_src, and_dst: bool, old: np.ndarray) -> np.ndarray:
    w = pred.copy()
    if or_src is not None:
        w |= or_src
    if and_dst:
        w &= old
    return w


def popcount(words: np.ndarray) -> int:
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


def host_values(t: Table, b: Batch):
    """The batch's values in the form colpred.evaluate takes."""
    if t.dt == "d16":
        return np.array([int(x) for x in b.values], dtype=object)
    if t.dt == "b1":
        return np.asarray(b.values, bool)
    if t.dt in ("s4", "s8"):
        return np.asarray(b.values[0], np.int64), np.asarray(b.values[1], np.uint8)
    return np.asarray(b.values)


# ------------------------------------------------------------------- cases
@dataclass
class Case:
    name: str
    table: Table
    compiled: CP.Compiled
    ref: dict


def with_flags(c: CP.Compiled, flags: int) -> CP.Compiled:
    return dataclasses.replace(c, flags=flags, _dev={})


def int_ranges(dt: str, n: int, rng) -> List[tuple]:
    """n disjoint, non-adjacent inclusive ranges spread over the whole
    domain of ``dt`` (Python ints)."""
    tmin, tmax = int_domain(dt)
    step = (tmax - tmin - 2) // n
    assert step >= 3
    rs = []
    for k in range(n):
        lo = tmin + 1 + k * step
        width = int(rng.integers(0, min(step - 2, 1 << 40) + 1)) if k % 3 else 0
        rs.append((lo, lo + width))
    return rs


def range_values(rs, nrows: int, rng, lo_lim, hi_lim, step, rand) -> list:
    """nrows values around ``rs``: both endpoints of ranges and the values
    just outside them (first, a middle and the last range always), below the
    first range and above the last, the domain's ends, then random ones."""
    def near(r):
        return [r[0], r[1], step(r[0], -1), step(r[1], +1), step(r[0], +1), step(r[1], -1)]
    must = near(rs[0]) + near(rs[len(rs) // 2]) + near(rs[-1])
    must += [step(step(rs[0][0], -1), -1), step(step(rs[-1][1], +1), +1), lo_lim, hi_lim]
    rest = [v for r in rs for v in near(r)]
    rest = [rest[i] for i in rng.permutation(len(rest))]
    vals = [v for v in must + rest if lo_lim <= v <= hi_lim][:max(nrows - nrows // 4, len(must))]
    vals = vals[:nrows]
    vals += [rand() for _ in range(nrows - len(vals))]
    return [vals[i] for i in rng.permutation(nrows)]


def np_values(dt: str, vals):
    if dt == "d16":
        return list(vals)
    if dt == "b1":
        return np.asarray(vals, bool)
    return np.array(vals, dtype=np.dtype(dt))


def int_ranges_compiled(dt: str, rs, flags: int = 0) -> CP.Compiled:
    """Hand-built range operands in the int64 compare domain (ranges past
    the column's own type, which compile_pred would clip away)."""
    arr = np.asarray(rs, dtype=np.int64).reshape(-1, 2)
    return CP.Compiled(CP.COL_CODE[dt], CP.QOP_RANGES, flags, len(rs), arr.tobytes(), ranges=arr)


def int_range_case(dt: str, n: int, rng, neg: bool = False, wide: bool = False) -> Case:
    """``wide``: the ranges spread over the 16-bit domain of the same
    signedness (an 8-bit type has no room for 1000 disjoint ranges)."""
    rs = int_ranges(dt[0] + "2" if wide else dt, n, rng)
    tmin, tmax = int_domain(dt)
    nrows = sum(GEOMETRY)
    span = tmax - tmin + 1

    def rand():
        return tmin + int(rng.integers(0, 1 << 62)) * int(rng.integers(1, 1 << 62)) % span
    vals = range_values(rs, nrows, rng, tmin, tmax, lambda v, d: v + d, rand)
    t = table(dt, np_values(dt, vals), rng)
    if wide:
        c = int_ranges_compiled(dt, rs)
    else:
        c = CP.compile_pred(CP.Pred("c", "ranges", tuple(rs)), column(dt))
    assert c.nconst == n
    if neg:
        c = with_flags(c, c.flags | CP.FLAG_NEGATE)
    return Case(f"{dt}-{n}{'-neg' if neg else ''}", t, c, dict(kind="ranges", ranges=rs, neg=neg))


def float_range_case(dt: str, n: int, rng, inf_ends: bool, nan: bool, neg: bool) -> Case:
    f = np.dtype(dt).type
    pts = np.sort(rng.choice(np.arange(-4000, 4000), 2 * n, replace=False)).astype(np.float64) / 4
    rs = [(float(pts[2 * k]), float(pts[2 * k + 1] if k % 3 else pts[2 * k])) for k in range(n)]
    if inf_ends:
        rs[0] = (-math.inf, rs[0][1])
        rs[-1] = (rs[-1][0], math.inf)
    if n == 1 and not inf_ends:
        rs = [(-0.0, 0.1)]                       # f32: 0.1f > 0.1 stays out; -0.0 == 0.0 is in
    nrows = sum(GEOMETRY)

    def step(v, d):                               # the neighbour in the column's own type
        return float(np.nextafter(f(v), f(d * math.inf)))
    vals = range_values(rs, nrows, rng, -math.inf, math.inf, step,
                        lambda: float(f(rng.normal() * 600)))
    special = [math.nan, math.inf, -math.inf, -0.0, 0.0, float(np.float32(0.1)), 0.1,
               float(np.finfo(f).max), float(np.finfo(f).tiny)]
    for k, s in enumerate(special * 3):
        vals[(k * 37 + 5) % nrows] = s
    t = table(dt, np.array(vals, dtype=f), rng)
    c = CP.compile_pred(CP.Pred("c", "ranges", tuple(rs)), column(dt))
    assert c.nconst == len(rs)
    flags = (CP.FLAG_NAN if nan else 0) | (CP.FLAG_NEGATE if neg else 0)
    c = with_flags(c, flags)
    name = f"{dt}-{n}{'-inf' if inf_ends else ''}{'-nan' if nan else ''}{'-neg' if neg else ''}"
    return Case(name, t, c, dict(kind="ranges", ranges=rs, nan=nan, neg=neg))


def bool_cases(rng) -> List[Case]:
    out = []
    for op, v, rs, neg in [("==", True, [(1, 1)], False), ("==", False, [(0, 0)], False),
                           ("!=", True, [(1, 1)], True), ("in", (False, True), [(0, 1)], False)]:
        t = table("b1", rng.random(sum(GEOMETRY)) < 0.4, rng)
        c = CP.compile_pred(CP.Pred("c", op, v), column("b1"))
        out.append(Case(f"b1-{op}-{v}", t, c, dict(kind="ranges", ranges=rs, neg=neg)))
    return out


def dec128_ranges_compiled(rs, flags: int = 0) -> CP.Compiled:
    """Hand-built operands of 128-bit ranges (bounds to the ends of int128)."""
    blob = b"".join(int(x).to_bytes(16, "little", signed=True) for r in rs for x in r)
    return CP.Compiled(CP.COL_CODE["d16"], CP.QOP_RANGES, flags, len(rs), blob,
                       ranges=np.array(rs, dtype=object).reshape(-1, 2))


def dec128_cases(rng) -> List[Case]:
    out = []
    for n in (1, 8, 9, 17):
        for neg in (False, True):
            case = int_range_case("d16", n, rng, neg)
            out.append(case)
    # bounds at the very ends of int128, operands by hand
    tmin, tmax = int_domain("d16")
    rs = [(tmin, tmin + 5), (-(1 << 64) - 3, -(1 << 64) + 3), (-2, 2), ((1 << 64) - 3, (1 << 64) + 3),
          ((1 << 100), (1 << 100) + (1 << 70)), (tmax - 6, tmax)]
    nrows = sum(GEOMETRY)
    vals = range_values(rs, nrows, rng, tmin, tmax, lambda v, d: v + d,
                        lambda: int(rng.integers(-1 << 62, 1 << 62)) << int(rng.integers(0, 65)))
    t = table("d16", vals, rng)
    out.append(Case("d16-ends", t, dec128_ranges_compiled(rs), dict(kind="ranges", ranges=rs)))
    return out


def numeric_cases(dt: str, rng) -> List[Case]:
    if dt == "b1":
        return bool_cases(rng)
    if dt == "d16":
        return dec128_cases(rng)
    if dt[0] == "f":
        out = [float_range_case(dt, 1, rng, False, False, False)]
        for n in (1, 8, 9, 17, 1000):
            for inf_ends, nan, neg in [(True, False, False), (False, True, True), (True, True, False),
                                       (False, False, True)]:
                if n in (17, 1000) and (nan != neg):
                    continue                  # the large lists: two variants each
                out.append(float_range_case(dt, n, rng, inf_ends, nan, neg))
        return out
    out = [int_range_case(dt, n, rng, wide=dt[1] == "1" and n == 1000) for n in (1, 8, 9, 17, 1000)]
    out.append(int_range_case(dt, 9, rng, neg=True))
    return out


def u64_high_case(rng) -> Case:
    """Values and bounds >= 2^63: the uint64 compare domain."""
    rs = [((1 << 63) - 2, (1 << 63) + 2), ((1 << 63) + 100, (1 << 63) + 100),
          ((1 << 64) - 4, (1 << 64) - 1)] + [((1 << 63) + 1000 * k, (1 << 63) + 1000 * k + k)
                                             for k in range(1, 9)]
    rs.sort()
    nrows = sum(GEOMETRY)
    vals = range_values(rs, nrows, rng, 0, M64, lambda v, d: v + d,
                        lambda: (1 << 63) + int(rng.integers(0, 10000)))
    t = table("u8", np.array(vals, dtype=np.uint64), rng)
    c = CP.compile_pred(CP.Pred("c", "ranges", tuple(rs)), column("u8"))
    assert c.nconst == len(rs)
    return Case("u8-high", t, c, dict(kind="ranges", ranges=rs))


def in_list_case(dt: str, n: int, rng, neg: bool) -> Case:
    """An IN-list of n non-adjacent values: n single-point ranges."""
    tmin, tmax = int_domain(dt)
    vals_in = [tmin + 2 + 5 * k for k in range(n)]
    nrows = sum(GEOMETRY)
    vals = [vals_in[int(rng.integers(n))] + int(rng.integers(-1, 2)) for _ in range(nrows)]
    t = table(dt, np_values(dt, vals), rng)
    c = CP.compile_pred(CP.Pred("c", "not in" if neg else "in", tuple(vals_in)), column(dt))
    assert c.nconst == n
    return Case(f"{dt}-in{n}{'-neg' if neg else ''}", t, c,
                dict(kind="ranges", ranges=[(v, v) for v in vals_in], neg=neg))


# ---- LUT
LUT_INDEX_TYPES = ["i1", "i2", "i4", "u1", "u2"]
LUT_SIZES = [1, 31, 32, 33, CP.MAX_LUT_BITS]


def lut_case(dt: str, nconst: int, rng) -> Case:
    """A dictionary-encoded int64 column with indices of type ``dt``: the
    predicate is evaluated on the dictionary by compile_pred and reaches the
    kernel as a lookup table."""
    col = Column("c", "int", 64, dictionary=DictEncoding(1, 8 * int(dt[1:]), dt[0] == "i"))
    dvals = np.arange(nconst, dtype=np.int64) * 3
    top = 3 * (nconst - 1)
    pts = np.sort(rng.integers(0, top + 1, 40))
    rs = [(0, 0), (top, top)] + [(int(pts[2 * k]), int(pts[2 * k + 1])) for k in range(20)]
    bits = np.zeros(nconst, bool)
    for lo, hi in rs:
        bits |= (dvals >= lo) & (dvals <= hi)
    c = CP.compile_pred(CP.Pred("c", "ranges", tuple(rs)), col, dictionary=(dvals, None))
    assert c.op == CP.QOP_LUT and c.nconst == nconst
    tmin, tmax = int_domain(dt)
    nrows = sum(GEOMETRY)
    special = [-1, tmin, 0, nconst - 1, nconst, nconst + 1, nconst + 31, nconst + 32, tmax, tmax - 1,
               nconst - 2, 31, 32, 33]
    special = [v for v in special if tmin <= v <= tmax]
    hi = min(nconst + 40, tmax + 1)
    vals = [int(rng.integers(max(tmin, -3), hi)) for _ in range(nrows)]
    for k, s in enumerate(special * 4):
        vals[(k * 29 + 3) % nrows] = s
    t = table(dt, np.array(vals, dtype=np.dtype(dt)), rng)
    return Case(f"lut-{dt}-{nconst}", t, c, dict(kind="lut", bits=bits))


# ---- strings
STR_LENGTHS = list(range(10)) + [15, 16, 17, 40]
# the master string: every constant and most rows are cut from it, so rows are
# proper prefixes of constants and the reverse; bytes >= 0x80 order unsigned
MASTER = bytes([0x61, 0xC3, 0xA9, 0x7A, 0x80, 0xFF, 0x41, 0x00, 0x7F, 0xE2, 0x82, 0xAC, 0x62, 0xFE,
                0x01, 0x81, 0x63, 0x20, 0xF0, 0x9F, 0x98, 0x80, 0x64, 0x90, 0x7E, 0xAA, 0x55, 0x65,
                0xBB, 0x10, 0xCC, 0x66, 0xDD, 0x30, 0xEE, 0x67, 0x8F, 0x40, 0x9E, 0x68])
assert len(MASTER) == 40


def str_rows(rng) -> List[bytes]:
    rows = []
    for L in STR_LENGTHS:
        rows.append(MASTER[:L])
        if L:
            rows.append(MASTER[:L - 1] + bytes([MASTER[L - 1] ^ 0x80]))   # last byte differs
            rows.append(MASTER[:L - 1] + bytes([(MASTER[L - 1] + 1) & 0xFF]))
            rows.append(bytes(rng.integers(0, 256, L, dtype=np.uint8)))
            rows.append(bytes([MASTER[0] ^ 0x80]) + MASTER[1:L])           # first byte differs
    return rows


def str_table(dt: str, rng, malformed: bool = False, row0: int = 0) -> Table:
    """Every row of str_rows() at every start alignment 0-3 of the character
    buffer (a filler row before it sets the alignment), over three batches
    with their own offsets and characters.  ``malformed``: three offsets of
    the second and third batch are replaced by a negative one, one past the
    characters and one below its predecessor; the buffers stay as they are."""
    rows = str_rows(rng)
    order = [(r, a) for a in range(4) for r in rows]
    order = [order[i] for i in rng.permutation(len(order))]
    cut = [0, len(order) // 5, len(order) // 2, len(order)]
    batches = []
    for k in range(3):
        offs, chars = [0], bytearray()
        for r, a in order[cut[k]:cut[k + 1]]:
            chars += bytes(rng.integers(0x80, 0x100, (a - len(chars)) % 4, dtype=np.uint8))
            offs.append(len(chars))                                   # the filler row
            assert len(chars) % 4 == a
            chars += r
            offs.append(len(chars))
        offs = np.array(offs, np.int64)
        if malformed and k:
            n = len(offs) - 1
            offs[n // 4] = -3
            offs[n // 2] = len(chars) + (64 if dt == "s4" else (1 << 33) + 5)
            offs[3 * n // 4] = offs[3 * n // 4 - 1] - 1
        n = len(offs) - 1
        mode = [None, "dirty", "clean"][k]
        batches.append(Batch(n, (offs, np.frombuffer(bytes(chars), np.uint8)),
                             make_valid(n, mode, rng), mode))
    batches.insert(1, Batch(0, (np.zeros(1, np.int64), np.zeros(0, np.uint8)), None))
    return Table(dt, batches, row0)


def str_ranges_compiled(dt: str, rs, flags: int = 0) -> CP.Compiled:
    """Hand-built string-range operands (exclusive bounds on both sides are
    not reachable through a Pred)."""
    blob, offs = bytearray(), []
    for lo, lm, hi, hm in rs:
        for b, m in ((lo, lm), (hi, hm)):
            b = b or b""
            offs += [len(blob), len(b), m]
            blob += b + b"\0" * (-len(b) % 4)
    return CP.Compiled(CP.COL_STR64 if dt == "s8" else CP.COL_STR32, CP.QOP_STR_RANGES, flags,
                       len(rs), bytes(blob) or b"\0\0\0\0", np.asarray(offs, np.uint32).tobytes(),
                       strings=list(rs))


def str_preds(rng):
    """(name, Pred or hand-built ranges, ref)."""
    M = MASTER
    in40 = sorted({M[:L] for L in STR_LENGTHS} | {M[:L - 1] + bytes([M[L - 1] ^ 0x80])
                                                  for L in (1, 4, 5, 8, 16, 17)} |
                  {bytes(rng.integers(0, 256, int(L), dtype=np.uint8))
                   for L in rng.integers(1, 20, 40)})[:40]
    assert len(in40) == 40 and b"" in in40
    out = []
    for name, consts in [("eq17", [M[:17]]), ("eq-empty", [b""]), ("eq3", [M[:3]]), ("in40", in40)]:
        for neg in (False, True):
            op = ("!=" if neg else "==") if len(consts) == 1 else ("not in" if neg else "in")
            v = consts[0] if len(consts) == 1 else tuple(consts)
            out.append((name + "-neg" * neg, CP.Pred("c", op, v),
                        dict(kind="str_in", consts=consts, neg=neg)))
    for name, consts in [("pre5", [M[:5]]), ("pre-list", [M[:16], M[:2] + b"\x00", b"\xff", M[:7]]),
                         ("pre-empty", [b""])]:
        for neg in (False, True):
            out.append((name + "-neg" * neg,
                        CP.Pred("c", "not prefix" if neg else "prefix",
                                consts[0] if len(consts) == 1 else list(consts)),
                        dict(kind="str_prefix", consts=consts, neg=neg)))
    for name, op, v, r in [("lt", "<", M[:8], (None, 0, M[:8], 2)),
                           ("le", "<=", M[:8], (None, 0, M[:8], 1)),
                           ("gt", ">", M[:5], (M[:5], 2, None, 0)),
                           ("ge", ">=", M[:5], (M[:5], 1, None, 0)),
                           ("ge-empty", ">=", b"", (b"", 1, None, 0)),
                           ("gt-empty", ">", b"", (b"", 2, None, 0)),
                           ("between", "between", (M[:4], M[:17]), (M[:4], 1, M[:17], 1))]:
        out.append((name, CP.Pred("c", op, v), dict(kind="str_ranges", ranges=[r])))
    multi = [(b"", b"\x00"), (M[:1], M[:3]), (M[:4], M[:4]), (M[:6], M[:15]), (M[:16] + b"\x00", M[:17]),
             (b"\x80", b"\xc0\xff"), (b"\xff", b"\xff\xff\xff\xff\xff")]
    out.append(("ranges7", CP.Pred("c", "ranges", tuple(multi)),
                dict(kind="str_ranges", ranges=[(a, 1, b, 1) for a, b in multi])))
    hand = [(M[:4], 2, M[:9], 2), (M[:15], 2, M[:16], 1), (b"\x90", 1, None, 0)]
    out.append(("excl", hand, dict(kind="str_ranges", ranges=hand)))
    out.append(("excl-neg", hand, dict(kind="str_ranges", ranges=hand, neg=True)))
    out.append(("is_valid", CP.Pred("c", "is_valid"), dict(kind="valid")))
    out.append(("is_null", CP.Pred("c", "is_null"), dict(kind="valid", neg=True)))
    return out


def str_cases(dt: str, rng, malformed: bool) -> List[Case]:
    t = str_table(dt, rng, malformed)
    out = []
    for name, p, ref in str_preds(rng):
        if isinstance(p, list):
            c = str_ranges_compiled(dt, p, CP.FLAG_NEGATE if ref.get("neg") else 0)
        else:
            c = CP.compile_pred(p, column(dt))
        out.append(Case(f"{dt}-{name}{'-bad' if malformed else ''}", t, c, ref))
    return out


# ---- limits: the largest operands compile_pred accepts
def limit_cases(rng) -> List[Case]:
    out = []
    n = CP.MAX_RANGES
    rs = [(-(1 << 62) + (1 << 50) * k, -(1 << 62) + (1 << 50) * k + (k % 7)) for k in range(n)]
    nrows = sum(GEOMETRY)
    vals = range_values(rs, nrows, rng, *int_domain("i8"), lambda v, d: v + d,
                        lambda: int(rng.integers(-1 << 62, 1 << 62)))
    c = CP.compile_pred(CP.Pred("c", "ranges", tuple(rs)), column("i8"))
    assert c.nconst == n and len(c.consts) == CP.MAX_QUAL_BYTES
    out.append(Case("limit-i8-ranges", table("i8", np.array(vals, np.int64), rng), c,
                    dict(kind="ranges", ranges=rs)))
    case = lut_case("i4", CP.MAX_LUT_BITS, rng)
    assert len(case.compiled.consts) == CP.MAX_QUAL_BYTES
    out.append(dataclasses.replace(case, name="limit-lut"))
    # string IN-list: 4096 constants of 8 bytes, 32 KiB of blob + 32 KiB of (start, len)
    consts = [b"k%07d" % (7 * k) for k in range(CP.MAX_RANGES)]
    rows = [b"k%07d" % int(x) for x in rng.integers(0, 7 * CP.MAX_RANGES, 300)] + consts[:3] + \
        consts[-3:] + [b"", b"k", consts[5][:7], consts[5] + b"0"]
    offs = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    chars = np.frombuffer(b"".join(rows), np.uint8)
    geo = [100, 0, len(rows) - 100]
    bs, at = [], 0
    for g, mode in zip(geo, [None, None, "dirty"]):
        o = offs[at:at + g + 1]
        bs.append(Batch(g, (o - o[0], chars[o[0]:o[-1]]), make_valid(g, mode, rng), mode))
        at += g
    c = CP.compile_pred(CP.Pred("c", "in", tuple(consts)), column("s4"))
    assert c.nconst == CP.MAX_RANGES and len(c.consts) + len(c.offs) == CP.MAX_QUAL_BYTES
    out.append(Case("limit-str-in", Table("s4", bs), c, dict(kind="str_in", consts=consts)))
    return out


# ---- range filter
INT_BOUNDS = [(-math.inf, math.inf), (-math.inf, 5.0), (-3.0, math.inf), (math.inf, math.inf),
              (-math.inf, -math.inf), (math.inf, -math.inf),
              (0.5, -0.5), (-0.5, 0.5), (2.5, 7.5), (math.nan, 5.0), (-5.0, math.nan),
              (math.nan, math.nan), (7.0, 2.0), (-100.0, 250.0), (3.0, 3.0), (2.5, 2.75)]
TYPE_BOUNDS = {
    "i4": INT_BOUNDS + [(-1e10, 1e10), (0.0, 1e10), (-1e10, 0.0), (1e10, 2e10), (-2e10, -1e10),
                        (-2147483648.0, -2147483648.0), (2147483647.0, 2147483647.5),
                        (2147483647.5, 3e9), (-2147483648.5, -2147483647.5)],
    "i8": INT_BOUNDS + [(-1e19, 1e19), (0.0, 1e19), (-1e19, 0.0), (1e19, 2e19), (-2e19, -1e19),
                        (-1e10, 1e10), (2.0 ** 63, 2.0 ** 63), (-2.0 ** 63, -2.0 ** 63),
                        (2.0 ** 62, 2.0 ** 63), (2.0 ** 53, 2.0 ** 53 + 2)],
    "f4": [(0.1, math.inf), (-math.inf, 0.1), (0.1, 0.1), (float(np.float32(0.1)), 1.0),
           (2.0 ** 24 + 1, math.inf), (-math.inf, 2.0 ** 24 + 1), (2.0 ** 24, 2.0 ** 24 + 1),
           (2.0 ** 24 + 1, 2.0 ** 24 + 1), (-math.inf, math.inf), (math.nan, 1.0), (1.0, math.nan),
           (1e39, math.inf), (-math.inf, -1e39), (3.5e38, 1e39), (-0.0, 0.0), (1e-46, 1.0),
           (-1.0, -1e-46), (7.0, 2.0), (-100.0, 250.0)],
    "f8": [(0.1, math.inf), (-math.inf, 0.1), (0.1, 0.1), (-math.inf, math.inf), (math.nan, 1.0),
           (1.0, math.nan), (7.0, 2.0), (-0.0, 0.0), (-100.0, 250.0)],
}


def filter_values(dt: str, nrows: int, rng) -> np.ndarray:
    if dt[0] == "i":
        tmin, tmax = int_domain(dt)
        base = [0, 1, -1, 2, 3, 7, 8, -100, -101, 250, 251, tmin, tmin + 1, tmax, tmax - 1,
                5, 6, -3, -4, 1 << 30]
        if dt == "i8":
            base += [10 ** 10, 10 ** 10 + 1, -10 ** 10, -10 ** 10 - 1, 1 << 62, (1 << 62) - 1,
                     1 << 53, (1 << 53) + 1, (1 << 53) + 2, (1 << 53) + 3]
        vals = base + [int(x) for x in rng.integers(-300, 300, max(nrows - len(base), 0))]
    else:
        f = np.dtype(dt).type
        base = [np.float32(0.1), 0.1, np.nextafter(np.float32(0.1), np.float32(0)), 2.0 ** 24,
                2.0 ** 24 + 2, 2.0 ** 24 - 1, math.nan, math.inf, -math.inf, 0.0, -0.0,
                np.finfo(f).max, -np.finfo(f).max, np.finfo(f).smallest_subnormal,
                -np.finfo(f).smallest_subnormal, 1.0, -1.0, 250.0, -100.0]
        vals = [float(x) for x in base] + list(rng.normal(size=max(nrows - len(base), 0)) * 200)
    vals = vals[:nrows]
    return np.array([vals[i] for i in rng.permutation(nrows)], dtype=np.dtype(dt))


def brute_filter(t: Table, lo: float, hi: float) -> List[np.ndarray]:
    """lo <= v <= hi with the double bounds, exactly: Python compares an int
    with a float without rounding, floats are widened to float64."""
    out = []
    for b in t.batches:
        ok = np.ones(b.nrows, bool) if b.valid is None else b.valid
        if t.dt[0] == "i":
            hit = np.array([lo <= int(x) <= hi for x in b.values], bool).reshape(b.nrows)
        else:
            hit = np.array([lo <= float(x) <= hi for x in b.values], bool).reshape(b.nrows)
        out.append(hit & ok)
    return out


def bounds_reference(dt: str, lo: float, hi: float):
    """(lo, hi) in the column's type as strom_filter_bounds defines them, or
    None for an empty range."""
    if math.isnan(lo) or math.isnan(hi) or lo > hi:
        return None
    if dt[0] == "i":
        tmin, tmax = int_domain(dt)
        l = tmin if lo == -math.inf else (tmax + 1 if lo == math.inf else math.ceil(lo))
        h = tmax if hi == math.inf else (tmin - 1 if hi == -math.inf else math.floor(hi))
        l, h = max(l, tmin), min(h, tmax)
        return (l, h) if l <= h else None
    f = np.dtype(dt).type
    with np.errstate(over="ignore"):
        l, h = f(lo), f(hi)
    if float(l) < lo:
        l = np.nextafter(l, f(math.inf))
    if float(h) > hi:
        h = np.nextafter(h, f(-math.inf))
    return (l, h) if l <= h else None


# ---- row emit
def emit_reference(t: Table, bits: List[np.ndarray]):
    """Global row ids of the set bits, batch by batch (numpy.nonzero +
    row_base), and per batch the selected local rows."""
    sel = [np.nonzero(h)[0] for h in bits]
    ids = np.concatenate([s + t.row_base[k] for k, s in enumerate(sel)]).astype(np.int64)
    return ids, sel
