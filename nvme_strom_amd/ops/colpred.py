"""Arrow scan predicates: the forms a query writes, their compilation to the
operands of the GPU qualifier kernel (csrc/kernels/colfilter.hip,
``strom_column_qual``), and a numpy twin of that kernel.

A qualifier list is a conjunction (CNF): each item is one predicate or an
``Or`` of predicates (on any columns).  Predicates:

    (name, lo, hi)                      lo <= v <= hi (the round-1 form)
    (name, op, value)  /  P(name) <op> value
        "==" "!=" "<" "<=" ">" ">="     numeric, bool, date/time/timestamp/duration,
                                        utf8/binary (bytewise, as pyarrow)
        "between" (lo, hi)              inclusive
        "in" / "not in" [values]        IN-lists (numbers, strings, dates ...)
        "ranges" [(lo, hi), ...]        an OR of inclusive ranges on one column
        "prefix" / "not prefix" s       utf8/binary starts-with (a list: any of)
        "suffix" / "not suffix" s       ... ends-with (a list: any of)
        "contains" / "not contains" s   ... holds s somewhere (a list: any of)
        "like" / "not like" pattern     SQL LIKE, see below
    (name, "is_null") / (name, "is_valid")

Nulls never satisfy a comparison (SQL: a NULL comparison is not true, and
NOT of it is not true either), so every predicate's bits are ANDed with the
row's validity; ``Or`` of a NULL and a true predicate is true.  Floats
follow pyarrow.compute: NaN compares false (so ``!=`` selects it) and
``in`` matches NaN to a NaN in the list.  Integers compare exactly (bounds
in the column's own integer domain: ``v < 2.5`` is ``v <= 2``), floats in
double (pyarrow promotes float32 against a Python float the same way).

LIKE follows pyarrow.compute.match_like: ``%`` matches any run of
characters (the empty one too), ``_`` exactly one character, a code point on
a utf8 column and a byte on a binary one, newlines included; ``\\`` escapes
``%``, ``_`` and itself, and before anything else (or at the end) it is a
``ValueError``.  The constants of ``contains`` / ``suffix`` are literal; they
compile to the patterns ``%x%`` / ``%x``, so one kernel
(csrc/kernels/collike.hip) serves all of them.  A utf8 column may hold bytes
that are not UTF-8 (file data): there ``_`` is one byte and every 0x80-0xBF
byte directly after it, in the kernel, its host copy and the twin here
alike; pyarrow parity holds for valid UTF-8 and for binary columns.  Limits
(``ValueError`` beyond them): ``MAX_LIKE_BYTES`` bytes per pattern,
``MAX_LIKE_SEGMENTS`` pieces between ``%`` per pattern, ``MAX_LIKE_PATTERNS``
patterns per predicate, and all operands within ``MAX_QUAL_BYTES``.  Not
offered: case-insensitive matching (ILIKE), regular expressions, another
escape character, collations, ``_`` as a grapheme cluster.

Dictionary-encoded columns are evaluated on the dictionary (host, numpy,
this module's twin) and the GPU tests each row's index against the
resulting lookup table — any predicate, including string ranges, costs one
bit test per row.  The reference has no columnar path (new
MI355X work); the predicate model follows PG-Strom's qualifier lists.
"""
from __future__ import annotations

import ctypes as C
import datetime as _dt
import math
import struct
from dataclasses import dataclass, field
from fractions import Fraction
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from ..utils.arrow_ipc import Column

# strom.h: STROM_COL_* storage types, STROM_QOP_* operators, STROM_QUAL_* flags
COL_CODE = {"i4": 1, "i8": 2, "f4": 3, "f8": 4, "i1": 5, "i2": 6, "u1": 7, "u2": 8, "u4": 9,
            "u8": 10, "b1": 11, "d16": 14}
COL_STR32, COL_STR64 = 12, 13
QOP_RANGES, QOP_STR_IN, QOP_STR_PREFIX, QOP_LUT, QOP_VALID, QOP_STR_RANGES = 1, 2, 3, 4, 5, 6
QOP_STR_LIKE = 7
FLAG_NEGATE, FLAG_NAN, FLAG_LIKE_WILD, FLAG_LIKE_UTF8 = 1, 2, 4, 8
LIKE_HEAD, LIKE_TAIL = 1, 2       # pattern flags: no leading / no trailing %
MAX_RANGES = 4096                 # the kernel stages constants in LDS (<= 64 KiB)
MAX_CONST_BYTES = 48 << 10
MAX_QUAL_BYTES = 64 << 10         # strom_column_qual: constants + string offsets
MAX_LUT_BITS = 512 << 10
MAX_LIKE_BYTES = 4096             # one LIKE pattern (a contains / suffix constant)
MAX_LIKE_SEGMENTS = 64            # its pieces between %
MAX_LIKE_PATTERNS = 64            # patterns OR-ed in one predicate

OPS = {"==", "!=", "<", "<=", ">", ">=", "between", "in", "not in", "ranges", "prefix",
       "not prefix", "suffix", "not suffix", "contains", "not contains", "like", "not like",
       "is_null", "is_valid"}
_NEG = {"!=": "==", "not in": "in", "not prefix": "prefix", "not suffix": "suffix",
        "not contains": "contains", "not like": "like"}
_LIKE_OPS = ("like", "contains", "suffix")


@dataclass(frozen=True)
class Pred:
    col: object                   # a column name, or an expression (ops/colexpr.E)
    op: str
    value: object = None

    def __post_init__(self):
        if self.op not in OPS:
            raise ValueError(f"predicate op {self.op!r}: one of {sorted(OPS)}")


class P:
    """Builder: ``P("name") == "abc"``, ``P("d").between(a, b)``,
    ``P("k").isin([1, 5])``, ``P("s").startswith("ab")``.  Arithmetic on it
    gives an expression (ops/colexpr.py): ``P("a") * 2 + P("b") > 5``."""

    def __init__(self, col: str):
        self.col = col

    def __eq__(self, v): return Pred(self.col, "==", v)      # noqa: E704
    def __ne__(self, v): return Pred(self.col, "!=", v)      # noqa: E704
    def __lt__(self, v): return Pred(self.col, "<", v)       # noqa: E704
    def __le__(self, v): return Pred(self.col, "<=", v)      # noqa: E704
    def __gt__(self, v): return Pred(self.col, ">", v)       # noqa: E704
    def __ge__(self, v): return Pred(self.col, ">=", v)      # noqa: E704
    __hash__ = None

    def _e(self):
        from .colexpr import E
        return E(self.col)

    def __add__(self, o): return self._e() + o               # noqa: E704
    def __radd__(self, o): return o + self._e()              # noqa: E704
    def __sub__(self, o): return self._e() - o               # noqa: E704
    def __rsub__(self, o): return o - self._e()              # noqa: E704
    def __mul__(self, o): return self._e() * o               # noqa: E704
    def __rmul__(self, o): return o * self._e()              # noqa: E704
    def __truediv__(self, o): return self._e() / o           # noqa: E704
    def __rtruediv__(self, o): return o / self._e()          # noqa: E704
    def __floordiv__(self, o): return self._e() // o         # noqa: E704
    def __mod__(self, o): return self._e() % o               # noqa: E704
    def __neg__(self): return -self._e()                     # noqa: E704
    def __abs__(self): return abs(self._e())                 # noqa: E704

    def between(self, lo, hi) -> Pred:
        return Pred(self.col, "between", (lo, hi))

    def isin(self, values) -> Pred:
        return Pred(self.col, "in", tuple(values))

    def not_in(self, values) -> Pred:
        return Pred(self.col, "not in", tuple(values))

    def ranges(self, rs) -> Pred:
        return Pred(self.col, "ranges", tuple(tuple(r) for r in rs))

    def startswith(self, prefix) -> Pred:
        return Pred(self.col, "prefix", prefix)

    def endswith(self, suffix) -> Pred:
        return Pred(self.col, "suffix", suffix)

    def contains(self, sub) -> Pred:
        return Pred(self.col, "contains", sub)

    def like(self, pattern) -> Pred:
        return Pred(self.col, "like", pattern)

    def not_like(self, pattern) -> Pred:
        return Pred(self.col, "not like", pattern)

    def is_null(self) -> Pred:
        return Pred(self.col, "is_null")

    def is_valid(self) -> Pred:
        return Pred(self.col, "is_valid")


@dataclass(frozen=True)
class Or:
    preds: Tuple[Pred, ...]

    def __init__(self, *preds):
        object.__setattr__(self, "preds", tuple(as_pred(p) for p in preds))
        if not self.preds:
            raise ValueError("Or() of nothing")


def as_pred(q) -> Pred:
    if isinstance(q, Pred):
        return q
    if isinstance(q, tuple) and len(q) >= 2 and (isinstance(q[0], str) or hasattr(q[0], "key")):
        if isinstance(q[1], str) and q[1] in OPS:
            return Pred(q[0], q[1], q[2] if len(q) > 2 else None)
        if len(q) == 3:
            return Pred(q[0], "between", (q[1], q[2]))
    raise ValueError(f"not a predicate: {q!r}")


def clauses(quals) -> List[List[Pred]]:
    """CNF: a list of OR-clauses (each a list of predicates), ANDed."""
    out = []
    for q in quals:
        if isinstance(q, Or):
            out.append(list(q.preds))
        elif isinstance(q, list):
            out.append([as_pred(p) for p in q])
        else:
            out.append([as_pred(q)])
    if not out:
        raise ValueError("at least one qualifier")
    return out


# ------------------------------------------------------------ compilation
@dataclass
class Compiled:
    """Kernel operands of one predicate on one column's record-batch data."""
    type: int                       # STROM_COL_*
    op: int                         # STROM_QOP_*
    flags: int = 0
    nconst: int = 0
    consts: bytes = b""             # ranges / string blob / LUT words
    offs: bytes = b""               # strings: (start, len) uint32 pairs
    # numpy twin operands
    ranges: Optional[np.ndarray] = None       # (n, 2) in the compare domain
    strings: Optional[List[bytes]] = None
    lut: Optional[np.ndarray] = None          # bool per dictionary index
    patterns: Optional[list] = None           # LIKE: (head, tail, segments) per pattern
    _dev: Dict[str, object] = field(default_factory=dict, repr=False)


_TICKS = {"s": 1, "ms": 10 ** 3, "us": 10 ** 6, "ns": 10 ** 9}
_EPOCH = _dt.datetime(1970, 1, 1, tzinfo=_dt.timezone.utc)


def _exact(v, col: Column) -> Fraction:
    """A scalar as an exact rational in the column's storage domain
    (date32 days, date64 ms, time/timestamp/duration ticks of its unit)."""
    if isinstance(v, (bool, np.bool_)):
        return Fraction(int(v))
    if isinstance(v, (int, np.integer)):
        return Fraction(int(v))
    if isinstance(v, Fraction):
        return v
    if isinstance(v, (float, np.floating)):
        if math.isnan(v) or math.isinf(v):
            raise OverflowError
        return Fraction(float(v))
    import decimal as _dec
    if isinstance(v, _dec.Decimal):
        if not v.is_finite():
            raise OverflowError
        return Fraction(v)
    k = col.kind
    tick = Fraction(86400) if col.unit == "d" else Fraction(1, _TICKS.get(col.unit, 1))
    if hasattr(v, "to_datetime64") or hasattr(v, "to_timedelta64"):   # pandas scalars
        v = v.to_datetime64() if hasattr(v, "to_datetime64") else v.to_timedelta64()
    if isinstance(v, np.datetime64) or isinstance(v, np.timedelta64):
        ns = int(v.astype("datetime64[ns]" if isinstance(v, np.datetime64)
                          else "timedelta64[ns]").astype(np.int64))
        return Fraction(ns, 10 ** 9) / tick
    if isinstance(v, str) and k in ("date", "timestamp"):
        v = (_dt.date.fromisoformat(v) if k == "date" and len(v) == 10
             else _dt.datetime.fromisoformat(v))
    if isinstance(v, _dt.datetime):
        if v.tzinfo is None:
            v = v.replace(tzinfo=_dt.timezone.utc)
        d = v - _EPOCH
        secs = Fraction(d.days * 86400 + d.seconds) + Fraction(d.microseconds, 10 ** 6)
        return secs / tick
    if isinstance(v, _dt.date):
        return Fraction((v - _dt.date(1970, 1, 1)).days * 86400) / tick
    if isinstance(v, _dt.time):
        secs = Fraction(v.hour * 3600 + v.minute * 60 + v.second) + Fraction(v.microsecond, 10 ** 6)
        return secs / tick
    if isinstance(v, _dt.timedelta):
        secs = Fraction(v.days * 86400 + v.seconds) + Fraction(v.microseconds, 10 ** 6)
        return secs / tick
    raise TypeError(f"column {col.name} ({col.kind}): cannot compare with {type(v).__name__}")


def _int_bounds(dt: str) -> Tuple[int, int]:
    if dt == "b1":
        return 0, 1
    if dt == "d16":
        return -(1 << 127), (1 << 127) - 1
    info = np.iinfo(np.dtype(dt))
    return int(info.min), int(info.max)


def _dbl(v, col: Column) -> float:
    if isinstance(v, (float, np.floating)):
        return float(v)
    return float(_exact(v, col))


def _dbl_floor(x: Fraction) -> float:
    f = float(x)
    return f if Fraction(f) <= x else math.nextafter(f, -math.inf)


def _dbl_ceil(x: Fraction) -> float:
    f = float(x)
    return f if Fraction(f) >= x else math.nextafter(f, math.inf)


def _merge(rs: List[Tuple], adjacent_int: bool) -> List[Tuple]:
    rs = sorted(r for r in rs if r[0] <= r[1])
    out: List[list] = []
    for lo, hi in rs:
        if out and lo <= out[-1][1] + (1 if adjacent_int else 0):
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return [tuple(r) for r in out]


def _dec_float_bound(x: float, side: str, scale: Fraction, tmin: int, tmax: int) -> int:
    """Bound on the unscaled integer u of a decimal column compared with a
    float constant the way pyarrow.compute does it: the column is cast to
    float64, so u qualifies iff float64(u / 10^scale) <op> x (float() of a
    Fraction rounds correctly, as the cast does for |u| < 2^53).  That map
    is monotone in u, so the bound is the first u whose float passes
    (``>=`` / ``>``), or the one before it (``<`` / ``<=``), found by
    bisection over the storage range (float spacing can exceed 10^-scale,
    so several u round onto x)."""
    strict = side in (">", "<=")               # first u with fl(u) > x, else >= x

    def ok(u: int) -> bool:
        f = float(Fraction(u) / scale)
        return f > x if strict else f >= x
    lo, hi = tmin - 1, tmax + 1                # ok(lo) taken false, ok(hi) true
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ok(mid):
            hi = mid
        else:
            lo = mid
    return hi if side in (">", ">=") else hi - 1


def _num_ranges(op: str, v, col: Column, dt: str) -> Tuple[List[Tuple], int]:
    """(ranges in the compare domain, extra flags) of a numeric predicate
    (op already stripped of its negation)."""
    isf = dt in ("f4", "f8")
    if isf:
        def bound(x, side):                   # side: "<", "<=", ">", ">="
            if isinstance(x, (float, np.floating)) and math.isnan(x):
                return None
            if isinstance(x, (float, np.floating)) and math.isinf(x):
                f = float(x)
            else:
                e = _exact(x, col)
                f = _dbl_floor(e) if side in ("<", "<=") else _dbl_ceil(e)
                if side == "<" and Fraction(f) == e:
                    f = math.nextafter(f, -math.inf)
                if side == ">" and Fraction(f) == e:
                    f = math.nextafter(f, math.inf)
                return f
            if side == "<":
                return math.nextafter(f, -math.inf)
            if side == ">":
                return math.nextafter(f, math.inf)
            return f
        NEG, POS = -math.inf, math.inf
    else:
        tmin, tmax = _int_bounds(dt)

        scale = Fraction(10) ** col.scale if col.kind == "decimal" else 1

        def bound(x, side):
            if col.kind == "decimal" and isinstance(x, (float, np.floating)) and math.isfinite(x):
                return _dec_float_bound(float(x), side, scale, tmin, tmax)
            try:
                e = _exact(x, col) * scale
            except OverflowError:               # NaN compares false, +-inf past any int
                if isinstance(x, (float, np.floating)) and math.isinf(x):
                    return tmax + 1 if x > 0 else tmin - 1
                return None
            if side == "<":
                return math.ceil(e) - 1
            if side == "<=":
                return math.floor(e)
            if side == ">":
                return math.floor(e) + 1
            return math.ceil(e)
        NEG, POS = tmin, tmax

    def rng(lo_v, lo_side, hi_v, hi_side):
        lo = NEG if lo_v is None else bound(lo_v, lo_side)
        hi = POS if hi_v is None else bound(hi_v, hi_side)
        if lo is None or hi is None:
            return []
        if not isf:
            lo, hi = max(lo, tmin), min(hi, tmax)
        return [(lo, hi)] if lo <= hi else []

    flags = 0
    if op == "==":
        rs = rng(v, ">=", v, "<=")
    elif op == "<":
        rs = rng(None, "", v, "<")
    elif op == "<=":
        rs = rng(None, "", v, "<=")
    elif op == ">":
        rs = rng(v, ">", None, "")
    elif op == ">=":
        rs = rng(v, ">=", None, "")
    elif op == "between":
        lo, hi = v
        rs = rng(lo, ">=", hi, "<=")
    elif op in ("in", "ranges"):
        rs = []
        for x in v:
            if op == "in":
                if isf and isinstance(x, (float, np.floating)) and math.isnan(x):
                    flags |= FLAG_NAN
                    continue
                rs += rng(x, ">=", x, "<=")
            else:
                rs += rng(x[0], ">=", x[1], "<=")
    else:
        raise ValueError(f"column {col.name} ({col.kind}): op {op!r} not defined")
    return _merge(rs, not isf), flags


def _string_const(v, col: Column) -> bytes:
    if isinstance(v, str):
        return v.encode()
    if isinstance(v, (bytes, bytearray, memoryview, np.bytes_)):
        return bytes(v)
    raise TypeError(f"column {col.name} ({col.kind}): cannot compare with {type(v).__name__}")


def _string_ranges(op: str, v, col: Column, code: int, flags: int) -> Compiled:
    """Bytewise-lexicographic ranges (pyarrow compares utf8 by its bytes):
    per range two bounds (start, len, mode), mode 0 unbounded, 1
    inclusive, 2 exclusive."""
    sc = lambda x: _string_const(x, col)
    if op == "<":
        rs = [(None, 0, sc(v), 2)]
    elif op == "<=":
        rs = [(None, 0, sc(v), 1)]
    elif op == ">":
        rs = [(sc(v), 2, None, 0)]
    elif op == ">=":
        rs = [(sc(v), 1, None, 0)]
    elif op == "between":
        rs = [(sc(v[0]), 1, sc(v[1]), 1)]
    elif op == "ranges":
        rs = [(sc(a), 1, sc(b), 1) for a, b in v]
    else:
        raise ValueError(f"column {col.name} ({col.kind}): op {op!r} not defined")
    blob, offs = bytearray(), []
    for lo, lm, hi, hm in rs:
        for b, m in ((lo, lm), (hi, hm)):
            b = b or b""
            offs += [len(blob), len(b), m]
            blob += b + b"\0" * (-len(b) % 4)
    if len(blob) > MAX_CONST_BYTES or len(rs) > MAX_RANGES or \
            len(blob) + 24 * len(rs) > MAX_QUAL_BYTES:
        raise ValueError(f"column {col.name}: {len(rs)} string ranges, {len(blob)} bytes "
                         f"(device limit {MAX_QUAL_BYTES} bytes with 24 per range)")
    return Compiled(code, QOP_STR_RANGES, flags, len(rs), bytes(blob) or b"\0\0\0\0",
                    np.asarray(offs, np.uint32).tobytes(), strings=rs)


def _like_escape(b: bytes) -> bytes:
    return b.replace(b"\\", b"\\\\").replace(b"%", b"\\%").replace(b"_", b"\\_")


def _like_parse(pat: bytes, col: Column):
    """(head, tail, segments) of one LIKE pattern.  head / tail: it has no
    leading / trailing ``%``.  A segment, one of the pieces between ``%``,
    is (pieces, trail, least): pieces a list of (number of ``_`` before
    it, literal bytes), trail the ``_`` after the last piece, least the
    fewest bytes it can match (a ``_`` is at least one byte)."""
    segs, toks, i, n = [], [], 0, len(pat)       # toks: a byte value, or None for _
    cuts = 0
    while i < n:
        ch = pat[i]
        if ch == 0x5C:                             # backslash
            if i + 1 >= n or pat[i + 1] not in b"%_\\":
                raise ValueError(f"column {col.name}: LIKE pattern {pat!r}: a backslash escapes "
                                 f"only %, _ and itself (at byte {i})")
            toks.append(pat[i + 1])
            i += 2
            continue
        if ch == 0x25:                             # %
            segs.append(toks)
            toks = []
            cuts += 1
        else:
            toks.append(None if ch == 0x5F else ch)
        i += 1
    segs.append(toks)
    head, tail = bool(segs[0]) or not cuts, bool(segs[-1]) or not cuts
    out = []
    for toks in segs:
        if not toks:
            continue
        pieces, skip, lit = [], 0, bytearray()
        for t in toks:
            if t is None:
                if lit:
                    pieces.append((skip, bytes(lit)))
                    skip, lit = 0, bytearray()
                skip += 1
            else:
                lit.append(t)
        trail = 0
        if lit:
            pieces.append((skip, bytes(lit)))
        else:
            trail = skip
        out.append((pieces, trail, len(toks)))
    return head, tail, out


def _compile_like(op: str, v, col: Column, code: int, flags: int) -> Compiled:
    """``like`` / ``contains`` / ``suffix`` to the STROM_QOP_STR_LIKE
    operands (strom.h has the layout): the literal pieces 4-aligned in
    ``consts``; in ``offs`` one word per pattern (where its record is),
    then the pattern records (flags, least bytes, nseg, where each segment
    record is) and the segment records (least bytes, npiece, trailing
    ``_``, then per piece: ``_`` before it, start, length)."""
    if op == "like":
        if isinstance(v, (list, tuple)):
            raise ValueError(f"column {col.name}: like takes one pattern")
        pats = [_string_const(v, col)]
    else:
        vs = v if isinstance(v, (list, tuple)) else [v]
        wrap = (b"%", b"%") if op == "contains" else (b"%", b"")
        pats = [wrap[0] + _like_escape(_string_const(x, col)) + wrap[1] for x in vs]
    pats = sorted(set(pats))
    if not pats or len(pats) > MAX_LIKE_PATTERNS:
        raise ValueError(f"column {col.name}: {len(pats)} patterns in one predicate "
                         f"(1 to MAX_LIKE_PATTERNS = {MAX_LIKE_PATTERNS})")
    parsed = []
    for pat in pats:
        if len(pat) > MAX_LIKE_BYTES:
            raise ValueError(f"column {col.name}: a pattern of {len(pat)} bytes "
                             f"(MAX_LIKE_BYTES = {MAX_LIKE_BYTES})")
        head, tail, segs = _like_parse(pat, col)
        if len(segs) > MAX_LIKE_SEGMENTS:
            raise ValueError(f"column {col.name}: {len(segs)} segments between % in one pattern "
                             f"(MAX_LIKE_SEGMENTS = {MAX_LIKE_SEGMENTS})")
        parsed.append((head, tail, segs))
    blob, words = bytearray(), [0] * len(parsed)
    wild = False
    for k, (head, tail, segs) in enumerate(parsed):
        words[k] = len(words)
        at = len(words)
        words += [(LIKE_HEAD if head else 0) | (LIKE_TAIL if tail else 0),
                  sum(s[2] for s in segs), len(segs)] + [0] * len(segs)
        for j, (pieces, trail, least) in enumerate(segs):
            words[at + 3 + j] = len(words)
            words += [least, len(pieces), trail]
            wild |= bool(trail) or any(sk for sk, _ in pieces)
            for sk, lit in pieces:
                words += [sk, len(blob), len(lit)]
                blob += lit + b"\0" * (-len(lit) % 4)
    if len(blob) + 4 * len(words) > MAX_QUAL_BYTES:
        raise ValueError(f"column {col.name}: LIKE operands of {len(blob) + 4 * len(words)} bytes "
                         f"(MAX_QUAL_BYTES = {MAX_QUAL_BYTES}: literals, 12 bytes per piece, "
                         f"16 per segment and per pattern)")
    if wild:
        flags |= FLAG_LIKE_WILD | (FLAG_LIKE_UTF8 if col.kind == "utf8" else 0)
    return Compiled(code, QOP_STR_LIKE, flags, len(parsed), bytes(blob) or b"\0\0\0\0",
                    np.asarray(words, np.uint32).tobytes(), patterns=parsed)


def _compile_value(p: Pred, col: Column, dt: str, code: int) -> Compiled:
    """A predicate on a plain (not dictionary-encoded) column."""
    op = p.op
    neg = op in _NEG
    base = _NEG.get(op, op)
    if base in ("is_null", "is_valid"):
        return Compiled(code, QOP_VALID, FLAG_NEGATE if base == "is_null" else 0)
    flags = FLAG_NEGATE if neg else 0
    if col.kind in ("utf8", "binary"):
        if base in _LIKE_OPS:
            return _compile_like(base, p.value, col, code, flags)
        if base == "==":
            vals, qop = [_string_const(p.value, col)], QOP_STR_IN
        elif base == "in":
            vals, qop = [_string_const(x, col) for x in p.value], QOP_STR_IN
        elif base == "prefix":
            pv = p.value if isinstance(p.value, (list, tuple)) else [p.value]
            vals, qop = [_string_const(x, col) for x in pv], QOP_STR_PREFIX
        else:
            return _string_ranges(base, p.value, col, code, flags)
        vals = sorted(set(vals))
        blob, offs = bytearray(), []
        for b in vals:
            offs += [len(blob), len(b)]
            blob += b + b"\0" * (-len(b) % 4)
        if len(blob) > MAX_CONST_BYTES or len(vals) > MAX_RANGES or \
                len(blob) + 8 * len(vals) > MAX_QUAL_BYTES:
            raise ValueError(f"column {col.name}: {len(vals)} string constants, "
                             f"{len(blob)} bytes (device limit {MAX_CONST_BYTES} bytes, "
                             f"{MAX_QUAL_BYTES} with 8 per constant)")
        return Compiled(code, qop, flags, len(vals), bytes(blob) or b"\0\0\0\0",
                        np.asarray(offs or [0, 0], np.uint32).tobytes(), strings=vals)
    if base == "prefix" or base in _LIKE_OPS:
        raise ValueError(f"column {col.name} ({col.kind}): {base} needs utf8/binary")
    rs, extra = _num_ranges(base, p.value, col, dt)
    limit = min(MAX_RANGES, MAX_QUAL_BYTES // (32 if dt == "d16" else 16))
    if len(rs) > limit:
        raise ValueError(f"column {col.name}: {len(rs)} disjoint ranges (limit {limit})")
    if dt == "d16":
        # 128-bit bounds, (lo, hi) pairs of little-endian two's complement
        blob = b"".join(int(x).to_bytes(16, "little", signed=True) for r in rs for x in r)
        return Compiled(code, QOP_RANGES, flags | extra, len(rs), blob or b"\0" * 32,
                        ranges=np.array(rs, dtype=object).reshape(-1, 2))
    isf = dt in ("f4", "f8")
    cdt = np.float64 if isf else (np.uint64 if dt == "u8" else np.int64)
    arr = np.asarray(rs, dtype=cdt).reshape(-1, 2)
    return Compiled(code, QOP_RANGES, flags | extra, len(rs),
                    arr.tobytes() if len(rs) else b"\0" * 16, ranges=arr)


def compile_pred(p: Pred, col: Column, dictionary=None) -> Compiled:
    """Kernel operands of ``p`` on ``col``.  A dictionary-encoded column
    needs ``dictionary`` = (values, valid) as arrow_ipc.dictionary_values
    returns them: the predicate is evaluated on it here and becomes a
    lookup table over the indices."""
    if not col.supported:
        raise NotImplementedError(f"column {col.name}: {col.kind} columns are not scanned")
    if col.dictionary is not None:
        code = COL_CODE[col.storage]
        if p.op in ("is_null", "is_valid"):
            return Compiled(code, QOP_VALID, FLAG_NEGATE if p.op == "is_null" else 0)
        if dictionary is None:
            raise ValueError(f"column {col.name}: dictionary values needed")
        vals, dvalid = dictionary
        vcol = Column(col.name, col.kind, col.bit_width, col.signed, unit=col.unit, tz=col.tz,
                      large=col.large, precision=col.precision, scale=col.scale)
        inner = compile_pred(p, vcol)
        n = len(vals[0]) - 1 if isinstance(vals, tuple) else len(vals)
        hit = evaluate(inner, vals, dvalid, n)
        if n > MAX_LUT_BITS:
            raise ValueError(f"column {col.name}: dictionary of {n} entries (limit {MAX_LUT_BITS})")
        words = np.packbits(np.concatenate([hit, np.zeros(-n % 32 or 0, bool)]),
                            bitorder="little").view("<u4") if n else np.zeros(1, "<u4")
        return Compiled(code, QOP_LUT, 0, n, words.tobytes(), lut=hit)
    if col.kind in ("utf8", "binary"):
        code = COL_STR64 if col.large else COL_STR32
        dt = col.storage
    else:
        dt = col.storage
        if dt not in COL_CODE:
            raise NotImplementedError(f"column {col.name}: storage {dt}")
        code = COL_CODE[dt]
    return _compile_value(p, col, dt, code)


# ------------------------------------------------------------ numpy twin
def _str_rows(values, n: int, ok: np.ndarray):
    """(start, length, characters, ok) of n rows of a utf8/binary column.
    A row whose offset pair is negative, decreasing or ends past the
    characters (file data) is selected by no string operator, negated or
    not (as the kernel): it leaves ``ok`` and reads as an empty string."""
    offs, data = values
    offs = np.asarray(offs[:n + 1], np.int64)
    if not isinstance(data, np.ndarray):
        data = np.frombuffer(bytes(data), np.uint8)
    a, e = offs[:-1], offs[1:]
    bad = (a < 0) | (e < a) | (e > len(data))
    return np.where(bad, 0, a), np.where(bad, 0, e - a), data, ok & ~bad


# LIKE: the kernel's segment algorithm (csrc/kernels/collike.hip), every step
# one numpy operation over the rows (or candidate positions) still matching;
# the Python loops run over a pattern's segments, pieces and bytes only.
def _like_fwd(seg, p, lim, data, nxt, want_need: bool = False):
    """The segment at positions ``p``, each inside [p, lim): (matches, where
    it ends[, need]).  ``nxt``: per position the next one that continues no
    character (utf8), None for one byte per ``_``.  ``need``: the end, or
    with a trailing ``_`` one byte past where the last ``_`` starts - a match
    found with a limit further out holds for a nearer limit iff need <= it,
    and then ends at min(end, limit): only the last ``_`` can be cut short."""
    pieces, trail, _ = seg
    q = np.array(p, np.int64)
    alive = np.arange(len(q))

    def skip(alive, k):
        for _ in range(k):
            alive = alive[q[alive] < lim[alive]]
            a = q[alive]
            q[alive] = a + 1 if nxt is None else np.minimum(nxt[a], lim[alive])
        return alive
    for sk, lit in pieces:
        alive = skip(alive, sk)
        alive = alive[lim[alive] - q[alive] >= len(lit)]
        for j, ch in enumerate(lit):
            alive = alive[data[q[alive] + j] == ch]
        q[alive] += len(lit)
    need = None
    if trail:
        alive = skip(alive, trail - 1)
        alive = alive[q[alive] < lim[alive]]
        need = q + 1
        alive = skip(alive, 1)
    ok = np.zeros(len(q), bool)
    ok[alive] = True
    if want_need:
        return ok, q, (q if need is None else need)
    return ok, q


def _like_bwd(seg, e, lo, data, prv):
    """The segment ending at positions ``e``, each inside [lo, e): (matches,
    where it begins).  ``prv``: per position the last one before it that
    continues no character (-1: none), None for one byte per ``_``."""
    pieces, trail, _ = seg
    q = np.array(e, np.int64)
    alive = np.arange(len(q))

    def skip(alive, k):
        for _ in range(k):
            alive = alive[q[alive] > lo[alive]]
            a = q[alive]
            q[alive] = a - 1 if prv is None else np.maximum(prv[a], lo[alive])
        return alive
    alive = skip(alive, trail)
    for sk, lit in reversed(pieces):
        L = len(lit)
        alive = alive[q[alive] - lo[alive] >= L]
        for j, ch in enumerate(lit):
            alive = alive[data[q[alive] - L + j] == ch]
        q[alive] -= L
        alive = skip(alive, sk)
    ok = np.zeros(len(q), bool)
    ok[alive] = True
    return ok, q


def _like_scan(seg, data, nxt):
    """Every position of the character buffer the segment matches at,
    ascending, with (need, end) of each match as _like_fwd defines them for
    the buffer's end as the limit."""
    N = len(data)
    pieces = seg[0]
    if pieces and not pieces[0][0]:                 # starts with a literal: its first byte
        L = len(pieces[0][1])
        p = np.flatnonzero(data[:max(N - L + 1, 0)] == pieces[0][1][0])
    else:
        p = np.arange(N + 1)
    ok, q, need = _like_fwd(seg, p, np.full(len(p), N, np.int64), data, nxt, True)
    return p[ok], need[ok], q[ok]


def _like_eval(c: Compiled, st, ln, data) -> np.ndarray:
    n, N = len(st), len(data)
    hit = np.zeros(n, bool)
    nxt = prv = None
    if c.flags & FLAG_LIKE_UTF8:
        lead = np.flatnonzero((data & 0xC0) != 0x80)
        at = np.arange(N + 1)
        nxt = np.concatenate([lead, [N]])[np.searchsorted(lead, at, side="right")]
        prv = np.concatenate([[-1], lead])[np.searchsorted(lead, at, side="left")]
    en = st + ln
    for head, tail, segs in c.patterns:
        rows = np.flatnonzero(~hit & (ln >= sum(s[2] for s in segs)))   # the length reject
        if not segs:
            hit[rows[ln[rows] == 0] if head else rows] = True
            continue
        cur, end = st[rows].astype(np.int64), en[rows].astype(np.int64)
        first, last = 0, len(segs)
        if head:
            ok, q = _like_fwd(segs[0], cur, end, data, nxt)
            if tail and len(segs) == 1:
                hit[rows[ok & (q == end)]] = True
                continue
            first = 1
            rows, cur, end = rows[ok], q[ok], end[ok]
        if tail:
            # from the end, and not beginning before the point the head ended at
            ok, q = _like_bwd(segs[-1], end, cur, data, prv)
            last -= 1
            rows, cur, end = rows[ok], cur[ok], q[ok]
        # the segments between, leftmost-first.  No backtracking across a %:
        # where a segment can end never decreases with where it starts, so
        # the leftmost match leaves the longest remainder for the rest.
        for seg in segs[first:last]:
            if not len(rows):
                break
            pos, need, e = _like_scan(seg, data, nxt)
            if not len(pos):
                rows = rows[:0]
                break
            j = np.searchsorted(pos, cur)
            jj = np.minimum(j, len(pos) - 1)
            ok = (j < len(pos)) & (need[jj] <= end)
            rows, cur, end = rows[ok], np.minimum(e[jj], end)[ok], end[ok]
        hit[rows] = True
    return hit


def evaluate(c: Compiled, values, valid: Optional[np.ndarray], n: int) -> np.ndarray:
    """The kernel's bits for n rows on the host: values as
    arrow_ipc.decode_values returns them (indices for a LUT)."""
    ok = np.ones(n, bool) if valid is None else np.asarray(valid[:n], bool)
    if c.op == QOP_VALID:
        return ~ok if c.flags & FLAG_NEGATE else ok
    if c.op == QOP_RANGES and c.type == COL_CODE["d16"]:
        rs = [(int(a), int(b)) for a, b in c.ranges]
        hit = np.array([any(a <= int(x) <= b for a, b in rs) for x in values[:n]], bool)
        if c.flags & FLAG_NEGATE:
            hit = ~hit
        return hit & ok
    if c.op == QOP_RANGES:
        x = np.asarray(values[:n])
        if x.dtype == bool:
            x = x.astype(np.int64)
        r = c.ranges
        if x.dtype.kind == "f":
            x = x.astype(np.float64)
        elif x.dtype == np.uint64:
            pass
        else:
            x = x.astype(np.int64)
        if len(r):
            r = r.astype(x.dtype) if x.dtype.kind != "f" else r
            k = np.searchsorted(r[:, 1], x, side="left")
            kk = np.minimum(k, len(r) - 1)
            hit = (k < len(r)) & (r[kk, 0] <= x)
        else:
            hit = np.zeros(n, bool)
        if c.flags & FLAG_NAN:
            hit |= np.isnan(x)
    elif c.op in (QOP_STR_IN, QOP_STR_PREFIX):
        st, ln, data, ok = _str_rows(values, n, ok)
        hit = np.zeros(n, bool)
        for s in c.strings:
            L = len(s)
            cand = np.flatnonzero(ln == L if c.op == QOP_STR_IN else ln >= L)
            if L == 0 or not len(cand):
                hit[cand] = True
                continue
            ref = np.frombuffer(s, np.uint8)
            m = data[st[cand][:, None] + np.arange(L)[None, :]] == ref[None, :]
            hit[cand[m.all(axis=1)]] = True
    elif c.op == QOP_STR_RANGES:
        st, ln, data, ok = _str_rows(values, n, ok)
        raw = data.tobytes()
        col = [raw[st[i]:st[i] + ln[i]] for i in range(n)]
        hit = np.zeros(n, bool)
        for lo, lm, hi, hm in c.strings:
            ok_lo = [True] * n if not lm else [x >= lo if lm == 1 else x > lo for x in col]
            ok_hi = [True] * n if not hm else [x <= hi if hm == 1 else x < hi for x in col]
            hit |= np.asarray(ok_lo, bool) & np.asarray(ok_hi, bool)
    elif c.op == QOP_STR_LIKE:
        st, ln, data, ok = _str_rows(values, n, ok)
        hit = _like_eval(c, st, ln, data)
    elif c.op == QOP_LUT:
        idx = np.asarray(values[:n]).astype(np.int64)
        inr = (idx >= 0) & (idx < len(c.lut))
        hit = np.zeros(n, bool)
        hit[inr] = c.lut[idx[inr]]
    else:
        raise ValueError(f"op {c.op}")
    if c.flags & FLAG_NEGATE:
        hit = ~hit
    return hit & ok


# ------------------------------------------------------------ device launch
class ColQual(C.Structure):
    """struct strom_col_qual (strom.h)."""
    _fields_ = [("type", C.c_int32), ("op", C.c_int32), ("flags", C.c_uint32),
                ("nconst", C.c_uint32), ("consts", C.c_uint64), ("offs", C.c_uint64),
                ("const_bytes", C.c_uint64), ("offs_bytes", C.c_uint64)]


# struct strom_qual_batch: values, valid, nrows, word_base, row_base, aux, aux_len
QUAL_BATCH_FIELDS = 7


def device_qual(c: Compiled, device) -> ColQual:
    """The kernel argument of ``c`` with its constants uploaded to
    ``device`` once (kept on ``c``)."""
    import torch
    key = str(device)
    if key not in c._dev:
        cs = torch.frombuffer(bytearray(c.consts or b"\0" * 4), dtype=torch.uint8).to(device)
        of = torch.frombuffer(bytearray(c.offs or b"\0" * 8), dtype=torch.uint8).to(device)
        q = ColQual(c.type, c.op, c.flags, c.nconst, cs.data_ptr(), of.data_ptr(),
                    len(c.consts), len(c.offs))
        c._dev[key] = (q, cs, of)
    return c._dev[key][0]


def like_host(c: Compiled, batches: np.ndarray, nwords: int, bitmap: np.ndarray,
              or_src: Optional[np.ndarray] = None, and_dst: bool = False) -> int:
    """The library's host copy of the LIKE kernel (strom_column_like_host)
    over a (nbatches, 7) uint64 table of host pointers: ``bitmap`` (uint64,
    nwords) is combined as the kernel does; returns the popcount of what was
    written.  Character buffers are 4-byte aligned and readable up to the
    dword holding their last byte (numpy allocations padded to 4 are)."""
    from .. import _native as N
    if c.op != QOP_STR_LIKE:
        raise ValueError("like_host: a LIKE predicate")
    batches = np.ascontiguousarray(batches, np.uint64)
    if batches.ndim != 2 or batches.shape[1] != QUAL_BATCH_FIELDS or bitmap.dtype != np.uint64 \
            or len(bitmap) < nwords:
        raise ValueError("like_host: batches uint64 (n, 7), bitmap uint64[nwords]")
    cs = np.frombuffer(c.consts, np.uint8).copy()
    of = np.frombuffer(c.offs, np.uint8).copy()
    q = ColQual(c.type, c.op, c.flags, c.nconst, cs.ctypes.data, of.ctypes.data, len(cs), len(of))
    cnt = np.zeros(1, np.uint64)
    rc = N.lib().strom_column_like_host(C.byref(q), batches.ctypes.data, len(batches), nwords,
                                        bitmap.ctypes.data,
                                        or_src.ctypes.data if or_src is not None else None,
                                        int(and_dst), cnt.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"column_like_host failed (rc={rc})")
    return int(cnt[0])


def qual_batched(c: Compiled, batches, nwords: int, bitmap, count, stream=None,
                 or_src=None, and_dst: bool = False) -> None:
    """One launch of the qualifier kernel over a (nbatches, 7) int64 batch
    table on the device.  bitmap[w] = (pred | or_src[w]) & (and_dst ?
    bitmap[w] : ~0); ``count`` (int64[1]) += popcount of what is written."""
    from ._util import check, lib, ptr, require_cuda, stream_handle
    require_cuda(batches, "batches")
    if batches.dim() != 2 or batches.shape[1] != QUAL_BATCH_FIELDS:
        raise ValueError("batches: int64 (n, 7)")
    if bitmap.numel() < nwords:
        raise ValueError("bitmap too small")
    q = device_qual(c, batches.device)
    check(lib().strom_column_qual(C.byref(q), ptr(batches), batches.shape[0], nwords, ptr(bitmap),
                                  ptr(or_src) if or_src is not None else 0, int(and_dst),
                                  ptr(count), stream_handle(stream)), "column_qual")
