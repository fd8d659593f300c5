"""Computed columns of an Arrow scan: the expressions a query writes, their
compilation to the postfix program of the GPU kernel
(csrc/kernels/colexpr.hip, ``strom_column_expr``) and a numpy twin of that
kernel.

    E("price") * E("qty")            sum(price * qty)
    E("a") + E("b") < 5              a qualifier (a Pred on the expression)
    E("ts_ms") // 86_400_000         a HashBy key: the day of a timestamp in ms
    E("x") / E("y")                  true division: the float domain

``E(name)`` names a column; ``+ - *``, unary ``-``, ``abs()``, ``/``, and
``//`` and ``%`` by a positive Python int build larger expressions; Python
ints and floats are constants on either side.  ``P(name)`` takes the same
operators and gives an ``E``.  Comparisons (``== != < <= > >=``) and
``between / isin / not_in / ranges / is_null / is_valid`` build a ``Pred``
whose column is the expression, so ``==`` cannot tell two expressions apart:
``key()`` is their structural identity.

An expression has one domain.  float64 if a source column or a constant is a
float or ``/`` appears: integer sources are converted with round-to-nearest,
every operation is one IEEE double operation (never fused), NaN and inf come
out of ``/`` as numpy gives them, and a NaN result is stored as the one quiet
NaN 0x7ff8000000000000.  int64 otherwise: sources int8-int64 and uint8-uint32
widened, arithmetic wrapping in 64 bits (``-`` and ``abs`` of INT64_MIN give
INT64_MIN), ``//`` and ``%`` rounding toward minus infinity as numpy's
``floor_divide`` and ``remainder``.  A row is null if any source column's row
is.  Limits: no uint64, bool, decimal, string, temporal or dictionary-encoded
sources, no cast of a float to an integer, no comparison inside an
expression, at most 4 source columns, 16 ops and a stack of 8.  The reference
has no columnar path; PG-Strom evaluates such expressions on
the device ahead of its scan, aggregate and sort stages.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Sequence, Tuple

import numpy as np

from ..utils.arrow_ipc import Column
from .colpred import COL_CODE, P, Pred

MAX_OPS, MAX_COLS, MAX_DEPTH = 16, 4, 8
INT, FLT = 0, 1
(XOP_COL, XOP_CONST, XOP_ADD, XOP_SUB, XOP_MUL, XOP_NEG, XOP_ABS, XOP_DIV, XOP_FDIV,
 XOP_MOD) = range(1, 11)
NAN_BITS = 0x7FF8000000000000
_BIN = {"+": XOP_ADD, "-": XOP_SUB, "*": XOP_MUL, "/": XOP_DIV}
_INT_SRC = ("i1", "i2", "i4", "i8", "u1", "u2", "u4")
_FLT_SRC = ("f4", "f8")


class E:
    """An arithmetic expression over columns (see the module's text)."""

    __slots__ = ("_key",)

    def __init__(self, name):
        if isinstance(name, E):
            self._key = name._key
        elif isinstance(name, str):
            self._key = ("col", name)
        else:
            raise TypeError(f"E({name!r}): a column name")

    @staticmethod
    def _of(key: tuple) -> "E":
        e = E.__new__(E)
        e._key = key
        return e

    @staticmethod
    def _operand(v) -> tuple:
        if isinstance(v, E):
            return v._key
        if isinstance(v, P):
            return ("col", v.col)
        if isinstance(v, (bool, np.bool_)):
            raise TypeError("a bool is not a constant of an expression")
        if isinstance(v, (int, np.integer)):
            return ("const", int(v))
        if isinstance(v, (float, np.floating)):
            return ("const", float(v))
        raise TypeError(f"cannot compute with {type(v).__name__}: columns (E), ints and floats")

    def key(self) -> tuple:
        """The expression's structure as nested tuples: equal keys, same
        expression."""
        return self._key

    def __hash__(self) -> int:
        return hash(self._key)

    def columns(self) -> List[str]:
        """The source columns, each once, in order of first appearance."""
        out: Dict[str, None] = {}

        def walk(k):
            if k[0] == "col":
                out.setdefault(k[1])
            elif k[0] != "const":
                for x in k[1:]:
                    if isinstance(x, tuple):
                        walk(x)
        walk(self._key)
        return list(out)

    def __repr__(self) -> str:
        def show(k) -> str:
            if k[0] == "col":
                return k[1]
            if k[0] == "const":
                return repr(k[1])
            if k[0] in ("neg", "abs"):
                return ("-" if k[0] == "neg" else "abs") + "(" + show(k[1]) + ")"
            if k[0] in ("//", "%"):
                return f"({show(k[1])} {k[0]} {k[2]})"
            return f"({show(k[1])} {k[0]} {show(k[2])})"
        return "E[" + show(self._key) + "]"

    # arithmetic
    def _bin(self, op: str, other, swap: bool = False) -> "E":
        try:
            o = E._operand(other)
        except TypeError:
            return NotImplemented
        return E._of((op, o, self._key) if swap else (op, self._key, o))

    def __add__(self, o): return self._bin("+", o)                # noqa: E704
    def __radd__(self, o): return self._bin("+", o, True)         # noqa: E704
    def __sub__(self, o): return self._bin("-", o)                # noqa: E704
    def __rsub__(self, o): return self._bin("-", o, True)         # noqa: E704
    def __mul__(self, o): return self._bin("*", o)                # noqa: E704
    def __rmul__(self, o): return self._bin("*", o, True)         # noqa: E704
    def __truediv__(self, o): return self._bin("/", o)            # noqa: E704
    def __rtruediv__(self, o): return self._bin("/", o, True)     # noqa: E704
    def __neg__(self): return E._of(("neg", self._key))           # noqa: E704
    def __pos__(self): return self                                # noqa: E704
    def __abs__(self): return E._of(("abs", self._key))           # noqa: E704

    def _idiv(self, op: str, o) -> "E":
        if isinstance(o, (bool, np.bool_)) or not isinstance(o, (int, np.integer)):
            raise ValueError(f"{op} takes a positive Python int as its divisor, not {o!r}")
        if int(o) <= 0:
            raise ValueError(f"{op} {int(o)}: the divisor is a positive constant")
        return E._of((op, self._key, int(o)))

    def __floordiv__(self, o): return self._idiv("//", o)         # noqa: E704
    def __mod__(self, o): return self._idiv("%", o)               # noqa: E704

    def __rfloordiv__(self, o):
        raise ValueError("// takes a positive Python int as its divisor, not an expression")

    __rmod__ = __rfloordiv__

    # predicates, as on P
    def __eq__(self, v): return Pred(self, "==", v)               # noqa: E704
    def __ne__(self, v): return Pred(self, "!=", v)               # noqa: E704
    def __lt__(self, v): return Pred(self, "<", v)                # noqa: E704
    def __le__(self, v): return Pred(self, "<=", v)               # noqa: E704
    def __gt__(self, v): return Pred(self, ">", v)                # noqa: E704
    def __ge__(self, v): return Pred(self, ">=", v)               # noqa: E704

    def between(self, lo, hi) -> Pred:
        return Pred(self, "between", (lo, hi))

    def isin(self, values) -> Pred:
        return Pred(self, "in", tuple(values))

    def not_in(self, values) -> Pred:
        return Pred(self, "not in", tuple(values))

    def ranges(self, rs) -> Pred:
        return Pred(self, "ranges", tuple(tuple(r) for r in rs))

    def is_null(self) -> Pred:
        return Pred(self, "is_null")

    def is_valid(self) -> Pred:
        return Pred(self, "is_valid")


class ExprName(str):
    """The name an expression goes by where a scan keeps column names
    (``AggOut.aggs``, ``TopOut.column.name``): its text, with the expression
    itself in ``expr``."""

    expr: E

    def __new__(cls, e: E):
        s = super().__new__(cls, repr(e))
        s.expr = e
        return s


def name_of(x):
    """``x`` as a scan's column name: an ExprName for an expression."""
    if isinstance(x, ExprName):
        return x
    return ExprName(x) if isinstance(x, E) else x


# ------------------------------------------------------------ compilation
@dataclass
class Program:
    """One compiled expression: the kernel's postfix program and the
    synthetic column that describes its result."""
    expr: E
    domain: int                          # INT / FLT
    columns: List[str]                   # source columns, COL i names columns[i]
    types: List[int]                     # their STROM_COL_* storage types
    ops: List[Tuple[int, int, int]]      # (op, arg, imm as uint64 bits)
    depth: int
    column: Column                       # the result: int64 or float64

    def struct(self) -> "ExprStruct":
        s = ExprStruct()
        s.domain, s.nops, s.ncols = self.domain, len(self.ops), len(self.columns)
        for i, t in enumerate(self.types):
            s.col_type[i] = t
        for i, (op, arg, imm) in enumerate(self.ops):
            s.ops[i].op, s.ops[i].arg, s.ops[i].imm = op, arg, imm
        return s


class ExprOp(C.Structure):
    """struct strom_expr_op (strom.h)."""
    _fields_ = [("op", C.c_uint32), ("arg", C.c_uint32), ("imm", C.c_uint64)]


class ExprStruct(C.Structure):
    """struct strom_expr (strom.h)."""
    _fields_ = [("domain", C.c_uint32), ("nops", C.c_uint32), ("ncols", C.c_uint32),
                ("reserved", C.c_uint32), ("col_type", C.c_uint32 * MAX_COLS),
                ("ops", ExprOp * MAX_OPS)]


def _f64_bits(x: float) -> int:
    return int(np.float64(x).view(np.uint64))


def _fold(op: str, a, b=None):
    """A constant sub-tree's value, computed as the kernel would."""
    with np.errstate(all="ignore"):
        if isinstance(a, float) or isinstance(b, float) or op == "/":
            x, y = np.float64(a), (np.float64(b) if b is not None else None)
            r = {"+": lambda: x + y, "-": lambda: x - y, "*": lambda: x * y, "/": lambda: x / y,
                 "neg": lambda: -x, "abs": lambda: np.abs(x)}[op]()
            return float(r)
        # Python ints: exact; the range is checked where the constant is emitted
        return {"+": lambda: a + b, "-": lambda: a - b, "*": lambda: a * b, "neg": lambda: -a,
                "abs": lambda: abs(a), "//": lambda: a // b, "%": lambda: a % b}[op]()


def _simplify(k: tuple) -> tuple:
    """The tree with constant sub-trees folded."""
    if k[0] in ("col", "const"):
        return k
    if k[0] in ("neg", "abs"):
        a = _simplify(k[1])
        return ("const", _fold(k[0], a[1])) if a[0] == "const" else (k[0], a)
    if k[0] in ("//", "%"):
        a = _simplify(k[1])
        if a[0] == "const":
            if isinstance(a[1], float):
                raise ValueError(f"{k[0]} {k[2]} of the float constant {a[1]!r}: // and % are "
                                 "integer operations")
            return ("const", _fold(k[0], a[1], k[2]))
        return (k[0], a, k[2])
    a, b = _simplify(k[1]), _simplify(k[2])
    if a[0] == "const" and b[0] == "const":
        return ("const", _fold(k[0], a[1], b[1]))
    return (k[0], a, b)


def _has(k: tuple, what) -> bool:
    if what(k):
        return True
    return any(isinstance(x, tuple) and _has(x, what) for x in k[1:]) if k[0] not in \
        ("col", "const") else False


def compile_expr(e: E, schema, nulls=None) -> Program:
    """The kernel program of ``e`` over ``schema`` (a list of Column or a
    name -> Column mapping).  ``nulls(name)`` tells whether the file has
    nulls in a column (default: the column's own ``nullable``): the result is
    nullable iff a source column has."""
    if not isinstance(e, E):
        raise TypeError("compile_expr: an E expression")
    if not isinstance(schema, dict):
        schema = {c.name: c for c in schema}
    names = e.columns()
    if not names:
        raise ValueError(f"{e!r}: an expression names at least one column")
    if len(names) > MAX_COLS:
        raise ValueError(f"{e!r}: {len(names)} source columns {names} (at most {MAX_COLS})")
    cols = []
    for n in names:
        if n not in schema:
            raise ValueError(f"no column {n!r}")
        c = schema[n]
        kind = "dictionary-encoded" if c.dictionary is not None else c.kind
        if c.dictionary is not None or c.kind not in ("int", "float") or \
                c.storage not in _INT_SRC + _FLT_SRC:
            what = "uint64" if (c.dictionary is None and c.kind == "int") else kind
            raise ValueError(f"{e!r}: source column {n} is {what}: int8-int64, uint8-uint32 and "
                             "float32/64 columns are computed with")
        cols.append(c)
    tree = _simplify(e.key())
    flt = any(c.storage in _FLT_SRC for c in cols) or \
        _has(tree, lambda k: k[0] == "/" or (k[0] == "const" and isinstance(k[1], float)))
    if flt:
        bad = []
        _has(tree, lambda k: bad.append(k[0]) if k[0] in ("//", "%") else False)
        if bad:
            raise ValueError(f"{e!r}: {bad[0]} in a float64 expression (a float source column, a "
                             "float constant or /): // and % are integer operations")
    ops: List[Tuple[int, int, int]] = []
    depth = [0, 0]                      # now, the most

    def push():
        depth[0] += 1
        depth[1] = max(depth[1], depth[0])

    def emit(k: tuple) -> None:
        if k[0] == "col":
            ops.append((XOP_COL, names.index(k[1]), 0))
            push()
        elif k[0] == "const":
            v = k[1]
            if flt:
                imm = _f64_bits(float(v))
            else:
                if not -(1 << 63) <= v < (1 << 63):
                    raise ValueError(f"{e!r}: the integer constant {v} is outside int64")
                imm = v & 0xFFFFFFFFFFFFFFFF
            ops.append((XOP_CONST, 0, imm))
            push()
        elif k[0] in ("neg", "abs"):
            emit(k[1])
            ops.append((XOP_NEG if k[0] == "neg" else XOP_ABS, 0, 0))
        elif k[0] in ("//", "%"):
            emit(k[1])
            if not 0 < k[2] < (1 << 63):
                raise ValueError(f"{e!r}: the divisor {k[2]} is outside (0, 2^63)")
            ops.append((XOP_FDIV if k[0] == "//" else XOP_MOD, 0, k[2]))
        else:
            emit(k[1])
            emit(k[2])
            ops.append((_BIN[k[0]], 0, 0))
            depth[0] -= 1
    emit(tree)
    if depth[1] > MAX_DEPTH:
        raise ValueError(f"{e!r}: an operand stack of depth {depth[1]} (at most {MAX_DEPTH}); "
                         "put the deeper operand of an operator on its left")
    if len(ops) > MAX_OPS:
        raise ValueError(f"{e!r}: {len(ops)} ops after folding constants (at most {MAX_OPS})")
    nulls = nulls if nulls is not None else (lambda n: bool(schema[n].nullable))
    column = Column(ExprName(e), "float" if flt else "int", 64, True,
                    nullable=any(nulls(n) for n in names))
    return Program(e, FLT if flt else INT, names, [COL_CODE[c.storage] for c in cols], ops,
                   depth[1], column)


# ------------------------------------------------------------ numpy twin
def host_expr(program: Program, values: Sequence, valids: Sequence, n: int):
    """The kernel's result for n rows on the host: ``values[i]`` /
    ``valids[i]`` (a bool array, or None: no nulls) belong to
    ``program.columns[i]``.  Returns (int64 or float64 values, validity or
    None when no source has any); null rows hold 0."""
    flt = program.domain == FLT
    dt = np.float64 if flt else np.int64
    src = [np.asarray(v[:n]).astype(dt) for v in values]
    ok = None
    for v in valids:
        if v is not None:
            b = np.asarray(v[:n], bool)
            ok = b.copy() if ok is None else ok & b
    stack: List[np.ndarray] = []
    with np.errstate(all="ignore"):
        for op, arg, imm in program.ops:
            if op == XOP_COL:
                stack.append(src[arg])
            elif op == XOP_CONST:
                c = np.uint64(imm).view(dt)
                stack.append(np.full(n, c, dt))
            elif op == XOP_NEG:
                stack.append(np.negative(stack.pop()))
            elif op == XOP_ABS:
                stack.append(np.abs(stack.pop()))
            elif op == XOP_FDIV:
                stack.append(np.floor_divide(stack.pop(), np.int64(imm)))
            elif op == XOP_MOD:
                stack.append(np.remainder(stack.pop(), np.int64(imm)))
            else:
                b, a = stack.pop(), stack.pop()
                f = {XOP_ADD: np.add, XOP_SUB: np.subtract, XOP_MUL: np.multiply,
                     XOP_DIV: np.divide}[op]
                stack.append(f(a, b))
    out = np.array(stack.pop(), dtype=dt, copy=True)
    if flt:
        out.view(np.uint64)[np.isnan(out)] = np.uint64(NAN_BITS)
    if ok is not None:
        out[~ok] = 0
    return out, ok


# ------------------------------------------------------------ device launch
def expr_batched(program: Program, src_tabs, nwords: int, out_tab, sel=None, stream=None) -> None:
    """One launch of the expression kernel: ``src_tabs`` the device batch
    tables of the source columns, int64 (ncols, nbatches, 5); ``out_tab``
    (nbatches, 5) the table of the 8-byte result rows and their validity
    words; ``sel`` an optional selection bitmap whose zero words are not
    evaluated (their validity words become 0)."""
    from ._util import check, lib, ptr, require_cuda, stream_handle
    from .colfilter import BATCH_FIELDS
    require_cuda(src_tabs, "src_tabs")
    require_cuda(out_tab, "out_tab")
    nc = len(program.columns)
    if src_tabs.dim() != 3 or src_tabs.shape[0] != nc or src_tabs.shape[2] != BATCH_FIELDS:
        raise ValueError(f"src_tabs: int64 ({nc}, nbatches, {BATCH_FIELDS})")
    if out_tab.dim() != 2 or tuple(out_tab.shape) != tuple(src_tabs.shape[1:]):
        raise ValueError("out_tab: int64 (nbatches, 5) of the same batches")
    if sel is not None and sel.numel() < nwords:
        raise ValueError("sel too small")
    s = program.struct()
    check(lib().strom_column_expr(C.byref(s), ptr(src_tabs), src_tabs.shape[1], nwords,
                                  ptr(sel) if sel is not None else 0, ptr(out_tab),
                                  stream_handle(stream)), "column_expr")
