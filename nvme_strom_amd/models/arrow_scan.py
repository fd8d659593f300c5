"""PG-Strom-style SSD→GPU direct scan of an Apache Arrow IPC file
(BASELINE config 5): only the scanned column's buffers travel storage → HBM
through the engine, are LZ4-decoded and filtered on the GPU, and the
selected row ids are appended on the device — one host sync per scan.

Pipeline (a ring of ``nslots`` HBM slots, groups of record batches):

    host:   plan groups from the footer / batch headers (utils/arrow_ipc.py):
            per batch the column's data (+ validity when it has nulls)
            buffer ranges -> the file chunks that cover them
    group g:  MEMCPY_SSD2GPU(chunk ids of g) -> slot g % nslots      (engine)
              WAIT(g) ; then on the slot's stream, no host sync:
                decode  one launch over every compressed buffer of g
                        (Arrow BodyCompression LZ4_FRAME: the length prefix and
                        frame header are parsed on the device);
                        status vs expected sizes -> device error counter
                filter  one launch over every batch of g (validity ANDed in,
                        each batch on fresh bitmap words), count on device
                emit    global row ids appended at a device-side cursor, on one
                        emit stream in group order (decode/filter of several
                        groups run concurrently on their slots' streams)
              event(g) ; the slot is refilled only after event(g)
    while group g computes, group g+1 is already being read.

Unreferenced columns are never read; files larger than HBM stream through
the ring.  The reference has no columnar path (new MI355X
work); its chunk-list I/O (MEMCPY_SSD2GPU with arbitrary chunk ids,
kmod/nvme_strom.c:1488-1604) is what fetches the scattered buffers.
"""
from __future__ import annotations

import gc
import os
import struct
import time
from dataclasses import dataclass, field, replace
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .. import api
from ..ops import colagg as A
from ..ops import colgroup as G
from ..ops import coljoin as J
from ..ops import colproject as PJ
from ..ops import colsort as SO
from ..ops import coltopk as T
from ..ops import decompress as D
from ..ops.colexpr import E, ExprName, Program, compile_expr, expr_batched, host_expr, name_of
from ..ops.colfilter import BATCH_FIELDS, bitmap_to_rows, bitmap_to_rows_str
from ..ops.colpred import (COL_CODE, QUAL_BATCH_FIELDS, Compiled, Pred, clauses, compile_pred,
                           evaluate, qual_batched)
from ..ops.reorder import chunk_scatter, landing_positions
from ..tensor import FileReader, HbmBuffer, host_buffer
from ..utils.arrow_ipc import (ArrowFile, Column, ColumnArrays, _Src, decode_values,
                               dictionary_values, read_buffer, read_metadata, validity_bits)

# projection output dtypes by storage (date/time/timestamp/duration: their
# integer ticks; dictionary-encoded: the indices)
_TORCH = {"i1": torch.int8, "u1": torch.uint8, "i2": torch.int16, "u2": torch.uint16,
          "i4": torch.int32, "u4": torch.uint32, "i8": torch.int64, "u8": torch.uint64,
          "f4": torch.float32, "f8": torch.float64}


class JoinAttr:
    """One attribute of a JoinTable (``dim["category"]``): what ``by=`` and
    ``project=`` name to group by or gather the joined attribute."""

    def __init__(self, table: "JoinTable", name: str):
        self.table, self.name = table, name

    @property
    def values(self) -> list:
        """The value of each code (None: the attribute was null)."""
        return self.table._attrs[self.name][0]

    @property
    def codes(self) -> np.ndarray:
        """The code of each build row (int32)."""
        return self.table._attrs[self.name][1]

    def __repr__(self) -> str:
        return f"JoinAttr({self.name!r})"


def _pylist(x) -> list:
    if hasattr(x, "to_pylist"):
        return x.to_pylist()
    if isinstance(x, np.ndarray):
        return x.tolist()
    return list(x)


class JoinTable:
    """The build side of a join: a dimension table's unique integer key and
    any number of attributes, one value per key.

    ``keys``: an integer numpy or pyarrow array; null keys are dropped with
    their attribute values (they never match).  ``attrs``: name -> strings,
    integers or bools, factorized on the host into codes 0..m-1 in order of
    first appearance; a null value is one ordinary code whose value is None.
    ``device``: where the hash tables (csrc/kernels/coljoin.hip) are built —
    one per attribute, its payload the attribute's code, and one whose
    payload is the build row; None keeps the table on the host (the CPU
    twins).  A key that appears twice raises ValueError after the build.  An
    empty table is legal.  Built once, usable by any number of scans on its
    device; ``close()`` frees it."""

    def __init__(self, keys, attrs: Optional[dict] = None, device=None):
        valid = None
        if hasattr(keys, "to_numpy") and hasattr(keys, "null_count"):      # pyarrow
            if hasattr(keys, "combine_chunks"):
                keys = keys.combine_chunks()
            if keys.null_count:
                valid = np.asarray(keys.is_valid())
                keys = keys.fill_null(0)
            keys = keys.to_numpy(zero_copy_only=False)
        keys = np.asarray(keys)
        if keys.ndim != 1 or keys.dtype.kind not in "iu":
            raise ValueError("JoinTable keys: a one-dimensional integer array")
        if keys.dtype == np.uint64 and len(keys) and int(keys.max()) >= 1 << 63:
            raise ValueError("JoinTable keys: values >= 2^63 are not int64 keys")
        nall = len(keys)
        keys = keys.astype(np.int64)
        self.keys = keys if valid is None else keys[valid]
        self._attrs: Dict[str, tuple] = {}
        for name, vals in (attrs or {}).items():
            vals = _pylist(vals)
            if len(vals) != nall:
                raise ValueError(f"attribute {name}: {len(vals)} values for {nall} keys")
            if valid is not None:
                vals = [v for v, ok in zip(vals, valid) if ok]
            code: Dict[object, int] = {}
            # bools and integers are different attribute values (True != 1)
            codes = np.fromiter((code.setdefault((type(v) is bool, v), len(code)) for v in vals),
                                np.int32, len(vals))
            self._attrs[str(name)] = ([v for _, v in code], codes)
        self.device = torch.device(device) if device is not None else None
        self._host: Optional[J.HostTable] = None
        self._dev: Dict[Optional[str], J.DeviceTable] = {}
        self._dkeys = None
        if self.device is not None:
            # every table now, so that no scan builds (and syncs for) one
            for name in [None] + list(self._attrs):
                self._device_table(name)
            dups = int(self._dev[None].header()[J.H_DUPS])
        else:
            dups = self.host().dups
        if dups:
            self.close()
            raise ValueError(f"JoinTable: {dups} duplicate key(s): the dimension's key must be "
                             "unique")

    def __len__(self) -> int:
        return len(self.keys)

    def __getitem__(self, name: str) -> JoinAttr:
        if name not in self._attrs:
            raise ValueError(f"JoinTable has no attribute {name!r}")
        return JoinAttr(self, name)

    def host(self) -> J.HostTable:
        """The numpy twin's table (payload: the build row)."""
        if self._host is None:
            self._host = J.host_build(self.keys)
        return self._host

    def _device_table(self, attr: Optional[str]) -> J.DeviceTable:
        if self.device is None:
            raise ValueError("JoinTable was built without a device")
        if attr not in self._dev:
            if self._dkeys is None:
                self._dkeys = torch.from_numpy(self.keys).to(self.device)
            pay = None
            if attr is not None:
                pay = torch.from_numpy(self._attrs[attr][1]).to(self.device)
            with torch.cuda.device(self.device):
                self._dev[attr] = J.build(self._dkeys, pay)
                self._dev[attr].keep = pay
                # the scans probe on their own streams
                torch.cuda.current_stream(self.device).synchronize()
        return self._dev[attr]

    def close(self) -> None:
        self._dev = {}
        self._dkeys = None


class Join:
    """``join=Join("fk", dim, how="semi")``: keep the rows whose ``fk`` is a
    key of ``dim`` (``how="anti"``: the rows whose ``fk`` is not; a null fk
    matches nothing, so the anti-join keeps it, as pyarrow's "left anti").
    ``fk`` is a stored column: an expression (ops/colexpr.E) is refused."""

    def __init__(self, col: str, table: JoinTable, how: str = "semi"):
        if how not in J.HOW:
            raise ValueError(f"join how={how!r}: one of {sorted(J.HOW)}")
        if not isinstance(table, JoinTable):
            raise TypeError("Join: the build side is a JoinTable")
        if isinstance(col, E):
            raise NotImplementedError(f"join on {col!r}: a computed column is not a join key "
                                      "(stored integer columns are)")
        self.col, self.table, self.how = str(col), table, how


class StarJoin:
    """``join=StarJoin(Join("cust", customers), Join("part", parts, "anti"), ...)``:
    a star join, one to four Join legs applied in one probe launch per group
    (strom_column_join_star): a row is kept if every leg keeps it.  The result
    does not depend on the order of the legs; the order is the probe order, and
    a row an earlier leg dropped costs the later ones nothing, so the most
    selective leg goes first.  The fk columns may differ in type; a column or a
    JoinTable may serve several legs.  ``dim[attr]`` in ``project=`` / ``by=`` /
    ``HashBy([...])`` belongs to the one semi leg whose table is ``dim``."""

    def __init__(self, *joins):
        if len(joins) == 1 and isinstance(joins[0], (list, tuple)):
            joins = tuple(joins[0])
        if not joins:
            raise ValueError("StarJoin: at least one Join leg")
        if len(joins) > J.MAX_LEGS:
            raise NotImplementedError(f"StarJoin of {len(joins)} legs: at most {J.MAX_LEGS} tables "
                                      "are probed in one pass")
        for j in joins:
            if not isinstance(j, Join):
                raise TypeError("StarJoin: every leg is a Join")
        self.legs: Tuple[Join, ...] = tuple(joins)

    def __repr__(self) -> str:
        return "StarJoin(" + ", ".join(f"{j.col} {j.how}" for j in self.legs) + ")"


def _legs(join) -> Tuple[Join, ...]:
    """The legs of a checked ``join=``: none, the one Join, a StarJoin's."""
    if join is None:
        return ()
    return join.legs if isinstance(join, StarJoin) else (join,)


def _leg_of(join, attr: JoinAttr) -> int:
    """The leg whose table carries ``attr`` (checked by _check_join)."""
    return next(i for i, j in enumerate(_legs(join)) if j.table is attr.table)


class HashBy:
    """``by=HashBy("customer_id", groups=1 << 20)``: GROUP BY an ordinary
    integer column (int8-int64, uint8-uint64 over its whole range, or a date /
    time / timestamp / duration column by its ticks) through a hash table in
    HBM (csrc/kernels/colgroup.hip) instead of the key-indexed accumulators
    in LDS that ``by="name"`` uses.  ``groups``: the largest number of
    distinct non-null keys the scan may meet, 1 <= groups <= 2^24; the table
    gets the next power of two >= 2 * groups slots and is not grown: a scan
    that meets more keys raises RuntimeError at its one sync.

    ``HashBy(["region", "day"], groups)`` — a list or tuple, also of one — is
    ``GROUP BY region, day``: up to four components, each such a column or
    an attribute of a semi-join leg of the scan (``dim["category"]``: one per
    JoinTable, of different tables with ``join=StarJoin(...)``), packed into
    the table's one 64-bit key word (ops/colgroup.KeySpec).  A column takes
    its storage width, one bit more when any record batch of the file has
    nulls in it; an attribute takes ceil(log2(number of its values)) bits.
    All widths together must fit 64 bits: ``bits={"col": n}`` declares that
    ``col``'s values lie in [-2^(n-1), 2^(n-1)) (signed) or [0, 2^n); a
    selected row outside that range raises RuntimeError at the sync.
    ``groups`` counts distinct tuples.  Rows come back in lexicographic
    order, each column ascending, nulls last (an attribute by its code).

    A key or a component may be an int64 expression (ops/colexpr.E:
    ``HashBy(E("ts_ms") // 86_400_000, groups)``), computed on the device per
    group before the table is probed; as a component it takes 64 bits (65 when
    a source column has nulls) unless ``bits={expr: n}`` declares fewer."""

    def __init__(self, col, groups: int = 1 << 16, bits: Optional[dict] = None):
        self.groups = G.check_groups(groups)
        self.comps: Optional[list] = None
        self.bits: Dict[str, int] = {}
        if isinstance(col, (list, tuple)):
            comps = list(col)
            if not comps:
                raise ValueError("HashBy: an empty list of key columns")
            if len(comps) > G.MAX_KEYS:
                raise NotImplementedError(f"HashBy of {len(comps)} components: at most "
                                          f"{G.MAX_KEYS} are packed into the 64-bit key")
            comps = [c if isinstance(c, (JoinAttr, ExprName)) else
                     (name_of(c) if isinstance(c, E) else str(c)) for c in comps]
            names = [("attr", id(c.table), c.name) if isinstance(c, JoinAttr) else ("col", c)
                     for c in comps]
            for n in names:
                if names.count(n) > 1:
                    raise ValueError(f"HashBy: {n[-1]!r} appears twice")
            tabs = [id(c.table) for c in comps if isinstance(c, JoinAttr)]
            if len(set(tabs)) < len(tabs):
                raise NotImplementedError("HashBy: one JoinTable attribute per JoinTable (the "
                                          "probe writes one attribute's codes per leg)")
            cols = [c for c in comps if not isinstance(c, JoinAttr)]
            for n, b in (bits or {}).items():
                n = name_of(n)
                if n not in cols:
                    raise ValueError(f"bits= names {n!r}, which is not a column of the key")
                if isinstance(b, bool) or int(b) != b or not 1 <= int(b) <= 64:
                    raise ValueError(f"bits={b!r} for {n}: 1 <= bits <= its storage width")
                self.bits[n] = int(b)
            self.comps = comps
            # a name that two components carry (attributes of different tables,
            # or an attribute and a column) is qualified by its position
            plain = [c.name if isinstance(c, JoinAttr) else c for c in comps]
            self.col = tuple(f"{n}[{i}]" if plain.count(n) > 1 and isinstance(c, JoinAttr) else n
                             for i, (n, c) in enumerate(zip(plain, comps)))
        else:
            if bits:
                raise ValueError("bits= belongs to a list of key columns")
            self.col = name_of(col) if isinstance(col, (E, ExprName)) else str(col)

    @property
    def attrs(self) -> List[JoinAttr]:
        """The JoinTable attributes among the components."""
        return [c for c in self.comps or [] if isinstance(c, JoinAttr)]

    def __repr__(self) -> str:
        if self.comps is not None:
            return f"HashBy({self.comps!r}, groups={self.groups}" + \
                (f", bits={self.bits}" if self.bits else "") + ")"
        return f"HashBy({self.col!r}, groups={self.groups})"


def _check_join(meta: ArrowFile, join, attrs):
    """Validate ``join=`` (a Join, a StarJoin or None) and the JoinAttrs of
    ``by=`` / ``project=`` (one, a list or None) against the schema."""
    attrs = [] if attrs is None else ([attrs] if isinstance(attrs, JoinAttr) else list(attrs))
    if isinstance(join, (list, tuple)):
        raise NotImplementedError("one join per scan (a list of joins is not supported; "
                                  "join=StarJoin(...) probes several tables in one pass)")
    if join is None:
        if attrs:
            raise ValueError(f"{attrs[0]!r} needs join= with its JoinTable")
        return None
    if not isinstance(join, (Join, StarJoin)):
        raise TypeError("join=: a Join or a StarJoin")
    schema = {c.name: c for c in meta.schema}
    for leg in _legs(join):
        if leg.col not in schema:
            raise ValueError(f"no column {leg.col!r}")
        c = schema[leg.col]
        if c.dictionary is not None or c.kind != "int" or c.storage not in J.FK_CODE:
            kind = "dictionary-encoded" if c.dictionary is not None else c.kind
            raise NotImplementedError(f"join on {leg.col}: {kind} columns are not joined "
                                      "(integer columns are)")
    for attr in attrs:
        mine = [leg for leg in _legs(join) if leg.table is attr.table]
        if not mine:
            raise ValueError(f"{attr!r} belongs to another JoinTable than the one in join=")
        if len(mine) > 1:
            raise ValueError(f"{attr!r} is ambiguous: its JoinTable is in {len(mine)} legs of "
                             "the StarJoin (on " + ", ".join(leg.col for leg in mine) + ")")
        if mine[0].how == "anti":
            raise ValueError(f"{attr!r} with how='anti': the rows an anti-join keeps matched "
                             "nothing")
    return join


MAX_EXPRS = 4          # computed columns per scan: 8 B of slot memory per row each


class _ExprMeta:
    """A file's metadata with a scan's computed columns appended: their
    synthetic Columns behind the schema's, and per expression a ColumnArrays
    whose null counts are its source columns' added up (nulls somewhere in the
    file, batch by batch).  Everything else is the file's.  The validators
    (_agg_spec, _top_spec, _key_spec, compile_pred) then see a computed column
    as they see a stored int64 / float64 one."""

    def __init__(self, meta: ArrowFile, progs: Dict[str, Program]):
        self._meta, self.progs = meta, progs
        self.schema = list(meta.schema) + [p.column for p in progs.values()]
        self.columns = list(meta.columns)
        for p in progs.values():
            src = [meta.columns[meta.column_index(n)] for n in p.columns]
            self.columns.append(ColumnArrays(
                src[0].length, sum(np.asarray(a.null_count, np.int64) for a in src),
                src[0].v_off, src[0].v_len, src[0].d_off, src[0].d_len))

    def __getattr__(self, name):
        return getattr(self._meta, name)

    def column_index(self, name: str) -> int:
        for i, c in enumerate(self.schema):
            if c.name == name:
                return i
        raise KeyError(name)


def _named_clauses(quals) -> List[List[Pred]]:
    """clauses(quals) with every expression a predicate is on by its name."""
    return [[replace(p, col=name_of(p.col)) if isinstance(p.col, E) else p for p in c]
            for c in clauses(quals)]


def _with_exprs(meta: ArrowFile, names) -> ArrowFile:
    """``meta``, or an _ExprMeta over it when ``names`` (the column names of a
    query, expressions as ExprName) hold computed columns: each distinct
    expression compiled once."""
    progs: Dict[str, Program] = {}
    schema = {c.name: c for c in meta.schema}
    for n in names:
        if not isinstance(n, ExprName) or n in progs:
            continue
        if n in schema:
            raise ValueError(f"the file has a column named {str(n)!r}: the expression cannot go "
                             "by that name")
        if len(progs) == MAX_EXPRS:
            raise ValueError(f"more than {MAX_EXPRS} computed columns in one scan")
        progs[n] = compile_expr(n.expr, schema, nulls=lambda c: _file_nulls(meta, c))
    return _ExprMeta(meta, progs) if progs else meta


def _split_names(meta, names: List[str]) -> Tuple[List[str], List[str]]:
    """(the stored columns a scan reads — ``names`` without the computed
    columns, then their source columns —, those followed by the computed
    columns: the index of a name there is its column number in the scan)."""
    progs = getattr(meta, "progs", None)
    if not progs:
        return names, names
    stored = [n for n in names if n not in progs]
    for p in progs.values():
        stored += [c for c in p.columns if c not in stored]
    return stored, stored + list(progs)


@dataclass
class ProjOut:
    """One column of a select list (``scan_where(quals, project=[...])``):
    the fields of a single projection's ScanOut, per column.  Device tensors
    from ArrowScan.scan_where, numpy arrays of the same layout from the host
    twin."""
    name: str
    values: object                # one value per selected row (utf8/binary: the characters)
    valid: object = None          # uint8 0/1 per selected row when the column may hold nulls
    column: Optional[Column] = None   # the column's type; None: an attribute of a JoinTable
    dictionary: object = None     # decoded dictionary / the attribute's value per code
    offsets: object = None        # utf8/binary: int64[selected + 1] into ``values``


def _select_items(project) -> list:
    """The items of a list ``project=`` checked among themselves: column
    names (expressions as ExprName) and JoinAttrs, in the order given."""
    items = list(project)
    if not items:
        raise ValueError("project=[]: an empty select list (project=None selects the row ids)")
    if len(items) > PJ.MAX_COLS:
        raise NotImplementedError(f"a select list of {len(items)} columns: at most "
                                  f"{PJ.MAX_COLS} are gathered in one emit pass")
    out = []
    for it in items:
        if isinstance(it, JoinAttr):
            out.append(it)
        elif isinstance(it, (str, E)):
            out.append(name_of(it))
        else:
            raise TypeError(f"project=[...]: {it!r} is no column name, expression or dim[attr]")
    keys = [("attr", id(c.table), c.name) if isinstance(c, JoinAttr) else ("col", str(c))
            for c in out]
    for k in keys:
        if keys.count(k) > 1:
            raise ValueError(f"project=[...]: {k[-1]!r} appears twice")
    tabs = [id(c.table) for c in out if isinstance(c, JoinAttr)]
    if len(set(tabs)) < len(tabs):
        raise NotImplementedError("project=[...]: one attribute per JoinTable (the probe writes "
                                  "one attribute's codes per leg)")
    return out


def _select_meta(xm, items: list) -> List[Optional[Column]]:
    """The Column of each item of a select list (None: a JoinAttr), every
    kind checked before anything is read: what a single projection takes,
    and bool columns."""
    schema = {c.name: c for c in xm.schema}
    metas = []
    for it in items:
        if isinstance(it, JoinAttr):
            metas.append(None)
            continue
        if it not in schema:
            raise ValueError(f"no column {str(it)!r}")
        c = schema[it]
        strings = c.kind in ("utf8", "binary") and c.dictionary is None
        if not c.supported or not (strings or c.storage in _TORCH or c.storage in ("d16", "b1")):
            raise NotImplementedError(f"projection of {it} ({c.kind}): fixed-width, bool, "
                                      "utf8/binary or dictionary-encoded columns")
        metas.append(c)
    return metas


def _arrow_type(c: Column):
    import pyarrow as pa
    if c.kind in ("utf8", "binary"):
        return {("utf8", False): pa.utf8(), ("utf8", True): pa.large_utf8(),
                ("binary", False): pa.binary(), ("binary", True): pa.large_binary()}[
                    (c.kind, bool(c.large))]
    if c.kind == "bool":
        return pa.bool_()
    if c.kind == "decimal":
        return pa.decimal128(c.precision, c.scale)
    if c.kind == "date":
        return pa.date32() if c.unit == "d" else pa.date64()
    if c.kind == "time":
        return pa.time32(c.unit) if c.bit_width == 32 else pa.time64(c.unit)
    if c.kind == "timestamp":
        return pa.timestamp(c.unit, tz=c.tz or None)
    if c.kind == "duration":
        return pa.duration(c.unit)
    return pa.from_numpy_dtype(np.dtype(Column(c.name, c.kind, c.bit_width, c.signed).storage))


def _arrow_array(c: Column, values: np.ndarray, valid, offsets=None):
    """The pyarrow array of a column's gathered buffers (numpy, the layout of
    ProjOut; ``c`` without its dictionary describes the values)."""
    import pyarrow as pa
    typ = _arrow_type(c)
    if offsets is not None:
        n = len(offsets) - 1
        ot = np.int64 if c.large else np.int32
        bufs = [pa.py_buffer(np.ascontiguousarray(offsets, dtype=ot)),
                pa.py_buffer(np.ascontiguousarray(values, dtype=np.uint8))]
    elif c.kind == "bool":
        n = len(values)
        bufs = [pa.py_buffer(np.packbits(np.asarray(values, np.uint8) != 0, bitorder="little"))]
    else:
        n = len(values)
        bufs = [pa.py_buffer(np.ascontiguousarray(values))]
    vbuf, nulls = None, 0
    if valid is not None:
        ok = np.asarray(valid) != 0
        nulls = int(len(ok) - ok.sum())
        if nulls:
            vbuf = pa.py_buffer(np.packbits(ok, bitorder="little"))
    return pa.Array.from_buffers(typ, n, [vbuf] + bufs, null_count=nulls)


def _arrow_table(cols: List[ProjOut]):
    """A pyarrow.Table of a select list's columns (numpy buffers), the
    column types restored from the Column metadata."""
    import pyarrow as pa
    arrays, fields = [], []
    for p in cols:
        c = p.column
        if c is None:
            # dim[attr]: a dictionary array over the attribute's values
            arr = pa.DictionaryArray.from_arrays(pa.array(np.asarray(p.values, np.int32)),
                                                 pa.array(list(p.dictionary)))
            nullable = True
        elif c.dictionary is not None:
            dv, dok = p.dictionary
            vc = replace(c, dictionary=None)
            if isinstance(dv, tuple):
                darr = _arrow_array(vc, dv[1], dok, offsets=dv[0])
            else:
                darr = _arrow_array(vc, np.asarray(dv), dok)
            idx = _arrow_array(Column(c.name, "int", c.dictionary.index_bits,
                                      c.dictionary.index_signed), p.values, p.valid)
            arr = pa.DictionaryArray.from_arrays(idx, darr, ordered=c.dictionary.ordered)
            nullable = c.nullable
        else:
            arr = _arrow_array(c, p.values, p.valid, p.offsets)
            nullable = True if isinstance(c.name, ExprName) else c.nullable
        arrays.append(arr)
        fields.append(pa.field(str(p.name), arr.type, nullable=nullable))
    return pa.Table.from_arrays(arrays, schema=pa.schema(fields))


def _to_host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


@dataclass
class ScanOut:
    rows: int
    selected: int
    indices: torch.Tensor
    seconds: Dict[str, float]
    bytes_read: int = 0           # file bytes moved storage -> HBM
    column_bytes: int = 0         # decoded bytes of the scanned columns
    groups: int = 0
    values: Optional[torch.Tensor] = None   # projected column, one value per selected row
    valid: Optional[torch.Tensor] = None    # its validity (uint8 0/1) when it has nulls
    column: Optional[Column] = None         # the projected column's type (units, tz, ...)
    dictionary: object = None               # its decoded dictionary when dictionary-encoded
    offsets: Optional[torch.Tensor] = None  # utf8/binary projection: int64[selected + 1]
                                            # into ``values`` (the characters, uint8)
    exprs: list = field(default_factory=list)   # the computed columns' Programs
    # project=[...]: one ProjOut per item, in the order given (values / valid /
    # column / dictionary / offsets above are then None)
    columns: Optional[List[ProjOut]] = None
    # order_by=: the normalized [(name, descending)] (None: file order), and
    # the gather's error word (device, uint64 as int64: permutation entries
    # that named no row; 0 unless the sort is broken), read by to_arrow
    order: Optional[List[Tuple[str, bool]]] = None
    sort_errors: Optional[torch.Tensor] = None

    def to_arrow(self):
        """The selected rows as a pyarrow.Table: the select list's columns
        (or the one projected column), one device -> host copy per buffer,
        the types restored from the file's schema: temporal units and time
        zone, decimal128(p, s) from the (lo, hi) words, dictionary columns as
        DictionaryArrays, utf8 / large_utf8 / binary from offsets and
        characters, ``dim[attr]`` as a dictionary array over the attribute's
        values, expressions as int64 / float64."""
        cols = self.columns
        if self.sort_errors is not None and int(self.sort_errors.item()):
            raise RuntimeError(f"sort: {int(self.sort_errors.item())} permutation entries named "
                               "no row")
        if cols is None:
            if self.values is None:
                raise ValueError("to_arrow: the scan projected no column")
            name = self.column.name if self.column is not None else "attr"
            cols = [ProjOut(name, self.values, self.valid, self.column, self.dictionary,
                            self.offsets)]
        return _arrow_table([ProjOut(p.name, _to_host(p.values), _to_host(p.valid), p.column,
                                     p.dictionary, _to_host(p.offsets)) for p in cols])


@dataclass
class _SelItem:
    """One column of a select list as _compute and _emit see it."""
    kind: int                     # ops/colproject FIXED / BOOL / STR32 / STR64
    width: int
    pcol: Optional[int] = None    # plan column; None: a join attribute's codes, in
    buf: int = -1                 # ... the slot's key buffer (-1) or leg buffer ``buf``
    out: Optional[torch.Tensor] = None
    valid: Optional[torch.Tensor] = None
    chars: Optional[torch.Tensor] = None
    cursor: Optional[torch.Tensor] = None     # view of one word of the scan's cursors


@dataclass
class _SelRun:
    """A scan's select list: its columns and their kernel descriptors."""
    items: List[_SelItem]
    cols: np.ndarray              # ops/colproject.proj_cols, tables filled in per group


@dataclass
class _LegRun:
    """One leg of a scan's join as _compute sees it."""
    col: int                      # plan column of the foreign key
    code: int                     # its STROM_COL_* storage type
    how: str
    dev: J.DeviceTable
    attr: Optional[str] = None    # attribute whose codes the probe writes
    buf: int = -1                 # star: which of the slot's leg buffers takes them


@dataclass
class _JoinRun:
    """A scan's join as _compute sees it: one leg (join=Join: the
    strom_column_join path) or a StarJoin's, all in one launch."""
    legs: List[_LegRun]
    star: bool = False


@dataclass
class _HashRun:
    """A scan's hash GROUP BY as _compute sees it."""
    col: int                      # plan column of the key
    code: int                     # its STROM_COL_* storage type
    dev: G.DeviceGroups
    # a composite key (dev.spec): the plan column of each component, None for
    # a join attribute, whose codes the probe leaves in the slot's key buffer
    # (join=Join) or in the leg buffer ``bufs`` names (join=StarJoin)
    cols: Optional[List[Optional[int]]] = None
    bufs: Optional[List[int]] = None


@dataclass
class _TopRun:
    """A scan's ORDER BY ... LIMIT k as _compute sees it."""
    col: int                      # plan column of the order column
    code: int                     # its STROM_COL_* storage type
    descending: bool
    state: T.State                # the k best so far (device; merged on the emit stream)
    pcol: Optional[int] = None    # plan column carried with each candidate
    pwidth: int = 0               # its bytes per row
    pattr: bool = False           # carry the joined attribute's codes instead


@dataclass
class _ExprRun:
    """One computed column of a scan as _compute sees it."""
    prog: Program
    cols: List[int]               # plan columns of its sources
    early: bool                   # a qualifier reads it: evaluated before the filter


@dataclass
class _Run:
    """One scan as _compute's stages see it: its totals over the groups and
    where its results go.  A stage whose field is None is not called."""
    count: torch.Tensor           # selected rows so far (device)
    err: torch.Tensor             # failed decodes so far (device)
    wait_s: float = 0.0
    bytes_read: int = 0
    column_bytes: int = 0
    marks: list = field(default_factory=list)    # (group, event, clock)
    join: Optional[_JoinRun] = None
    hash: Optional[_HashRun] = None
    top: Optional[_TopRun] = None
    exprs: List[_ExprRun] = field(default_factory=list)   # column len(names) + j each
    # rows (scan_where): the row ids and the projection behind their cursors
    out: Optional[torch.Tensor] = None
    cursor: Optional[torch.Tensor] = None
    ccursor: Optional[torch.Tensor] = None       # characters written
    pout: Optional[torch.Tensor] = None
    pvalid: Optional[torch.Tensor] = None
    pchars: Optional[torch.Tensor] = None
    poff: Optional[torch.Tensor] = None
    owidth: int = 4                              # offset bytes of a projected utf8/binary column
    pattr: bool = False                          # project the joined attribute's codes
    pcol: Optional[int] = None                   # plan column of the projection
    sel: Optional[_SelRun] = None                # project=[...]: the select list instead
    # aggregate
    agg: Optional[_AggSpec] = None
    block: Optional[torch.Tensor] = None         # the scan's accumulator block
    block_ready: Optional[torch.cuda.Event] = None   # ... initialised (emit stream)


@dataclass
class _Buf:
    off: int          # file offset of the stored buffer
    length: int       # stored bytes (prefix + frame when compressed)
    need: int         # bytes the scan reads from the decoded buffer
    cap: int          # decode capacity (need rounded up to 64)
    compressed: bool


@dataclass
class _Batch:
    rows: int
    row_base: int
    # per scanned column: (data, validity, extra) — data: values / bool bits /
    # dictionary indices / utf8-binary offsets; extra: the characters
    cols: List[Tuple[_Buf, Optional[_Buf], Optional[_Buf]]]


class _PlanArr:
    """The plan as arrays (no per-batch Python objects: a cold qualifier-list
    plan over thousands of record batches was ~0.1 s of Python): per batch
    ``rows`` / ``row_base``, per (batch, column, buffer) with buffer 0 data,
    1 validity, 2 characters: file ``off``, stored ``length``, decoded
    ``need``, decode ``cap`` and ``present``; ``comp`` per batch.  Indexing
    gives the _Batch view of one batch; slicing a range of batches."""

    def __init__(self, rows, row_base, off, length, need, cap, present, comp):
        self.rows, self.row_base = rows, row_base
        self.off, self.length, self.need, self.cap = off, length, need, cap
        self.present, self.comp = present, comp

    def __len__(self) -> int:
        return len(self.rows)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return _PlanArr(*(a[i] for a in (self.rows, self.row_base, self.off, self.length,
                                             self.need, self.cap, self.present, self.comp)))
        cols = []
        for k in range(self.off.shape[1]):
            cols.append(tuple(_Buf(int(self.off[i, k, j]), int(self.length[i, k, j]),
                                   int(self.need[i, k, j]), int(self.cap[i, k, j]),
                                   bool(self.comp[i])) if self.present[i, k, j] else None
                              for j in range(3)))
        return _Batch(int(self.rows[i]), int(self.row_base[i]), cols)

    def __iter__(self):
        return (self[i] for i in range(len(self)))


@dataclass
class _Group:
    b0: int                               # batches [b0, b1) of the scanned range
    b1: int
    ids: np.ndarray                       # sorted file chunk ids
    dec_bytes: int = 0
    words: int = 0
    # slot-relative launch tables, built once per plan (_prepare): decoder
    # descriptors, and per batch and column the data/validity pointers as
    # (kind, offset) with kind 0 none, 1 slot region, 2 decode buffer
    descs: Optional[np.ndarray] = None
    need: Optional[np.ndarray] = None
    descs_lanes: Optional[np.ndarray] = None   # literal-heavy LZ4 buffers (lane decoder)
    need_lanes: Optional[np.ndarray] = None
    ptr_kind: Optional[np.ndarray] = None   # (n, ncols, 3)
    ptr_rel: Optional[np.ndarray] = None    # (n, ncols, 3)
    aux_len: Optional[np.ndarray] = None    # (n, ncols) decoded character bytes
    table: Optional[np.ndarray] = None      # (n, QUAL_BATCH_FIELDS), pointer columns 0
    column_bytes: int = 0
    has_valid: Optional[np.ndarray] = None  # (ncols,) some batch has a validity buffer
    # extent reads (ArrowScan.EXTENTS): the group's buffers as strom_file_extent
    # records in file order with their slot offsets, the slot span they take
    # and the bytes the reads cover (buffers + holes read through + padding)
    ext: Optional[np.ndarray] = None
    ones: Optional[np.ndarray] = None       # every row selected (aggregate without qualifiers)
    span: int = 0
    read_bytes: int = 0
    gap_bytes: int = 0


@dataclass
class _Slot:
    off: int                               # byte offset of the slot in the ring buffer
    cap: int                               # slot bytes
    dec: torch.Tensor
    bitmap: torch.Tensor
    bm2: Optional[torch.Tensor] = None     # OR-clause scratch bitmap
    event: Optional[torch.cuda.Event] = None
    stream: Optional[torch.cuda.Stream] = None
    count: Optional[torch.Tensor] = None   # selected rows of the slot's group
    junk: Optional[torch.Tensor] = None    # counts of non-final qualifiers
    err: Optional[torch.Tensor] = None     # failed decodes of the slot's group
    scratch: Optional[torch.Tensor] = None # chunk-order restore (page-cache hits)
    pending: object = None                # (CopyResult, landed ids, group)
    keep: List[torch.Tensor] = field(default_factory=list)
    pin: Optional[torch.Tensor] = None     # pinned arena for the group's tables
    keybuf: Optional[torch.Tensor] = None  # int32 per row: the joined attribute's code
    # a StarJoin's attribute legs: one more such buffer each, reused like keybuf
    legbuf: List[torch.Tensor] = field(default_factory=list)
    # computed columns: per expression 8 bytes per row of the bitmap and its
    # validity words, allocated on first use and kept for the slot's later groups
    exprbuf: List[torch.Tensor] = field(default_factory=list)
    exprvalid: List[torch.Tensor] = field(default_factory=list)
    pin_off: int = 0


class _Tables:
    """One batch table per referenced column of a group in its slot: resolved
    on the host when first asked for, uploaded once per group."""

    def __init__(self, upload, s: _Slot, g: _Group, base: int, dec_base: int):
        self.upload, self.s, self.g, self.base, self.dec_base = upload, s, g, base, dec_base
        self.tabs: Dict[int, torch.Tensor] = {}
        self.tabs_np: Dict[int, np.ndarray] = {}
        self.xtabs: Optional[torch.Tensor] = None    # the expression stage's tables

    def _host(self, col: int) -> np.ndarray:
        """The group's strom_qual_batch table for one column: values,
        validity and character pointers resolved against this slot.  A
        column number past the plan's is a computed column: batch b's results
        at row word_base * 64 of the slot's buffer for it, their validity
        words at word word_base."""
        if col not in self.tabs_np and col >= self.g.ptr_kind.shape[1]:
            g, j = self.g, col - self.g.ptr_kind.shape[1]
            t = self.tabs_np[col] = g.table.copy()
            t[:, 0] = self.s.exprbuf[j].data_ptr() + g.table[:, 3] * 512
            t[:, 1] = self.s.exprvalid[j].data_ptr() + g.table[:, 3] * 8
        if col not in self.tabs_np:
            g = self.g
            t = self.tabs_np[col] = g.table.copy()
            kind, rel = g.ptr_kind[:, col, :], g.ptr_rel[:, col, :]
            ptrs = np.where(kind == 1, self.base + rel,
                            np.where(kind == 2, self.dec_base + rel, 0))
            t[:, 0], t[:, 1], t[:, 5] = ptrs[:, 0], ptrs[:, 1], ptrs[:, 2]
            t[:, 6] = g.aux_len[:, col]
        return self.tabs_np[col]

    def host5(self, col: int) -> np.ndarray:
        """The strom_filter_batch prefix of the column's table, on the host."""
        return self._host(col)[:, :BATCH_FIELDS]

    def qual(self, col: int) -> torch.Tensor:
        """The column's full table on the device."""
        if col not in self.tabs:
            self.tabs[col] = self.upload(self.s, self._host(col))
            self.s.keep.append(self.tabs[col])
        return self.tabs[col]

    def dev5(self, col: int) -> torch.Tensor:
        """The strom_filter_batch prefix of ``qual(col)``, on the device."""
        return self.qual(col)[:, :BATCH_FIELDS].contiguous()


def _up64(n: int) -> int:
    return (n + 63) // 64 * 64


def _up64_np(n: np.ndarray) -> np.ndarray:
    return (n + 63) // 64 * 64


def _stored_sizes(path: str, off: np.ndarray, ln: np.ndarray, comp: np.ndarray) -> np.ndarray:
    """Decoded bytes of variable-size buffers (utf8/binary characters):
    the stored length when raw, else the Arrow BodyCompression prefix
    (i64 uncompressed length, -1 = stored raw after it), read with a few
    preads in flight — the plan needs the decode capacity before any data
    is read into HBM."""
    out = np.asarray(ln, np.int64).copy()
    comp = np.asarray(comp, bool)
    out[comp & (out < 8)] = 0
    idx = np.flatnonzero(comp & (np.asarray(ln) >= 8))
    if len(idx):
        from concurrent.futures import ThreadPoolExecutor
        fd = os.open(path, os.O_RDONLY)
        try:
            with ThreadPoolExecutor(16) as ex:
                vals = np.array(list(ex.map(
                    lambda o: struct.unpack("<q", os.pread(fd, 8, o))[0],
                    np.asarray(off)[idx].tolist())), dtype=np.int64)
        finally:
            os.close(fd)
        raw = vals == -1
        bad = ~raw & ((vals < 0) | (vals >= (1 << 31)))
        if bad.any():
            k = int(idx[np.flatnonzero(bad)[0]])
            raise ValueError(f"record batch {k}: buffer length prefix {int(vals[bad][0])}")
        out[idx] = np.where(raw, out[idx] - 8, vals)
    return out


class ArrowScan:
    # the decoder runs one stream per compressed buffer at a roughly fixed
    # per-stream rate (profiles/r2/dec): a launch needs thousands of streams
    # to fill the GPU, so compressed groups grow to hold that many buffers
    TARGET_STREAMS = 8192
    # streams per group: one round of the block-parallel decoder's resident
    # workgroups (its 512-thread build: 3 per CU, 768 config-5 frames at
    # 115 GB/s), so a group's decode takes one stream's latency and the last
    # group's decode — the part no read overlaps — stays short.  0: cut a
    # compressed column into nslots groups instead.  (Same-box A/B of 2 / 4
    # per CU and 0 on config 5 was inside the storage noise:
    # profiles/r3/arrow_group_policy_ab/.)
    ROUND_STREAMS_PER_CU = int(os.environ.get("STROM_ARROW_ROUND_PER_CU", "3"))
    # ZSTD groups: 1 / ZSTD_ROUND_DIV of the zstd decoder's resident round
    # (lane-parallel decoder: 2, four groups for config 5's val — its
    # decode latency is per block, so a group's decode overlaps the next
    # groups' reads; 4+ groups lose to the reads' interleaving)
    ZSTD_ROUND_DIV = int(os.environ.get("STROM_ARROW_ZSTD_DIV", "2"))
    # the zstd decoder per group launch: 2 lane-parallel (default: the
    # blocks' entropy stages on the lanes of a wave, so a group's decode
    # takes about one block's latency, not one stream's), None the wave /
    # frame-parallel choice by stream count, 0 one wave per stream, 1
    # frame-parallel
    ZSTD_MODE = (int(os.environ["STROM_ARROW_ZSTD_MODE"])
                 if os.environ.get("STROM_ARROW_ZSTD_MODE") else 2)
    # reads: the group's buffers as exact extents (MEMCPY_SSD2GPU_EXTENTS,
    # VERDICT r5 #4) — a column's buffers in large requests, holes up to
    # EXTENT_GAP read through — instead of the fixed-size chunk ids covering
    # them (whole chunks: read amplification, small scattered requests).
    # STROM_ARROW_EXTENTS=0: chunk ids (A/B)
    EXTENTS = os.environ.get("STROM_ARROW_EXTENTS", "1") != "0"
    EXTENT_GAP = int(os.environ.get("STROM_ARROW_EXTENT_GAP", str(64 << 10)))

    def __init__(self, path: str, device=None, chunk_sz: Optional[int] = None,
                 slot_bytes: int = 256 << 20, nslots: Optional[int] = None,
                 max_slot_bytes: int = 4 << 30):
        """``chunk_sz`` / ``nslots`` default by the file's codec: LZ4 64 KiB
        chunks, 3 slots; ZSTD 16 KiB chunks (a buffer is read as whole
        chunks: 600 -> 500 MB read for config 5's ``val``) and 4 slots, so
        the reads of every one of its groups are in flight behind the first
        (profiles/r5/zstd_arrow/group_ab/)."""
        self.path = path
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        self.meta: ArrowFile = read_metadata(path)
        zstd = set(self.meta.codecs) - {None} == {"zstd"}
        self.chunk_sz = chunk_sz if chunk_sz else ((16 << 10) if zstd else (64 << 10))
        self.slot_bytes = slot_bytes
        self.max_slot_bytes = max(slot_bytes, max_slot_bytes)
        self.nslots = max(2, nslots if nslots else (4 if zstd else 3))
        self.reader: Optional[FileReader] = None
        self._slots: List[_Slot] = []
        self._wbs: List[Optional[torch.Tensor]] = []
        # (column tuple, batch range) -> (dtypes, rows, groups)
        self._plans: Dict[tuple, tuple] = {}
        self._bplans: Dict[tuple, tuple] = {}   # column tuple -> _plan()
        self._dicts: Dict[str, tuple] = {}      # decoded dictionaries
        self._compiled: Dict[tuple, Compiled] = {}

    # ------------------------------------------------------------- plan
    def _plan(self, names: Sequence[str]) -> tuple:
        """(per batch _Batch with each column's (data, validity, extra)
        buffers, the Column metas, total rows).  data: the values / bool
        bits / dictionary indices / utf8-binary offsets; extra: the
        characters of a utf8/binary column."""
        cis, cols = [], []
        for name in names:
            ci = self.meta.column_index(name)
            col = self.meta.schema[ci]
            if not col.supported:
                raise NotImplementedError(f"column {name}: {col.kind} columns are not scanned "
                                          "on the GPU")
            cis.append(ci)
            cols.append(col)
        m = self.meta
        used = set(m.codecs) - {None}
        if not used <= {"lz4_frame", "zstd"} or len(used) > 1:
            raise NotImplementedError(f"body compression {sorted(used)} (GPU decoders: one of "
                                      "LZ4 frame, ZSTD per file)")
        # lz4par.hip / zstd.hip (Arrow IPC buffer codecs: length prefix + frame)
        self._codec = D.ARROW_ZSTD if used == {"zstd"} else D.ARROW_LZ4
        comp = np.array([c is not None for c in m.codecs], dtype=bool)
        rows = m.columns[cis[0]].length if m.nbatches else np.zeros(0, np.int64)
        base = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
        nb, nc = len(rows), len(cols)
        off = np.zeros((nb, nc, 3), np.int64)
        length = np.zeros((nb, nc, 3), np.int64)
        need = np.zeros((nb, nc, 3), np.int64)
        present = np.zeros((nb, nc, 3), bool)
        for k, (ci, col) in enumerate(zip(cis, cols)):
            a = m.columns[ci]
            n = a.length
            st = col.storage
            if st == "b1":
                dneed = (n + 7) // 8
            elif st == "d16":
                dneed = n * 16
            elif col.kind in ("utf8", "binary") and col.dictionary is None:
                dneed = np.where(n > 0, (n + 1) * (8 if col.large else 4), 0)
            else:
                dneed = n * np.dtype(st).itemsize
            strings = a.x_off is not None and col.dictionary is None
            xneed = _stored_sizes(self.path, a.x_off, a.x_len, comp) if strings else None
            for what, o, ln, nd in (("data", a.d_off, a.d_len, dneed),
                                    ("characters", a.x_off, a.x_len, xneed)):
                if nd is None:
                    continue
                # a raw buffer shorter than its rows, or an empty one (compressed
                # or not) for a non-empty batch, would send the kernels past
                # the bytes the plan reserves for it
                short = (~comp & (ln < nd)) | ((ln == 0) & (nd > 0))
                if short.any():
                    b = int(np.flatnonzero(short)[0])
                    raise ValueError(f"column {col.name}, record batch {b}: {what} buffer of "
                                     f"{int(ln[b])} bytes for {int(nd[b])}")
            off[:, k, 0], length[:, k, 0], need[:, k, 0] = a.d_off, a.d_len, dneed
            present[:, k, 0] = True
            off[:, k, 1], length[:, k, 1], need[:, k, 1] = a.v_off, a.v_len, (n + 7) // 8
            present[:, k, 1] = (a.null_count != 0) & (a.v_len != 0)
            if strings:
                off[:, k, 2], length[:, k, 2], need[:, k, 2] = a.x_off, a.x_len, xneed
                present[:, k, 2] = True
        # decode capacities: data / characters rounded up to 64, validity
        # + 64 (the filters read it as whole 64-bit words)
        cap = _up64_np(need)
        cap[:, :, 1] += 64
        cap[:, :, 2] += 64
        plan = _PlanArr(rows.astype(np.int64), base[:-1], off, length, need, cap, present, comp)
        return plan, cols, int(base[-1])

    def _round_streams(self) -> int:
        cus = 256
        if self.device.type == "cuda":
            cus = torch.cuda.get_device_properties(self.device).multi_processor_count
        if getattr(self, "_codec", None) == D.ARROW_ZSTD:
            # zstd.hip: one wavefront per stream, residency bound by its LDS.
            # A group's decode takes about one stream's latency whatever its
            # size (the entropy stage is serial per stream), so groups stay a
            # whole round: smaller ones queue on the HBM slot ring one
            # latency each (A/B, profiles/r3/zstd/arrow_group_div_ab.json:
            # val 11.0-12.8 GB/s at a round, 5.8 at a quarter, 4.2 at an eighth)
            from .. import _native as N
            if self.ZSTD_MODE == 2:
                # lane-parallel: a group of about one resident round of its
                # entropy waves' blocks (config-5 buffers: 4 blocks each)
                info = np.zeros(8, np.uint32)
                N.lib().strom_zstd_lp_info(info.ctypes.data)
                rnd = cus * int(info[2]) * int(info[1]) // 4
            elif self.ZSTD_MODE == 1:             # frame-parallel: its own round
                rnd = cus * max(1, int(N.lib().strom_zstd_fp_per_cu()))
            else:
                rnd = cus * max(1, (160 << 10) // int(N.lib().strom_zstd_lds_bytes()))
            return max(1, rnd // self.ZSTD_ROUND_DIV)
        return self.ROUND_STREAMS_PER_CU * cus

    def _groups(self, pl: _PlanArr) -> List[_Group]:
        slot = self.slot_bytes
        nb = len(pl)
        # really compressed buffers (a stored-raw one is as long as its data)
        # (zstd: every compressed buffer takes the entropy stage's latency,
        # however little it compressed — only stored ones are skipped)
        lim = 1.0 if getattr(self, "_codec", None) == D.ARROW_ZSTD else 0.9
        d_len, d_need = pl.length[:, :, 0], pl.need[:, :, 0]
        real = pl.comp[:, None] & (d_len > 0) & (d_len < lim * d_need)     # (nb, ncols)
        ncomp = int(real.sum())
        if ncomp:
            # few streams per launch are fine for the block-parallel decoder
            # (lz4par.hip: a workgroup per stream), so a column of many
            # buffers is cut into nslots groups: the decode of group g then
            # overlaps the reads of groups g+1.. (with the round-2 lane
            # decoder every launch took one serial stream's time and the
            # split measured slower, profiles/r3/arrow_split3.json)
            stored = pl.present & (pl.length > 0)
            total = float((pl.length * stored * real[:, :, None]).sum())
            avg = total / ncomp
            want = avg * self.TARGET_STREAMS
            # groups of at most one resident round of streams: the decode of
            # a group takes one stream's latency, and the last group's
            # decode (the part no read overlaps) is as short as it gets
            rnd = self._round_streams()
            if rnd and ncomp > rnd:
                slot = int(min(self.max_slot_bytes, want, total / -(-ncomp // rnd) * 1.02))
            else:
                if not rnd and ncomp >= self.nslots * 256:
                    want = min(want, total / self.nslots)     # one group per slot
                slot = int(min(self.max_slot_bytes, max(slot, want)))
        limit = max(1, slot // self.chunk_sz)
        # (batch, chunk) pairs of every stored buffer, in file order: record
        # batch bodies follow each other, so chunk ids never decrease from one
        # batch to the next, and the distinct chunks of batches [a, b] are
        # the "new" pairs among theirs (prefix sums: no per-batch sets)
        c = self.chunk_sz
        st = pl.present & (pl.length > 0)
        bi, ki, ji = np.nonzero(st)
        lo = pl.off[bi, ki, ji] // c
        hi = (pl.off[bi, ki, ji] + pl.length[bi, ki, ji] + c - 1) // c
        cnt = hi - lo
        tot = int(cnt.sum())
        pb = np.repeat(bi, cnt)
        start = np.repeat(np.cumsum(cnt) - cnt, cnt)
        ch = np.repeat(lo, cnt) + (np.arange(tot) - start)
        order = np.lexsort((ch, pb))
        pb, ch = pb[order], ch[order]
        if tot:
            keep = np.ones(tot, bool)
            keep[1:] = (pb[1:] != pb[:-1]) | (ch[1:] != ch[:-1])
            pb, ch = pb[keep], ch[keep]
        new = np.ones(len(ch), bool)
        if len(ch):
            new[1:] = ch[1:] != ch[:-1]
        cum = np.concatenate([[0], np.cumsum(new)])
        first = np.searchsorted(pb, np.arange(nb), "left")
        last = np.searchsorted(pb, np.arange(nb), "right")
        bounds = []
        a = 0
        firstl, lastl, cuml = first.tolist(), last.tolist(), cum.tolist()
        for b in range(nb):
            s0, e1 = firstl[a], lastl[b]
            # distinct chunks of batches [a, b]: the first pair counts too
            d = (cuml[e1] - cuml[s0 + 1] + 1) if e1 > s0 else 0
            if b > a and d > limit:
                bounds.append((a, b))
                a = b
        if nb:
            bounds.append((a, nb))
        groups = []
        for a, b in bounds:
            ids = np.unique(ch[first[a]:last[b - 1]]).astype(np.int64)
            g = _Group(a, b, ids)
            sub = pl[a:b]
            g.dec_bytes = int((sub.cap * (sub.present & sub.comp[:, None, None])).sum())
            g.words = int(((sub.rows + 63) // 64).sum())
            self._prepare(g, sub)
            groups.append(g)
        return groups

    def _prepare(self, g: _Group, pl: _PlanArr) -> None:
        c = self.chunk_sz
        n, ncols = pl.off.shape[0], pl.off.shape[1]
        pres = pl.present
        comp3 = np.broadcast_to(pl.comp[:, None, None], pres.shape)
        empty = pres & (pl.length == 0)               # empty batch: nothing is read
        dec = pres & ~empty & comp3
        raw = pres & ~empty & ~comp3
        kind = np.zeros((n, ncols, 3), np.int8)
        kind[empty | dec] = 2
        kind[raw] = 1
        rel = np.zeros((n, ncols, 3), np.int64)
        # decode buffer offsets in (batch, column, buffer) order
        capd = np.where(dec, pl.cap, 0).reshape(-1)
        dstart = (np.cumsum(capd) - capd).reshape(n, ncols, 3)
        rel[dec] = dstart[dec]

        if self.EXTENTS:
            # the group's buffers as extents in file order, laid out by the
            # engine's planner (plan only: the slot offsets and span)
            stm = pres & (pl.length > 0)
            eo, el = pl.off[stm].astype(np.int64), pl.length[stm].astype(np.int64)
            order = np.argsort(eo, kind="stable")
            eo, el = eo[order], el[order]
            uo, first = np.unique(eo, return_index=True)
            ul = np.maximum.reduceat(el, first) if len(uo) else el[:0]
            g.ext = api.extents_array(uo, ul)
            r = api.memcpy_ssd2gpu_extents(0, 0, self._plan_fd(), g.ext, gap_max=self.EXTENT_GAP,
                                           plan_only=True)
            g.span = int(-(-r.dst_bytes // 4096) * 4096)
            g.read_bytes, g.gap_bytes = int(r.bytes_read), int(r.gap_bytes)

            def slot_off(off):
                off = np.asarray(off, dtype=np.int64)
                return g.ext["dst_off"][np.searchsorted(uo, off)].astype(np.int64)
        else:
            # file offsets -> offsets in the slot (chunks land in id order)
            def slot_off(off):
                off = np.asarray(off, dtype=np.int64)
                return np.searchsorted(g.ids, off // c) * c + off % c
            g.span = len(g.ids) * c
            g.read_bytes = g.span
        rel[raw] = slot_off(pl.off[raw])
        g.descs = g.descs_lanes = None
        # LZ4 buffers that barely compressed (>= 0.9 of their data: long
        # literal runs, e.g. a utf8 column's characters) go to the
        # lane-group decoder, which copies literals wide and parses their
        # few tokens serially; the block-parallel one is for the rest
        # (lz4par_bench chars: lanes 174 / par 109 GB/s at 2,048 streams;
        # val: lanes 28 / par 109)
        lit = dec & (pl.length >= 0.9 * pl.need) if self._codec == D.ARROW_LZ4 else \
            np.zeros_like(dec)
        for m, attr in ((dec & ~lit, "descs"), (lit, "descs_lanes")):
            if not m.any():
                continue
            # largest decodes first: a stream's decode time grows with its
            # size, and the decoders hand streams to workgroups in descriptor
            # order (zstd.hip's persistent grid takes stream w, w + grid, ...),
            # so the small validity buffers fill in behind the data buffers
            # instead of taking a resident round of their own
            dl = pl.cap[m]
            order = np.argsort(-dl, kind="stable")
            setattr(g, attr, D.make_descs_arrays(slot_off(pl.off[m])[order], pl.length[m][order],
                                                 dstart[m][order], dl[order]))
            setattr(g, "need" if attr == "descs" else "need_lanes",
                    pl.need[m].astype(np.int32)[order])
        g.ptr_kind, g.ptr_rel = kind, rel
        g.aux_len = np.where(pres[:, :, 2], pl.need[:, :, 2], 0)
        words = (pl.rows + 63) // 64
        table = np.zeros((n, QUAL_BATCH_FIELDS), dtype=np.int64)
        table[:, 2] = pl.rows
        table[:, 3] = np.concatenate([[0], np.cumsum(words)[:-1]]) if n else 0
        table[:, 4] = pl.row_base
        g.table = table
        # decoded bytes the scan reads: values / indices / offsets + characters
        g.column_bytes = int(pl.need[:, :, 0].sum() + (pl.need[:, :, 2] * pres[:, :, 2]).sum())
        g.has_valid = pres[:, :, 1].any(axis=0)

    # --------------------------------------------------------- pipeline
    # HBM for the slot ring beyond nslots (a slot per group up to this):
    # with a slot of its own a group's read never waits for an earlier
    # group's decode to free one (r5 timeline: date_ts group 4 was submitted
    # 12 ms late, behind group 0's decode, and held groups 2-3's launches)
    MAX_RING_BYTES = 8 << 30
    MAX_SLOTS = 16
    # HBM for everything a slot holds: its compressed ring share, its decode
    # buffer and (ZSTD lane-parallel) the entry pool the library keeps for
    # its stream (only the ring was counted)
    MAX_SLOT_HBM = 48 << 30

    def _lp_pool_bytes(self, dec: int) -> int:
        """The LP decoder's entry pool for a decode of ``dec`` bytes
        (zstd.hip strom_decompress_zstd_lp: STROM_ZSTD_LP_ENT x dst + block
        and stream tables), 0 for other decoders."""
        if getattr(self, "_codec", None) != D.ARROW_ZSTD or self.ZSTD_MODE != 2:
            return 0
        f = float(os.environ.get("STROM_ZSTD_LP_ENT") or 0) or 3.0
        return int(f * dec) + (1 << 20) + dec // 32768 * 64

    def _slot_count(self, groups: List[_Group], nbytes: int, dec: int = 0) -> int:
        """Slots of the HBM ring: one per group while they fit MAX_RING_BYTES
        / MAX_SLOTS and, with their decode buffers and LP pools, MAX_SLOT_HBM;
        never fewer than nslots (or than the groups).  ZSTD lane-parallel
        slots are also capped by the pools the library keeps per stream
        (strom_zstd_scratch_keep): one more slot would evict another slot's
        pool every decode — a hipFree that waits for the device, and a
        multi-GB hipMalloc.  The read-ahead stays nslots - 1 groups."""
        n = len(groups)
        per_slot = nbytes + dec + self._lp_pool_bytes(dec)
        fit = max(1, min(self.MAX_SLOTS, self.MAX_RING_BYTES // max(nbytes, 1),
                         self.MAX_SLOT_HBM // max(per_slot, 1)))
        want = max(1, min(n, max(self.nslots, fit)))
        if self._lp_pool_bytes(dec):
            from .. import _native as N
            want = min(want, max(1, int(N.lib().strom_zstd_scratch_keep())))
        return want

    def _plan_fd(self) -> int:
        """A descriptor of the file for the extent planner (file size)."""
        if getattr(self, "_pfd", None) is None:
            self._pfd = os.open(self.path, os.O_RDONLY)
        return self._pfd

    def _ensure_slots(self, groups: List[_Group]) -> None:
        nbytes = max(max(g.span for g in groups), self.chunk_sz)
        nbytes = -(-nbytes // self.chunk_sz) * self.chunk_sz
        dec = max(max(g.dec_bytes for g in groups), 64)
        words = max(max(g.words for g in groups), 1)
        want_slots = self._slot_count(groups, nbytes, dec)
        if self._slots and len(self._slots) >= want_slots and (
                self._slots[0].cap >= nbytes and
                            self._slots[0].dec.numel() >= dec and
                            self._slots[0].bitmap.numel() >= words):
            return
        self._free_slots()
        # one registered HBM ring for every slot: one MAP (dma-buf export +
        # BAR mapping) per scan object instead of one per slot (cold cost);
        # no more slots than groups
        nsl = want_slots
        self._hbm = HbmBuffer(nbytes * nsl, self.device)
        for k in range(nsl):
            sl = _Slot(k * nbytes, nbytes,
                       torch.empty(dec, dtype=torch.uint8, device=self.device),
                       torch.empty(words, dtype=torch.int64, device=self.device),
                       torch.empty(words, dtype=torch.int64, device=self.device))
            sl.stream = torch.cuda.Stream(device=self.device)
            sl.count = torch.zeros(1, dtype=torch.int64, device=self.device)
            sl.junk = torch.zeros(1, dtype=torch.int64, device=self.device)
            sl.err = torch.zeros(1, dtype=torch.int64, device=self.device)
            self._slots.append(sl)
        if self.reader is None:
            self.reader = FileReader(self.path, chunk_sz=self.chunk_sz,
                                     max_chunks=nbytes // self.chunk_sz)
        # pinned write-back buffers only once the BAR path is refused (a
        # cold-scan cost otherwise: GiBs of pinned host memory per scan)
        self._wbs = [None] * len(self._slots)
        self._wb_bytes = nbytes

    def _submit(self, k: int, g: _Group) -> None:
        s = self._slots[k % len(self._slots)]
        if s.event is not None:
            s.event.synchronize()            # the slot's previous group is consumed
            s.event = None
        s.keep = []
        # the slot's own write-back buffer, sized for this scan's groups and
        # pinned only if page-cache chunks have to go through host memory
        # (a group may outgrow the reader's own buffer, and slots in flight
        # must not share one)
        i = k % len(self._wbs)

        def wb():
            if self._wbs[i] is None:
                self._wbs[i] = host_buffer(self._wb_bytes)
            return self._wbs[i]
        if self.EXTENTS:
            res = api.memcpy_ssd2gpu_extents(self._hbm.handle, s.off, self.reader.fd, g.ext,
                                             gap_max=self.EXTENT_GAP, sess=self.reader.sess)
            s.pending = (res, None, g)
            return
        res, landed = self.reader.submit(self._hbm, s.off, g.ids.astype(np.uint32), wb=wb)
        s.pending = (res, landed, g)

    def _upload(self, s: "_Slot", arr: np.ndarray) -> torch.Tensor:
        """``arr`` as a device tensor, copied on the current stream through
        the slot's pinned arena.  A pinned allocation per group (pin_memory())
        could synchronize the device: the host then waited for group k's
        decode before launching group k+1's (r5 Arrow ZSTD timeline: 12.7 ms
        between group 1 landing and its launch).  The arena is reused once
        the slot's previous group is consumed (_submit waits for it)."""
        a = np.ascontiguousarray(arr)
        raw = a.reshape(-1).view(np.uint8)
        n = raw.nbytes
        o = (s.pin_off + 255) & ~255
        if s.pin is None or o + n > s.pin.numel():
            if s.pin is not None:
                s.keep.append(s.pin)          # earlier copies of this group read it
            s.pin = torch.empty(max(4 << 20, 2 * (n + 256)), dtype=torch.uint8,
                                pin_memory=self.device.type == "cuda")
            o = 0
        s.pin_off = o + n
        host = s.pin[o:o + n]
        host.numpy()[:] = raw
        d = torch.empty(n, dtype=torch.uint8, device=self.device)
        d.copy_(host, non_blocking=True)
        return d.view(torch.from_numpy(a[:0].reshape(-1)).dtype).reshape(a.shape)

    def _compute(self, k: int, spec, run: _Run) -> None:
        """Group k in its slot: every stage but the emit on the slot's stream."""
        s = self._slots[k % len(self._slots)]
        g, region = self._land(k, s, run)
        with torch.cuda.stream(s.stream):
            self._decode(k, s, g, region, run)
            t = _Tables(self._upload, s, g, region.data_ptr(), s.dec.data_ptr())
            if run.exprs:
                # the computed columns a qualifier reads, over every row
                self._evaluate(s, g, t, run, True, None)
            bitmap = self._filter(s, g, t, spec, counts=run.join is None)
            # the table of the slot's key buffer once a stage writes codes there
            d_codes = None
            if run.join is not None:
                bitmap, d_codes = self._probe(s, g, t, run.join, bitmap)
                if run.join.star and d_codes is not None:
                    # project= / by=dim[attr] / top carry one attribute: leg
                    # buffer 0 (a HashBy of several reads them by its own tables)
                    d_codes = d_codes[0]
            if run.exprs:
                # the others, over the words that still select something
                self._evaluate(s, g, t, run, False, bitmap)
            if run.hash is not None:
                bitmap, d_codes = self._group_codes(s, g, t, run.hash, bitmap)
            run.marks.append((k, "quals_queued", time.perf_counter()))
            # emit tables: the strom_filter_batch prefix of the qual tables
            any_col = spec[0][0][0] if spec else (run.join.legs[0].col if run.join is not None
                                                  else 0)
            d_rows = t.dev5(any_col)
            args = d_proj = slabs = None
            if run.top is not None:
                slabs = self._select(s, g, t, run.top, bitmap, d_codes)
            if run.agg is not None:
                args = self._accumulate(s, g, t, run, any_col, bitmap,
                                        d_codes.data_ptr() if d_codes is not None else 0)
            if run.pattr:
                d_proj = d_codes                 # the joined attribute's codes
            elif run.pcol is not None:
                d_proj = t.qual(run.pcol) if run.pchars is not None else t.dev5(run.pcol)
            elif run.sel is not None:
                d_proj = self._select_tables(s, g, t, run.sel)
            s.keep += [d_rows] + ([d_proj] if d_proj is not None else [])
        self._emit(s, g, run, d_rows, d_proj, args, slabs)
        run.bytes_read += g.read_bytes
        run.column_bytes += g.column_bytes
        run.marks.append((k, "launched", time.perf_counter()))

    def _land(self, k: int, s: _Slot, run: _Run) -> Tuple[_Group, torch.Tensor]:
        """The slot's read finished: (its group, the group's bytes in file order)."""
        res, landed, g = s.pending
        s.pending = None
        s.pin_off = 0
        t0 = time.perf_counter()
        self.reader.finish(res)
        t1 = time.perf_counter()
        run.wait_s += t1 - t0
        run.marks.append((k, "landed", t1))
        region = self._hbm.tensor[s.off:s.off + g.span]
        nr_ram = getattr(res, "nr_ram", 0)            # extent reads: all from storage
        # write-back copies of page-cache chunks (FileReader.submit without a
        # BAR) were queued on the current stream; only then wait for it (a
        # wait on the default stream also waits for whatever blocking
        # streams hold)
        if nr_ram:
            s.stream.wait_stream(torch.cuda.current_stream(self.device))
        if nr_ram and not np.array_equal(landed, g.ids.astype(np.uint32)):
            # page-cache chunks landed at the tail: restore chunk order
            with torch.cuda.stream(s.stream):
                if s.scratch is None:
                    s.scratch = torch.empty(s.cap, dtype=torch.uint8, device=self.device)
                tmp = s.scratch[:region.numel()]
                tmp.copy_(region)
                chunk_scatter(tmp, region, landing_positions(g.ids.astype(np.uint32), landed,
                                                             res.nr_ssd), self.chunk_sz)
        return g, region

    def _decode(self, k: int, s: _Slot, g: _Group, region: torch.Tensor, run: _Run) -> None:
        for dsc, need, lanes in ((g.descs, g.need, False), (g.descs_lanes, g.need_lanes, True)):
            if dsc is None:
                continue
            # every compressed buffer of every scanned column: one launch
            # (two when some are literal-heavy LZ4)
            d_desc = self._upload(s, dsc.view(np.uint8))
            d_need = self._upload(s, need)
            status = torch.empty(len(dsc), dtype=torch.int32, device=self.device)
            D.decompress_async(self._codec, region, s.dec, d_desc, status, stream=s.stream,
                               lanes=lanes, zstd_mode=self.ZSTD_MODE)
            # status = decoded bytes; short or failed -> error count
            s.err += ((status < d_need) | (status < 0)).sum()
            s.keep += [d_desc, d_need, status]
            run.marks.append((k, "decode_queued", time.perf_counter()))

    def _filter(self, s: _Slot, g: _Group, t: _Tables, spec, counts: bool) -> torch.Tensor:
        """The CNF qualifier list: clause 0 writes the bitmap (its predicates
        ORed in place), a later single-predicate clause ANDs into it, a later
        OR-clause collects in the scratch bitmap and its last predicate ORs
        that in and ANDs into the bitmap.  ``counts``: the list's last launch
        counts the selection (no later stage does).  Returns the bitmap of
        the selection."""
        for ci, clause in enumerate(spec):
            for j, (col, cq) in enumerate(clause):
                last = counts and ci == len(spec) - 1 and j == len(clause) - 1
                cnt = s.count if last else s.junk
                if ci == 0:
                    dst, how = s.bitmap, dict(or_src=s.bitmap if j else None)
                elif len(clause) == 1:
                    dst, how = s.bitmap, dict(and_dst=True)
                elif j < len(clause) - 1:
                    dst, how = s.bm2, dict(or_src=s.bm2 if j else None)
                else:
                    dst, how = s.bitmap, dict(or_src=s.bm2, and_dst=True)
                qual_batched(cq, t.qual(col), g.words, dst, cnt, stream=s.stream, **how)
        if spec:
            return s.bitmap
        # no qualifier (aggregate only): every row of every batch,
        # each batch's last word bounded by its rows
        if g.ones is None:
            g.ones = _all_rows_bitmap(g.table[:, 2])
        bitmap = self._upload(s, g.ones)
        s.keep.append(bitmap)
        return bitmap

    def _evaluate(self, s: _Slot, g: _Group, t: _Tables, run: _Run, early: bool,
                  sel: Optional[torch.Tensor]) -> None:
        """The computed columns of one stage (csrc/kernels/colexpr.hip), one
        launch each: ``early`` those a qualifier reads, before the filter and
        over every row; the others after the probe with the selection ``sel``,
        so that a word no row of which is selected costs nothing.  The source
        tables of all of the group's expressions and the tables of their
        buffers go up in one copy, at the first stage that runs."""
        todo = [x for x in run.exprs if x.early == early]
        if not todo:
            return
        nst = g.ptr_kind.shape[1]
        if t.xtabs is None:
            rows = s.bitmap.numel() * 64
            while len(s.exprbuf) < len(run.exprs):
                s.exprbuf.append(torch.empty(rows, dtype=torch.int64, device=self.device))
                s.exprvalid.append(torch.empty(rows // 64, dtype=torch.int64, device=self.device))
            for j in range(len(run.exprs)):
                if s.exprbuf[j].numel() < rows:
                    s.exprbuf[j] = torch.empty(rows, dtype=torch.int64, device=self.device)
                    s.exprvalid[j] = torch.empty(rows // 64, dtype=torch.int64,
                                                 device=self.device)
            t.xtabs = self._upload(s, np.stack(
                [t.host5(c) for x in run.exprs for c in x.cols] +
                [t.host5(nst + j) for j in range(len(run.exprs))]))
            s.keep.append(t.xtabs)
        nsrc = sum(len(x.cols) for x in run.exprs)
        o = 0
        for j, x in enumerate(run.exprs):
            if x.early == early:
                expr_batched(x.prog, t.xtabs[o:o + len(x.cols)], g.words, t.xtabs[nsrc + j], sel,
                             stream=s.stream)
            o += len(x.cols)

    def _expr_runs(self, meta, full: List[str], cl) -> List[_ExprRun]:
        """The scan's computed columns (``meta``: _with_exprs) for _compute."""
        qual = {p.col for c in cl for p in c}
        return [_ExprRun(p, [full.index(c) for c in p.columns], n in qual)
                for n, p in getattr(meta, "progs", {}).items()]

    def _code_table(self, s: _Slot, g: _Group, leg: int = -1) -> np.ndarray:
        """The batch table of the slot's key buffer, or of its buffer for the
        codes of a StarJoin's attribute leg ``leg`` (int32 per row of the
        bitmap, allocated on first use and kept for the slot's later groups):
        batch b's codes at row word_base * 64."""
        rows = s.bitmap.numel() * 64
        new = lambda: torch.empty(rows, dtype=torch.int32, device=self.device)
        if leg < 0:
            if s.keybuf is None or s.keybuf.numel() < rows:
                s.keybuf = new()
            buf = s.keybuf
        else:
            while len(s.legbuf) <= leg:
                s.legbuf.append(new())
            if s.legbuf[leg].numel() < rows:
                s.legbuf[leg] = new()
            buf = s.legbuf[leg]
        c5 = g.table[:, :BATCH_FIELDS].copy()
        c5[:, 0] = buf.data_ptr() + g.table[:, 3] * 256
        c5[:, 1] = 0
        return c5

    def _probe(self, s: _Slot, g: _Group, t: _Tables, jn: _JoinRun,
               bitmap: torch.Tensor) -> tuple:
        """The probe, the list's last launch (and_dst semantics, its count is
        the selection's): the fk's batch table and, when an attribute is
        wanted, the table of the slot's key buffer go up in one copy.  Returns
        (the selection's bitmap, the latter table on the device or None)."""
        if jn.star:
            return self._probe_star(s, g, t, jn, bitmap)
        leg = jn.legs[0]
        both = [t.host5(leg.col)]
        if leg.attr is not None:
            both.append(self._code_table(s, g))
        d_j = self._upload(s, np.stack(both))
        s.keep.append(d_j)
        d_kout = d_j[1] if leg.attr is not None else None
        J.probe(leg.dev, leg.code, d_j[0], g.words, bitmap, s.bitmap, s.count,
                how=J.HOW[leg.how], key_out=d_kout, stream=s.stream)
        return s.bitmap, d_kout

    def _probe_star(self, s: _Slot, g: _Group, t: _Tables, jn: _JoinRun,
                    bitmap: torch.Tensor) -> tuple:
        """join=StarJoin: every leg's fk table and the tables of the attribute
        legs' code buffers in one copy, every leg in one launch.  Returns (the
        selection's bitmap, the code buffers' tables on the device
        (buffers, batches, 5) or None)."""
        nout = sum(leg.buf >= 0 for leg in jn.legs)
        tabs = [t.host5(leg.col) for leg in jn.legs] + \
            [self._code_table(s, g, j) for j in range(nout)]
        d_j = self._upload(s, np.stack(tabs))
        s.keep.append(d_j)
        d_kout = d_j[len(jn.legs):] if nout else None
        J.probe_star([(leg.dev, leg.code, J.HOW[leg.how], leg.buf) for leg in jn.legs],
                     d_j[:len(jn.legs)], g.words, bitmap, s.bitmap, s.count, key_out=d_kout,
                     stream=s.stream)
        return s.bitmap, d_kout

    def _group_codes(self, s: _Slot, g: _Group, t: _Tables, hs: _HashRun,
                     bitmap: torch.Tensor) -> tuple:
        """by=HashBy: find-or-insert of the key column over the bitmap the
        qualifiers and the probe left; each row's code goes into the slot's
        key buffer, the accumulate launches' key column.  Returns (the
        selection's bitmap, the key buffer's table on the device)."""
        c5 = self._code_table(s, g)
        # a composite key: every component's table, the join attribute's
        # being the code buffers' own (the launch runs in place there: a lane
        # reads its row's components before it stores the row's code) or, with
        # join=StarJoin, each attribute leg's buffer; then, in the same copy,
        # the code buffers'
        k5 = [t.host5(hs.col)] if hs.cols is None else \
            [(c5 if b < 0 else self._code_table(s, g, b)) if c is None else t.host5(c)
             for c, b in zip(hs.cols, hs.bufs)]
        d_h = self._upload(s, np.stack(k5 + [c5]))
        s.keep.append(d_h)
        if hs.cols is None:
            G.group_codes(hs.dev, hs.code, d_h[0], g.words, bitmap, s.bitmap, d_h[1],
                          stream=s.stream)
        else:
            G.group_codes_multi(hs.dev, d_h[:-1], g.words, bitmap, s.bitmap, d_h[-1],
                                stream=s.stream)
        return s.bitmap, d_h[-1]

    def _select_tables(self, s: _Slot, g: _Group, t: _Tables, sel: _SelRun) -> torch.Tensor:
        """project=[...]: the strom_qual_batch table of every column of the
        select list — a stored or computed column's own, a join attribute's
        that of the buffer the probe left its codes in — stacked into one
        upload (columns, batches, 7)."""
        tabs = []
        for it in sel.items:
            if it.pcol is None:
                t7 = g.table.copy()
                t7[:, :BATCH_FIELDS] = self._code_table(s, g, it.buf)
                tabs.append(t7)
            else:
                tabs.append(t._host(it.pcol))
        return self._upload(s, PJ.stack_tables(tabs))

    def _select(self, s: _Slot, g: _Group, t: _Tables, tr: _TopRun, bitmap: torch.Tensor,
                d_codes: Optional[torch.Tensor]) -> tuple:
        """ORDER BY ... LIMIT k: the group's candidates over the selection the
        qualifiers and the probe left (csrc/kernels/coltopk.hip), each
        workgroup's k best in a slab.  The launch reads the state's threshold
        as the emit stream's merges have left it so far.  Returns (slabs, how
        many) for the emit stream to merge."""
        both = [t.host5(tr.col)] + ([t.host5(tr.pcol)] if tr.pcol is not None else [])
        d_t = self._upload(s, np.stack(both))
        d_pay = d_codes if tr.pattr else (d_t[1] if tr.pcol is not None else None)
        slabs, n = T.select(tr.state, tr.code, d_t[0], g.words, bitmap, tr.descending,
                            pay=d_pay, pay_width=tr.pwidth, stream=s.stream)
        s.keep += [d_t, slabs]
        return slabs, n

    def _accumulate(self, s: _Slot, g: _Group, t: _Tables, run: _Run, any_col: int,
                    bitmap: torch.Tensor, key_ptr: int):
        """The aggregate launches over the selection.  The host's time here
        delays the next group's read: the columns' batch tables go up in one
        copy and the launches are one native call.  Returns the entries'
        arguments when slabs are left for the emit stream to fold."""
        agg, hs = run.agg, run.hash
        n = len(g.table)
        cols = sorted({any_col if c is None else c for c in agg.entry_cols} |
                      ({agg.key_col} if agg.key_col is not None else set()))
        d_t5 = self._upload(s, np.stack([t.host5(c) for c in cols]))
        s.keep.append(d_t5)
        at = {c: d_t5.data_ptr() + i * n * BATCH_FIELDS * 8 for i, c in enumerate(cols)}
        if hs is not None:
            # the accumulate launches add into the table's arrays in HBM:
            # no slabs, nothing left for the emit stream to fold
            for e, c in enumerate(agg.entry_cols):
                hs.dev.args[e].vals = at[any_col if c is None else c]
            G.group_agg_many(hs.dev, bitmap, g.words, key_ptr, n, stream=s.stream)
            return None
        # one aggregate launch per aggregated column on the slot's stream,
        # each leaving its workgroups' slabs: the slabs are one allocation
        lay = agg.layout
        if g.words not in agg.slab_words:
            agg.slab_words[g.words] = [A.slab_words(lay, e, g.words)
                                       for e in range(len(lay.entries))]
        sw = agg.slab_words[g.words]
        d_slabs = torch.empty(sum(sw), dtype=torch.int64, device=self.device)
        s.keep.append(d_slabs)
        args = A.entry_args(lay, run.block)
        o = d_slabs.data_ptr()
        for e, c in enumerate(agg.entry_cols):
            args[e].vals = at[any_col if c is None else c]
            args[e].slabs = o
            o += 8 * sw[e]
        A.agg_many(lay, args, run.block, bitmap, g.words,
                   at[agg.key_col] if agg.key_col is not None else key_ptr, n, stream=s.stream)
        return args

    def _emit(self, s: _Slot, g: _Group, run: _Run, d_rows: torch.Tensor,
              d_proj: Optional[torch.Tensor], args, slabs=None) -> None:
        """Decode + filter of successive groups overlap on their slots'
        streams; the row-id emit (+ projection gather) and the fold of the
        slabs run in group order on one stream (the output cursor and the
        block are shared), which then frees the slot."""
        ready = torch.cuda.Event()
        ready.record(s.stream)
        es = self.emit_stream
        es.wait_event(ready)
        with torch.cuda.stream(es):
            if args is not None:
                # the slabs into the scan's accumulator block, in group order
                A.agg_reduce_many(run.agg.layout, args, g.words, stream=es)
            if slabs is not None:
                # the group's candidates into the scan's k best, in group order;
                # the new threshold is there for the launches not yet queued
                T.merge(run.top.state, slabs[0], slabs[1], stream=es)
            if run.sel is not None:
                # the select list: ids and every column in one walk
                PJ.bitmap_to_rows_multi(s.bitmap, g.words, d_rows, run.out, run.cursor,
                                        run.sel.cols, d_proj, stream=es)
            elif run.pchars is not None:
                bitmap_to_rows_str(s.bitmap, g.words, d_rows, run.out, run.cursor, d_proj,
                                   run.owidth, run.poff, run.pchars, run.ccursor,
                                   pvalid=run.pvalid, stream=es)
            elif run.out is not None:
                bitmap_to_rows(s.bitmap, g.words, d_rows, run.out, run.cursor, stream=es,
                               proj=d_proj, proj_out=run.pout, proj_valid=run.pvalid)
            run.count += s.count
            s.count.zero_()
            if g.descs is not None or g.descs_lanes is not None:
                run.err += s.err
                s.err.zero_()
            s.event = torch.cuda.Event()
            s.event.record(es)

    # ------------------------------------------------------------- query
    def dictionary(self, name: str):
        """Decoded dictionary of a dictionary-encoded column (host, cached):
        (values, valid) as utils.arrow_ipc.dictionary_values returns them."""
        return _dictionary(self.meta, self.path, self._dicts, name)

    def _compile(self, p: Pred, meta=None) -> Compiled:
        key = (p.col, p.op, repr(p.value))
        if key not in self._compiled:
            meta = meta if meta is not None else self.meta
            col = meta.schema[meta.column_index(p.col)]
            self._compiled[key] = _compile_pred(p, col, self.dictionary)
        return self._compiled[key]

    def _join_run(self, join, names: List[str], attrs) -> _JoinRun:
        """The checked ``join=`` with the attributes the scan wants written
        (one, a list or None; a StarJoin's attribute legs get the slot's leg
        buffers 0, 1, ... in the order of ``attrs``)."""
        attrs = [] if attrs is None else ([attrs] if isinstance(attrs, JoinAttr) else list(attrs))
        # "cuda" and "cuda:<current device>" are the same place
        idx = lambda d: d.index if d.index is not None else torch.cuda.current_device()
        star = isinstance(join, StarJoin)
        legs = []
        for i, leg in enumerate(_legs(join)):
            td = leg.table.device
            if td is None or td.type != self.device.type or (td != self.device and
                                                              idx(td) != idx(self.device)):
                raise ValueError(f"JoinTable on {td}, scan on {self.device}")
            col = self.meta.schema[self.meta.column_index(leg.col)]
            at = [k for k, a in enumerate(attrs) if _leg_of(join, a) == i]
            name = attrs[at[0]].name if at else None
            legs.append(_LegRun(names.index(leg.col), J.FK_CODE[col.storage], leg.how,
                                leg.table._device_table(name), name,
                                at[0] if at and star else -1))
        return _JoinRun(legs, star)

    def _resolve(self, names: List[str], batches: Optional[Tuple[int, int]]) -> tuple:
        """(Column metas, rows, groups) of a scan of ``names`` over ``batches``,
        planned once per object.  No names: the footer's rows, nothing to read."""
        nb = self.meta.nbatches
        rng = (0, nb) if batches is None else (max(0, int(batches[0])), min(nb, int(batches[1])))
        if not names:
            return [], int(np.asarray(self.meta.rows)[rng[0]:max(rng[0], rng[1])].sum()), []
        key = (tuple(names), rng)
        if key not in self._plans:                # the file's layout is fixed once opened
            if tuple(names) not in self._bplans:
                self._bplans[tuple(names)] = self._plan(names)
            allb, cols, _ = self._bplans[tuple(names)]
            sel = allb[rng[0]:max(rng[0], rng[1])]
            self._plans[key] = (cols, int(sel.rows.sum()) if len(sel) else 0, self._groups(sel))
        return self._plans[key]

    def _zero(self) -> torch.Tensor:
        return torch.zeros(1, dtype=torch.int64, device=self.device)

    def _emit_stream(self) -> torch.cuda.Stream:
        # one emit stream per scan object (its library-kept scratch follows it)
        if getattr(self, "emit_stream", None) is None:
            self.emit_stream = torch.cuda.Stream(device=self.device)
        return self.emit_stream

    def _drive(self, groups: List[_Group], spec, run: _Run) -> float:
        """Every group through the slot ring, then the scan's one sync.
        Returns the clock before the first submit."""
        self._ensure_slots(groups)
        self._emit_stream()
        t_start = time.perf_counter()

        def submit(k: int) -> None:
            self._submit(k, groups[k])
            run.marks.append((k, "submitted", time.perf_counter()))
        # depth nslots - 1 of reads ahead of the group being computed
        ahead = max(1, min(self.nslots, len(self._slots)) - 1)
        for k in range(min(ahead, len(groups))):
            submit(k)
        for k in range(len(groups)):
            if run.block_ready is not None:
                # the aggregate launches (slot streams) count malformed keys
                # in the block: they must see it initialised
                self._slots[k % len(self._slots)].stream.wait_event(run.block_ready)
            self._compute(k, spec, run)
            if k + ahead < len(groups):
                submit(k + ahead)
        torch.cuda.synchronize(self.device)
        # whatever the scan's outcome, no slot keeps its tensors and events
        for s in self._slots:
            s.keep, s.event = [], None
        return t_start

    def _check_decoded(self, err: int, names: List[str]) -> None:
        if err:
            raise RuntimeError(f"{'ZSTD' if self._codec == D.ARROW_ZSTD else 'LZ4'} decode "
                               f"failed for {err} buffer(s) of columns {names}")

    @staticmethod
    def _seconds(run: _Run, t0: float, t_plan: float, t_alloc: float) -> dict:
        return {"plan_s": t_plan - t0, "alloc_s": t_alloc - t_plan, "wait_s": run.wait_s,
                "total_s": time.perf_counter() - t0}

    def scan_where(self, quals, project=None, batches: Optional[Tuple[int, int]] = None,
                   join: Union[Join, StarJoin, None] = None, order_by=None,
                   limit: Optional[int] = None, offset: int = 0) -> ScanOut:
        """Row ids (int64, file order) of the rows every qualifier selects —
        a PG-Strom qualifier list.  ``quals`` items: ``(name, lo, hi)``
        ranges, ``(name, op, value)`` / ``P(name) <op> value`` predicates,
        or ``Or(...)`` clauses of them (ops/colpred.py: comparisons, IN,
        OR of ranges, string equality and prefix, null tests, on ints,
        floats, bool, date/time/timestamp/duration, utf8/binary and
        dictionary-encoded columns).  Nulls never satisfy a comparison.
        Each referenced column is read from storage and decoded once per
        group; the predicates' bitmaps are combined on the device.
        ``project`` names a column whose values (indices for a dictionary:
        ``ScanOut.dictionary`` holds the values; for utf8/binary the
        characters, with ``ScanOut.offsets``) and validity, when it has
        nulls, are gathered for the selected rows while their ids are
        written.  ``batches=(b0, b1)``
        scans only record batches [b0, b1) (row ids stay file-global:
        parallel/scan.py splits a file over ranks this way).
        ``join=Join(fk, dim, how)`` keeps the rows whose ``fk`` is (semi) or
        is not (anti) a key of the JoinTable ``dim``: a hash probe
        (csrc/kernels/coljoin.hip) on the slot's stream after the qualifier
        list, which may then be empty.  ``project=dim[attr]`` gathers the
        joined attribute's code per selected row (``ScanOut.dictionary``
        holds the codes' values).  ``join=StarJoin(Join(...), Join(...), ...)``
        applies up to four such legs in that one launch (a row is kept if every
        leg keeps it); ``dim[attr]`` then names the leg whose table is ``dim``.
        A predicate may be on an expression (ops/colexpr.E: ``E("a") + E("b") <
        5``, every numeric operator) and ``project`` may be one (its int64 or
        float64 values): computed on the device per group (colexpr.hip), at
        most four distinct expressions per scan.
        ``project=[...]`` — a list or tuple, also of one — is a select list:
        up to 16 such items, and bool columns (gathered as uint8 0/1), all
        gathered in one emit pass (csrc/kernels/colproject.hip) and returned
        as ``ScanOut.columns``, one ProjOut per item in the order given;
        ``ScanOut.to_arrow()`` assembles them.  No item twice, one attribute
        per JoinTable.
        ``order_by`` (with a select list) returns the rows sorted instead of
        in file order: one item or a list of up to four, an item a column
        name or an expression, alone (ascending) or in a pair with
        "ascending" / "descending" — ``pyarrow.compute.sort_indices``'
        sort keys, and its order with the default null placement: per column
        a value before a NaN before a null in both directions, -0.0 equal to
        +0.0, rows equal in every column in file order.  The kinds ``top``
        orders: non-dictionary int8-64, uint8-64, float32/64, date, time,
        timestamp, duration, and int64 / float64 expressions.  An order
        column outside the select list is gathered too and not returned
        (listed and hidden items together stay within 16).  ``limit`` and
        ``offset`` (non-negative) cut the sorted rows.  After the scan's one
        sync, whose count sizes them, the launches of a stable radix sort
        (csrc/kernels/colsort.hip, ops/colsort.py: one 8-bit pass per byte of
        a column's storage type, one more for its classes) and one gather of
        every column are enqueued on the emit stream, which the caller's
        stream then waits for; nothing is synchronized again.  The sort holds
        24 bytes per selected row on the device while it runs; the outputs
        are sized for every scanned row as before.  A windowed string
        column's ``values`` keep the capacity of all selected rows'
        characters: ``offsets[-1]`` of them are the result's.
        ``ScanOut.order`` is the normalized [(name, descending)]; ``top``
        remains the path for small k, allocating nothing of the table's
        height."""
        _check_order_args(project, order_by, limit, offset)
        if isinstance(project, (list, tuple)):
            return self._scan_select(quals, project, batches, join, order_by, limit, offset)
        pattr = project if isinstance(project, JoinAttr) else None
        join = _check_join(self.meta, join, pattr)
        if pattr is not None:
            project = None
        project = name_of(project)
        cl = _named_clauses(quals) if (quals or join is None) else []
        t0 = time.perf_counter()
        names = _scanned(cl, join, [project] if project else [])
        xm = _with_exprs(self.meta, names)
        names, full = _split_names(xm, names)
        cols, nrows, groups = self._resolve(names, batches)
        spec = [[(full.index(p.col), self._compile(p, xm)) for p in c] for c in cl]
        t_plan = time.perf_counter()
        out = torch.empty(max(nrows, 1), dtype=torch.int64, device=self.device)
        pcol = full.index(project) if project else None
        pout = pvalid = pchars = poff = None
        pmeta = xm.schema[xm.column_index(project)] if project else None
        pstrings = bool(project) and pmeta.kind in ("utf8", "binary") and pmeta.dictionary is None
        if project:
            st = pmeta.storage
            if pstrings:
                # characters: at most the column's, per the plan
                nch = sum(int(g.aux_len[:, pcol].sum()) for g in groups)
                pchars = torch.empty(max(nch, 1), dtype=torch.uint8, device=self.device)
                poff = torch.empty(max(nrows, 1) + 1, dtype=torch.int64, device=self.device)
            elif st == "d16":
                # decimal128: (lo, hi) int64 words per row, value x 10^scale
                pout = torch.empty((max(nrows, 1), 2), dtype=torch.int64, device=self.device)
            elif st not in _TORCH:
                raise NotImplementedError(f"projection of {project} ({pmeta.kind}): fixed-width, "
                                          "utf8/binary or dictionary-encoded columns")
            else:
                pout = torch.empty(max(nrows, 1), dtype=_TORCH[st], device=self.device)
            if pmeta.nullable if pcol >= len(names) else \
                    any(bool(g.has_valid[pcol]) for g in groups):
                pvalid = torch.empty(max(nrows, 1), dtype=torch.uint8, device=self.device)
        pdict = self.dictionary(project) if project and pmeta.dictionary is not None else None
        if pattr is not None:
            pout = torch.empty(max(nrows, 1), dtype=torch.int32, device=self.device)
            pdict = pattr.values
        if not groups or nrows == 0:
            return ScanOut(nrows, 0, out[:0], {"total_s": time.perf_counter() - t0},
                           values=pout[:0] if pout is not None else
                           (pchars[:0] if pchars is not None else None),
                           column=pmeta, dictionary=pdict,
                           offsets=self._zero() if pstrings else None)
        run = _Run(self._zero(), self._zero(), out=out, cursor=self._zero(),
                   ccursor=self._zero(), pout=pout, pvalid=pvalid, pchars=pchars, poff=poff,
                   owidth=8 if pstrings and pmeta.large else 4, pattr=pattr is not None,
                   pcol=pcol, exprs=self._expr_runs(xm, full, cl))
        if join is not None:
            run.join = self._join_run(join, names, pattr)
        t_alloc = self._drive(groups, spec, run)
        cursor, count, err, nchars = torch.cat([run.cursor, run.count, run.err,
                                                run.ccursor]).tolist()
        secs = self._seconds(run, t0, t_plan, t_alloc)
        self._check_decoded(err, names)
        if cursor != count:
            raise RuntimeError(f"row emit mismatch: {cursor} ids for {count} selected")
        offsets = None
        if pstrings:
            poff[count] = nchars
            offsets = poff[:count + 1]
        # per group: (group, event, ms since the scan's first submit)
        secs["timeline_ms"] = [(k, e, round((t - t_alloc) * 1e3, 3)) for k, e, t in run.marks]
        return ScanOut(nrows, int(count), out[:count], secs,
                       bytes_read=run.bytes_read, column_bytes=run.column_bytes,
                       groups=len(groups),
                       values=pout[:count] if pout is not None else
                       (pchars[:nchars] if pchars is not None else None),
                       valid=pvalid[:count] if pvalid is not None else None,
                       column=pmeta, dictionary=pdict, offsets=offsets,
                       exprs=[x.prog for x in run.exprs])

    def _scan_select(self, quals, project, batches, join, order_by=None, limit=None,
                     offset=0) -> ScanOut:
        """scan_where with a select list: the stages of the single form up to
        the emit, which writes the row ids and every column of the list in
        one walk of each group's bitmap (ops/colproject.py), on the emit
        stream, in group order, behind the shared cursors."""
        items = _select_items(project)
        keys = SO.order_keys(order_by) if order_by is not None else None
        nvis = len(items)
        items = _with_hidden(items, keys)
        order = [(str(n), d) for n, d in keys] if keys else None
        attrs = [it for it in items if isinstance(it, JoinAttr)]
        join = _check_join(self.meta, join, attrs)
        cl = _named_clauses(quals) if (quals or join is None) else []
        t0 = time.perf_counter()
        pnames = [it for it in items if not isinstance(it, JoinAttr)]
        names = _scanned(cl, join, pnames)
        xm = _with_exprs(self.meta, names)
        _order_columns(xm, keys)
        metas = _select_meta(xm, items)
        names, full = _split_names(xm, names)
        cols, nrows, groups = self._resolve(names, batches)
        spec = [[(full.index(p.col), self._compile(p, xm)) for p in c] for c in cl]
        t_plan = time.perf_counter()
        cap = max(nrows, 1)
        new = lambda *shape, dtype: torch.empty(*shape, dtype=dtype, device=self.device)
        out = new(cap, dtype=torch.int64)
        # the row cursor, then one character cursor per string column
        nstr = sum(m is not None and m.kind in ("utf8", "binary") and m.dictionary is None
                   for m in metas)
        cursors = torch.zeros(1 + nstr, dtype=torch.int64, device=self.device)
        sel, outs, k = [], [], 0
        star = isinstance(join, StarJoin)
        for it, m in zip(items, metas):
            if m is None:
                # the joined attribute's codes: int32 per row in the probe's buffer
                si = _SelItem(PJ.FIXED, 4, None, attrs.index(it) if star else -1,
                              out=new(cap, dtype=torch.int32))
                outs.append(ProjOut(it.name, None, None, None, it.values))
                sel.append(si)
                continue
            pcol = full.index(it)
            st = m.storage
            if m.kind in ("utf8", "binary") and m.dictionary is None:
                k += 1
                nch = sum(int(g.aux_len[:, pcol].sum()) for g in groups)
                si = _SelItem(PJ.STR64 if m.large else PJ.STR32, 0, pcol,
                              out=new(cap + 1, dtype=torch.int64),
                              chars=new(max(nch, 1), dtype=torch.uint8), cursor=cursors[k:k + 1])
            elif st == "b1":
                si = _SelItem(PJ.BOOL, 0, pcol, out=new(cap, dtype=torch.uint8))
            elif st == "d16":
                si = _SelItem(PJ.FIXED, 16, pcol, out=new((cap, 2), dtype=torch.int64))
            else:
                si = _SelItem(PJ.FIXED, np.dtype(st).itemsize, pcol, out=new(cap, dtype=_TORCH[st]))
            if m.nullable if pcol >= len(names) else any(bool(g.has_valid[pcol]) for g in groups):
                si.valid = new(cap, dtype=torch.uint8)
            sel.append(si)
            outs.append(ProjOut(str(it), None, None, m,
                                self.dictionary(it) if m.dictionary is not None else None))
        if not groups or nrows == 0:
            for si, po in zip(sel, outs):
                po.values = si.out[:0] if si.chars is None else si.chars[:0]
                po.offsets = self._zero() if si.chars is not None else None
            return ScanOut(nrows, 0, out[:0], {"total_s": time.perf_counter() - t0},
                           columns=outs[:nvis], order=order)
        ptr = lambda x: x.data_ptr() if x is not None else 0
        desc = PJ.proj_cols([(si.kind, si.width, ptr(si.out), ptr(si.valid), ptr(si.chars),
                              ptr(si.cursor)) for si in sel])
        run = _Run(self._zero(), self._zero(), out=out, cursor=cursors[0:1],
                   exprs=self._expr_runs(xm, full, cl), sel=_SelRun(sel, desc))
        if join is not None:
            run.join = self._join_run(join, names, attrs)
        t_alloc = self._drive(groups, spec, run)
        got = torch.cat([run.count, run.err, cursors]).tolist()
        count, err, cursor, nchars = got[0], got[1], got[2], got[3:]
        secs = self._seconds(run, t0, t_plan, t_alloc)
        self._check_decoded(err, names)
        if cursor != count:
            raise RuntimeError(f"row emit mismatch: {cursor} ids for {count} selected")
        k = 0
        for si, po in zip(sel, outs):
            po.valid = si.valid[:count] if si.valid is not None else None
            if si.chars is not None:
                si.out[count] = nchars[k]
                po.values, po.offsets = si.chars[:nchars[k]], si.out[:count + 1]
                k += 1
            else:
                po.values = si.out[:count]
        secs["timeline_ms"] = [(k, e, round((t - t_alloc) * 1e3, 3)) for k, e, t in run.marks]
        indices, errs = out[:count], None
        if keys:
            t_sort = time.perf_counter()
            indices, errs = self._sort_select(keys, items, metas, sel, outs, out, int(count),
                                              limit, offset)
            secs["sort_s"] = time.perf_counter() - t_sort
            secs["total_s"] += secs["sort_s"]
        return ScanOut(nrows, int(count), indices, secs, bytes_read=run.bytes_read,
                       column_bytes=run.column_bytes, groups=len(groups),
                       exprs=[x.prog for x in run.exprs], columns=outs[:nvis], order=order,
                       sort_errors=errs)

    def _sort_select(self, keys, items, metas, sel: List[_SelItem], outs: List[ProjOut],
                     rows: torch.Tensor, n: int, limit, offset) -> tuple:
        """order_by=: the n selected rows the emit left (``rows``, ``sel``,
        ``outs``) sorted by ``keys`` and cut to the window, every ProjOut
        replaced by its gathered copy.  The launches go to the emit stream;
        the current stream waits for them on the device.  Returns (the row
        ids in result order, the gather's error word)."""
        first, cnt = SO.window(n, limit, offset)
        new = lambda *shape, dtype: torch.empty(*shape, dtype=dtype, device=self.device)
        ids = new(max(cnt, 1), dtype=torch.int64)
        st = SO.State(n, self.device)
        if n == 0:
            return ids[:0], st.err
        at = {str(it): k for k, it in enumerate(items) if not isinstance(it, JoinAttr)}
        order = [(T.TYPE_CODE[metas[at[str(nm)]].storage], sel[at[str(nm)]].out,
                  sel[at[str(nm)]].valid, desc) for nm, desc in keys]
        specs, strs = [], []
        for si, po in zip(sel, outs):
            v = new(max(cnt, 1), dtype=torch.uint8) if si.valid is not None else None
            if si.chars is not None:
                # the permuted lengths behind a leading zero: their running sum
                # is the output offsets
                off = torch.zeros(cnt + 1, dtype=torch.int64, device=self.device)
                ch = new(max(po.values.numel(), 4), dtype=torch.uint8)
                specs.append((SO.LEN, 0, si.out.data_ptr(), off[1:].data_ptr(),
                              si.valid.data_ptr() if v is not None else 0,
                              v.data_ptr() if v is not None else 0))
                strs.append((si, po, off, ch))
                po.offsets = off
            else:
                o = new((max(cnt, 1),) + tuple(si.out.shape[1:]), dtype=si.out.dtype)
                width = si.out.element_size() * (2 if si.out.dim() == 2 else 1)
                specs.append((SO.FIXED, width, si.out.data_ptr(), o.data_ptr(),
                              si.valid.data_ptr() if v is not None else 0,
                              v.data_ptr() if v is not None else 0))
                po.values = o[:cnt]
            po.valid = v[:cnt] if v is not None else None
        if cnt == 0:
            # an empty window: nothing to order, nothing to gather
            for si, po, off, ch in strs:
                po.values = ch[:0]
            return ids[:0], st.err
        es = self._emit_stream()
        cur = torch.cuda.current_stream(self.device)
        es.wait_stream(cur)
        with torch.cuda.stream(es):
            SO.order(st, order, stream=es)
            SO.apply(st.order, n, first, cnt, rows, ids, SO.sort_cols(specs), st.err, stream=es)
            for si, po, off, ch in strs:
                off[1:].cumsum_(0)
                SO.chars(st.order, n, first, cnt, si.out, si.chars, po.values.numel(), off, ch,
                         stream=es)
                po.values = ch[:po.values.numel()]
        cur.wait_stream(es)
        return ids[:cnt], st.err

    def aggregate(self, quals, aggs, by=None, batches: Optional[Tuple[int, int]] = None,
                  join: Union[Join, StarJoin, None] = None) -> "AggOut":
        """``SELECT by, aggs... WHERE quals GROUP BY by`` in one pass over
        the file: the qualifier, aggregated and key columns are read and
        decoded once per group, the qualifier kernels leave the selection
        bitmap and the aggregate kernels (csrc/kernels/colagg.hip) consume
        it on the slot's stream — no row ids are written, a few kilobytes of
        accumulators stay on the device until the scan's one sync.

        ``quals`` as in scan_where; an empty list selects every row.
        ``aggs``: ``(fn, column)`` with fn ``count`` (column None: count(*)),
        ``sum``, ``min``, ``max``, ``mean``.  sum / min / max take integer
        and float columns, min / max also date / time / timestamp / duration
        (their ticks); count takes any column.  Integer sums wrap in 64
        bits, float sums are float64; NaN propagates into a sum and is
        ignored by min / max; nulls are skipped.  ``by``: a
        dictionary-encoded, bool or 8-bit integer column (null keys form a
        group of their own, key None), or ``HashBy(col, groups)`` for an
        ordinary integer or temporal column of up to ``groups`` distinct
        values: a hash table in HBM (csrc/kernels/colgroup.hip) gives each
        row a code and the accumulators are updated with global atomics —
        rows come back ascending by key, the null group last, and float sums
        are not bitwise reproducible from run to run (the keyed LDS path's are
        not either).  More than ``groups`` distinct keys raise RuntimeError at
        the scan's sync; there is no retry.  ``HashBy([a, b, ...])`` groups by
        up to four such columns (or one attribute of the semi-join among
        them) packed into the table's key word: ``AggOut.keys`` are tuples in
        lexicographic order, nulls last per column, ``AggOut.key_columns``
        the same as arrays; a selected value outside a declared ``bits=``
        raises RuntimeError at the sync.  ``join=`` as in scan_where: only the
        joined rows are aggregated, and ``by=dim[attr]`` groups them by an
        attribute of the JoinTable — the probe writes each row's attribute
        code into the slot's key buffer and the aggregate kernels take it as
        their key column.  With ``join=StarJoin(...)`` each attribute leg
        writes a code buffer of its own, and ``HashBy([dimA[x], dimB[y], ...])``
        groups by attributes of different JoinTables.

        Where a column is named, an expression (ops/colexpr.E) may stand: as
        the column of an aggregate (``("sum", E("price") * E("qty"))``), in a
        qualifier, as the key of ``HashBy`` (int64 expressions) or one of its
        components (``bits={expr: n}``).  ``by=`` itself takes no expression:
        the LDS-slot GROUP BY needs a stored key column.  At most four
        distinct expressions per scan; one that a qualifier and an aggregate
        share is computed once.  See AggOut."""
        t0 = time.perf_counter()
        battr = by if isinstance(by, JoinAttr) else None
        hb = by if isinstance(by, HashBy) else None
        jattrs = battr if hb is None else hb.attrs
        join = _check_join(self.meta, join, jattrs)
        if battr is not None or hb is not None:
            by = None
        cl = _named_clauses(quals) if quals else []
        aggs, xm = _agg_exprs(self.meta, cl, aggs, by, hb)
        agg = _agg_spec(xm, aggs, by, self.dictionary, battr, hb)
        names = _scanned(cl, join, agg.names)
        names, full = _split_names(xm, names)
        cols, nrows, groups = self._resolve(names, batches)
        if not names:
            # count(*) of everything: the footer answers
            block = A.new_block(agg.layout)
            block[agg.layout.pos(0, A.COUNT)] = np.uint64(nrows)
            return _agg_out(agg, block, nrows, {"total_s": time.perf_counter() - t0})
        spec = [[(full.index(p.col), self._compile(p, xm)) for p in c] for c in cl]
        t_plan = time.perf_counter()
        if not groups or nrows == 0:
            secs = {"total_s": time.perf_counter() - t0}
            if hb is None:
                return _agg_out(agg, A.new_block(agg.layout), nrows, secs)
            return _hash_out(agg, G.empty_groups(agg.layout.entries, agg.hash_unsigned,
                                                 agg.keyspec), nrows, secs)
        agg.entry_cols = [None if n is None else full.index(n) for n in agg.entry_names]
        # by=dim[attr]: no file column, the key is the probe's code buffer
        agg.key_col = full.index(by) if by is not None else None
        run = _Run(self._zero(), self._zero(), agg=agg, exprs=self._expr_runs(xm, full, cl))
        if join is not None:
            run.join = self._join_run(join, names, jattrs)
        # the block is initialised on the emit stream, where the reduces follow
        es = self._emit_stream()
        with torch.cuda.stream(es):
            run.block = A.alloc_block(agg.layout, self.device, stream=es)
            dev = None
            if hb is not None:
                # the table and its accumulators, initialised before any
                # launch can see a slot (block_ready below)
                dev = G.DeviceGroups(agg.layout.entries, hb.groups, self.device,
                                     agg.hash_unsigned, stream=es, spec=agg.keyspec)
        if agg.keyspec is not None:
            # a StarJoin's attribute legs write leg buffers 0, 1, ... in the
            # order of the components; a Join's one attribute the key buffer
            star = isinstance(join, StarJoin)
            run.hash = _HashRun(-1, 0, dev, [None if isinstance(c, JoinAttr) else
                                             full.index(c) for c in hb.comps],
                                [hb.attrs.index(c) if star and isinstance(c, JoinAttr) else -1
                                 for c in hb.comps])
        elif hb is not None:
            kc = xm.schema[xm.column_index(hb.col)]
            run.hash = _HashRun(full.index(hb.col), G.KEY_CODE[kc.storage], dev)
        run.block_ready = torch.cuda.Event()
        run.block_ready.record(es)
        t_alloc = self._drive(groups, spec, run)
        if dev is not None:
            # behind the last group on the emit stream: the occupied slots
            # and the two reserved codes, compacted; only they and the header
            # are read back
            with torch.cuda.stream(es):
                hdr, found = G.compact(dev)
        err = int(run.err.item())
        host = A.block_to_host(run.block)
        secs = self._seconds(run, t0, t_plan, t_alloc)
        self._check_decoded(err, names)
        moved = dict(bytes_read=run.bytes_read, column_bytes=run.column_bytes, groups=len(groups))
        if dev is None:
            return _agg_out(agg, host, nrows, secs, **moved)
        _check_groups(hb, int(hdr[G.H_NKEYS]), int(hdr[G.H_OVERFLOW]))
        if agg.keyspec is not None:
            _check_range(agg.keyspec, hdr[G.H_RANGE:G.H_RANGE + len(agg.keyspec)])
        return _hash_out(agg, found, nrows, secs, **moved)

    def host_aggregate(self, quals, aggs, by=None, batches: Optional[Tuple[int, int]] = None,
                       join: Union[Join, StarJoin, None] = None) -> "AggOut":
        """The same query on the CPU (host_scan_where's path plus the
        aggregate kernels' numpy twin, ops/colagg.py)."""
        return host_aggregate(self.path, quals, aggs, by, batches, meta=self.meta,
                              dicts=self._dicts, join=join)

    def top(self, quals, order_by: str, k: int, descending: bool = False, project=None,
            batches: Optional[Tuple[int, int]] = None, join: Union[Join, StarJoin, None] = None) -> "TopOut":
        """``SELECT row, order_by[, project] WHERE quals ORDER BY order_by
        [DESC] LIMIT k`` in one pass: the first ``k`` of the selected rows by
        (a value before a NaN before a null — in both directions —, the value
        ascending or descending, the file-global row id ascending), which is
        ``pyarrow.compute.sort_indices`` with its default null placement,
        cut to ``k``.  -0.0 and +0.0 are equal; integers compare by value,
        uint64 over its whole range, temporal columns by their ticks.

        Per group a selection kernel (csrc/kernels/coltopk.hip) on the slot's
        stream leaves each workgroup's ``k`` best candidates, a merge on the
        emit stream folds them into the scan's state of ``k`` candidates and
        tightens the threshold the later groups' launches read; the state's
        few KB are read back at the scan's one sync.  No row ids are written
        and nothing of the table's height is allocated.

        ``order_by``: a non-dictionary int8-64, uint8-64, float32/64, date,
        time, timestamp or duration column.  ``k``: 1 .. ops.coltopk.MAX_K;
        more than the selected rows returns them all, sorted.  ``project``:
        one column carried with each candidate — fixed-width of at most 8
        bytes, a dictionary-encoded column's indices (``TopOut.dictionary``
        holds the values) or ``dim[attr]`` of the semi-join.  ``quals`` (may
        be empty), ``batches`` and ``join`` as in scan_where.  One order
        column, no OFFSET: ``scan_where(order_by=, limit=)`` sorts by several
        columns and serves k beyond MAX_K.  ``order_by`` (and ``project``, and a qualifier's
        column) may be an expression (ops/colexpr.E), computed on the device
        per group: a float64 one orders its NaNs and nulls as a stored column's.
        See TopOut."""
        t0 = time.perf_counter()
        k = T.check_k(k)
        pattr = project if isinstance(project, JoinAttr) else None
        join = _check_join(self.meta, join, pattr)
        if pattr is not None:
            project = None
        order_by, project = _order_name(order_by), name_of(project)
        cl = _named_clauses(quals) if quals else []
        names = _scanned(cl, join, [order_by] + ([project] if project else []))
        xm = _with_exprs(self.meta, names)
        spec_out = _top_spec(xm, order_by, k, descending, project, pattr, self.dictionary)
        names, full = _split_names(xm, names)
        cols, nrows, groups = self._resolve(names, batches)
        spec = [[(full.index(p.col), self._compile(p, xm)) for p in c] for c in cl]
        t_plan = time.perf_counter()
        none = np.zeros((0, T.ENTRY_WORDS), np.uint64)
        if not groups or nrows == 0:
            return _top_out(spec_out, none, nrows, 0, {"total_s": time.perf_counter() - t0})
        # the state is initialised on the emit stream, where the merges follow
        es = self._emit_stream()
        with torch.cuda.stream(es):
            state = T.init(k, self.device, stream=es)
        run = _Run(self._zero(), self._zero(), exprs=self._expr_runs(xm, full, cl))
        run.top = _TopRun(full.index(order_by), T.TYPE_CODE[spec_out.column.storage],
                          bool(descending), state,
                          full.index(project) if project else None,
                          4 if pattr is not None else
                          (np.dtype(spec_out.pcolumn.storage).itemsize if project else 0),
                          pattr is not None)
        if join is not None:
            run.join = self._join_run(join, names, pattr)
        # the select launches (slot streams) read the state's threshold: they
        # must see it initialised
        run.block_ready = torch.cuda.Event()
        run.block_ready.record(es)
        t_alloc = self._drive(groups, spec, run)
        host = torch.cat([state.words, run.err]).cpu().numpy()
        secs = self._seconds(run, t0, t_plan, t_alloc)
        self._check_decoded(int(host[-1]), names)
        words = host[:-1].view(np.uint64)
        if int(words[T.H_ERRORS]) or int(words[T.H_MERGES]) != len(groups):
            raise RuntimeError(f"top-k state: {int(words[T.H_ERRORS])} slab(s) refused, "
                               f"{int(words[T.H_MERGES])} merges for {len(groups)} groups")
        secs["timeline_ms"] = [(i, e, round((t - t_alloc) * 1e3, 3)) for i, e, t in run.marks]
        return _top_out(spec_out, T.state_entries(words).copy(), nrows, int(words[T.H_SEEN]), secs,
                        bytes_read=run.bytes_read, column_bytes=run.column_bytes,
                        groups=len(groups))

    def host_top(self, quals, order_by: str, k: int, descending: bool = False, project=None,
                 batches: Optional[Tuple[int, int]] = None,
                 join: Union[Join, StarJoin, None] = None) -> "TopOut":
        """The same query on the CPU (the host twins' scan, the candidates'
        numpy twin, ops/coltopk.py)."""
        return host_top(self.path, quals, order_by, k, descending, project, batches,
                        meta=self.meta, dicts=self._dicts, join=join)

    def scan(self, name: str, lo, hi) -> ScanOut:
        """Row ids (int64, file order) of ``lo <= column <= hi`` (nulls never
        qualify)."""
        return self.scan_where([(name, lo, hi)])

    # the pre-pipeline name
    filter = scan

    def host_scan_where(self, quals, project=None, batches: Optional[Tuple[int, int]] = None,
                        join: Union[Join, StarJoin, None] = None, order_by=None,
                        limit: Optional[int] = None, offset: int = 0) -> "HostScanOut":
        """The same query on the CPU (buffers read with pread, decoded by
        the decoders' host twins, predicates by colpred's numpy twin, the
        join by coljoin's)."""
        return host_scan_where(self.path, quals, project, batches, meta=self.meta,
                               dicts=self._dicts, join=join, order_by=order_by, limit=limit,
                               offset=offset)

    def _free_slots(self) -> None:
        if self._slots:
            self._hbm.close()
        self._slots = []

    def close(self) -> None:
        self._free_slots()
        if self.reader is not None:
            self.reader.close()
            self.reader = None
        if getattr(self, "_pfd", None) is not None:
            os.close(self._pfd)
            self._pfd = None


# ------------------------------------------------------------ host twin
@dataclass
class HostScanOut:
    rows: int
    indices: np.ndarray                # int64 global row ids
    values: object = None              # projected values (numpy; strings: list of bytes)
    valid: Optional[np.ndarray] = None
    dictionary: object = None          # project=dim[attr]: the value of each code
    exprs: list = field(default_factory=list)   # the computed columns' Programs
    # project=[...]: one ProjOut of numpy arrays per item, laid out as the
    # device scan's (values / valid / dictionary above are then None)
    columns: Optional[List[ProjOut]] = None
    order: Optional[List[Tuple[str, bool]]] = None   # order_by=, normalized

    def to_arrow(self):
        """The select list's columns as a pyarrow.Table (ScanOut.to_arrow)."""
        if self.columns is None:
            raise ValueError("to_arrow: host_scan_where(project=[...]) assembles a table")
        return _arrow_table(self.columns)


def _check_order_args(project, order_by, limit, offset) -> None:
    """What scan_where / host_scan_where take of order_by / limit / offset,
    checked before anything else."""
    SO.window(0, limit, offset)
    if order_by is None:
        if limit is not None or offset:
            raise ValueError("limit= / offset= cut a sorted result: they need order_by=")
        return
    if not isinstance(project, (list, tuple)):
        raise ValueError("order_by= needs the list form of project= (project=[...]): the sort "
                         "gathers a select list's columns")


def _with_hidden(items: list, keys) -> list:
    """The select list followed by the order columns it does not name."""
    if not keys:
        return items
    shown = [str(it) for it in items if not isinstance(it, JoinAttr)]
    items = items + [n for n, _ in keys if str(n) not in shown]
    if len(items) > PJ.MAX_COLS:
        raise NotImplementedError(f"a select list of {len(shown)} columns and {len(items)} with "
                                  f"the order columns outside it: at most {PJ.MAX_COLS} are "
                                  "gathered in one emit pass")
    return items


def _order_columns(meta, keys) -> None:
    """The order columns' kinds, checked before anything is read: what
    ``top`` orders."""
    schema = {c.name: c for c in meta.schema}
    for name, _ in keys or []:
        if name not in schema:
            raise ValueError(f"no column {str(name)!r}")
        c = schema[name]
        if c.dictionary is not None or c.kind not in ("int", "float") + _TEMPORAL or \
                c.storage not in T.TYPE_CODE:
            kind = "dictionary-encoded" if c.dictionary is not None else c.kind
            raise NotImplementedError(f"ORDER BY {name}: {kind} columns are not ordered on the "
                                      "GPU (integer, float32/64, date, time, timestamp and "
                                      "duration columns are)")


def _host_select(path: str, quals, project, batches, meta: ArrowFile, dicts: dict,
                 join, order_by=None, limit=None, offset=0) -> HostScanOut:
    """host_scan_where with a select list: every column gathered per record
    batch with the rows the qualifiers and the join select, in the layout of
    the device scan's ProjOut."""
    items = _select_items(project)
    keys = SO.order_keys(order_by) if order_by is not None else None
    nvis = len(items)
    items = _with_hidden(items, keys)
    attrs = [it for it in items if isinstance(it, JoinAttr)]
    join = _check_join(meta, join, attrs)
    cl = _named_clauses(quals) if (quals or join is None) else []
    pnames = [it for it in items if not isinstance(it, JoinAttr)]
    meta = _with_exprs(meta, [p.col for c in cl for p in c] + pnames)
    _order_columns(meta, keys)
    metas = _select_meta(meta, items)
    base = np.concatenate([[0], np.cumsum(meta.rows)]).astype(np.int64)
    nrows = 0
    ids: List[np.ndarray] = []
    parts: List[list] = [[] for _ in items]
    for bi, b, data, m, jrow in _host_batches(path, meta, dicts, cl, join, pnames, batches):
        nrows += b.length
        sel = np.flatnonzero(m)
        ids.append(sel + base[bi])
        for k, (it, c) in enumerate(zip(items, metas)):
            if c is None:
                codes = it.codes[jrow[_leg_of(join, it)][sel]] if len(it.codes) else \
                    np.zeros(0, np.int32)
                parts[k].append((codes.astype(np.int32), None, None))
                continue
            v, ok = data[it]
            okb = ok[sel].astype(np.uint8) if ok is not None else np.ones(len(sel), np.uint8)
            if isinstance(v, tuple):
                offs, chars = v
                a = offs[sel]
                ln = offs[sel + 1] - a if len(sel) else a
                st = np.cumsum(ln) - ln
                idx = np.repeat(a - st, ln) + np.arange(int(ln.sum()))
                parts[k].append((ln, okb, np.asarray(chars)[idx]))
            elif c.kind == "decimal" and c.dictionary is None:
                raw = b"".join(int(x).to_bytes(16, "little", signed=True) for x in v[sel])
                parts[k].append((np.frombuffer(raw, "<i8").reshape(-1, 2), okb, None))
            else:
                x = np.asarray(v)[sel]
                parts[k].append((x.astype(np.uint8) if c.kind == "bool" and c.dictionary is None
                                 else x, okb, None))
    cols = []
    for it, c, p in zip(items, metas, parts):
        if c is None:
            cols.append(ProjOut(it.name, np.concatenate([x[0] for x in p]) if p else
                                np.zeros(0, np.int32), None, None, it.values))
            continue
        ok = np.concatenate([x[1] for x in p]) if p else np.zeros(0, np.uint8)
        po = ProjOut(str(it), None, None if ok.all() else ok, c,
                     _dictionary(meta, path, dicts, it) if c.dictionary is not None else None)
        if c.kind in ("utf8", "binary") and c.dictionary is None:
            ln = np.concatenate([x[0] for x in p]) if p else np.zeros(0, np.int64)
            po.values = np.concatenate([x[2] for x in p]) if p else np.zeros(0, np.uint8)
            po.offsets = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
        elif p:
            po.values = np.concatenate([x[0] for x in p])
        else:
            st = c.storage
            po.values = np.zeros((0, 2), np.int64) if st == "d16" else \
                np.zeros(0, np.uint8 if st == "b1" else st)
        cols.append(po)
    rows = np.concatenate(ids) if ids else np.zeros(0, np.int64)
    if keys:
        # the twin's order (coltopk's encoding, np.lexsort), then every column
        at = {str(it): k for k, it in enumerate(items) if not isinstance(it, JoinAttr)}
        perm = SO.host_order([(cols[at[str(n)]].values, cols[at[str(n)]].valid, d)
                              for n, d in keys], len(rows))
        first, cnt = SO.window(len(rows), limit, offset)
        rows = rows[perm[first:first + cnt]]
        for po in cols:
            po.values, po.valid, po.offsets = SO.host_apply(perm, first, cnt, po.values, po.valid,
                                                            po.offsets)
    return HostScanOut(nrows, rows, exprs=list(getattr(meta, "progs", {}).values()),
                       columns=cols[:nvis],
                       order=[(str(n), d) for n, d in keys] if keys else None)


def _order_name(order_by):
    """``order_by`` of top / host_top as a column name."""
    if not isinstance(order_by, (str, E)):
        raise NotImplementedError("ORDER BY one column (a list of order columns is not supported)")
    return name_of(order_by)


def _agg_exprs(meta: ArrowFile, cl, aggs, by, hb: Optional[HashBy]) -> tuple:
    """(``aggs`` with expressions by their names, the metadata with the
    computed columns of the qualifiers ``cl``, the aggregates and the HashBy
    key) of aggregate / host_aggregate."""
    if isinstance(by, (E, ExprName)):
        raise NotImplementedError(f"GROUP BY {by!r}: by= names a stored key column (its values "
                                  "index accumulators in LDS); by=HashBy(expression) groups by a "
                                  "computed one")
    aggs = [(fn, name_of(col)) for fn, col in aggs]
    keys = [] if hb is None else ([hb.col] if hb.comps is None else
                                  [c for c in hb.comps if not isinstance(c, JoinAttr)])
    return aggs, _with_exprs(meta, [p.col for c in cl for p in c] + [c for _, c in aggs] + keys)


def _host_join(join: Join, v, ok, m: np.ndarray):
    """(rows of ``m`` the join keeps, build row per row) for one batch's
    foreign keys ``v`` / validity ``ok``."""
    keys, can = J.widen(np.asarray(v))
    act = m & can & (np.ones(len(m), bool) if ok is None else np.asarray(ok, bool))
    match, row = J.host_lookup(join.table.host(), keys, act)
    return (m & ~match if join.how == "anti" else m & match), row


def _scanned(cl, join, more: Sequence[str]) -> List[str]:
    """The columns a scan reads, each once: the qualifiers', the foreign keys
    of the join's legs, then ``more`` — the order of the plan's columns."""
    return list(dict.fromkeys([p.col for c in cl for p in c] + [j.col for j in _legs(join)] +
                              list(more)))


def _dictionary(meta: ArrowFile, path: str, dicts: dict, name: str):
    """Decoded dictionary of a dictionary-encoded column, cached in ``dicts``."""
    if name not in dicts:
        dicts[name] = dictionary_values(meta, meta.schema[meta.column_index(name)], path)
    return dicts[name]


def _compile_pred(p: Pred, col: Column, dictionary) -> Compiled:
    """compile_pred with the column's dictionary (``dictionary(name)``) where
    the predicate looks at values: a null test needs none."""
    dic = dictionary(p.col) if (col.dictionary is not None and
                                p.op not in ("is_null", "is_valid")) else None
    return compile_pred(p, col, dic)


def _host_batches(path: str, meta: ArrowFile, dicts: dict, cl, join,
                  more: Sequence[str], batches: Optional[Tuple[int, int]],
                  values=lambda name: True):
    """The host twins' scan: per record batch of the range (batch index,
    batch, {column: (values, validity)}, the rows the CNF ``cl`` and the join
    select, per leg of the join its build row per row, or None).  The legs are
    applied in turn, each to the rows the ones before it left.  The qualifier and join
    columns and ``more`` are read and decoded; a column of ``more`` for which
    ``values(name)`` is false gets its validity alone (values None)."""
    schema = {c.name: (i, c) for i, c in enumerate(meta.schema)}
    dictionary = lambda name: _dictionary(meta, path, dicts, name)
    comp = []
    for c in cl:
        for p in c:
            if p.col not in schema:
                raise ValueError(f"no column {p.col!r}")
        comp.append([(p.col, _compile_pred(p, schema[p.col][1], dictionary)) for p in c])
    # computed columns (meta: _with_exprs): their sources are read whole,
    # they themselves come from the kernel's numpy twin
    progs = getattr(meta, "progs", {})
    must = (set(_scanned(cl, join, [])) | {c for p in progs.values() for c in p.columns}) - \
        set(progs)
    more = [n for n in more if n not in progs]
    nb = meta.nbatches
    b0, b1 = (0, nb) if batches is None else (max(0, batches[0]), min(nb, batches[1]))
    src = _Src(path)
    try:
        for bi in range(b0, b1):
            b = meta.batches[bi]
            data = {}
            for n in sorted(must | set(more)):
                ci, col = schema[n]
                ch = b.columns[ci]
                vraw = read_buffer(src, ch.validity, b.codec) if ch.null_count else b""
                ok = validity_bits(vraw, ch.length)
                if n not in must and not values(n):
                    data[n] = (None, ok)
                    continue
                d = read_buffer(src, ch.data, b.codec)
                vcol = col if col.dictionary is None else Column(n, "int", col.dictionary.index_bits,
                                                                 col.dictionary.index_signed)
                x = read_buffer(src, ch.extra, b.codec) if (ch.extra is not None and
                                                            col.dictionary is None) else b""
                data[n] = (decode_values(vcol, ch.length, d, x), ok)
            for n, p in progs.items():
                data[n] = host_expr(p, [data[c][0] for c in p.columns],
                                    [data[c][1] for c in p.columns], b.length)
            m = np.ones(b.length, bool)
            for c in comp:
                cm = np.zeros(b.length, bool)
                for name, cq in c:
                    v, ok = data[name]
                    cm |= evaluate(cq, v, ok, b.length)
                m &= cm
            jrow = None
            if join is not None:
                jrow = []
                for leg in _legs(join):
                    m, row = _host_join(leg, *data[leg.col], m)
                    jrow.append(row)
            yield bi, b, data, m, jrow
    finally:
        src.close()


def host_scan_where(path: str, quals, project=None,
                    batches: Optional[Tuple[int, int]] = None, meta: Optional[ArrowFile] = None,
                    dicts: Optional[dict] = None, join: Union[Join, StarJoin, None] = None,
                    order_by=None, limit: Optional[int] = None, offset: int = 0) -> HostScanOut:
    """ArrowScan.scan_where on the CPU: the same metadata, the same
    compiled predicates (ops/colpred.py), evaluated by the kernel's numpy
    twin over buffers decoded by the GPU decoders' host twins.  The
    reference point for the GPU path and a scan for machines without one."""
    _check_order_args(project, order_by, limit, offset)
    meta = meta if meta is not None else read_metadata(path)
    dicts = dicts if dicts is not None else {}
    if isinstance(project, (list, tuple)):
        return _host_select(path, quals, project, batches, meta, dicts, join, order_by, limit,
                            offset)
    pattr = project if isinstance(project, JoinAttr) else None
    join = _check_join(meta, join, pattr)
    if pattr is not None:
        project = None
    project = name_of(project)
    cl = _named_clauses(quals) if (quals or join is None) else []
    meta = _with_exprs(meta, [p.col for c in cl for p in c] + ([project] if project else []))
    base =np.concatenate([[0], np.cumsum(meta.rows)]).astype(np.int64)
    nrows = 0
    ids, vals, valid = [], [], []
    pleg = _leg_of(join, pattr) if pattr is not None else None
    for bi, b, data, m, jrow in _host_batches(path, meta, dicts, cl, join,
                                              [project] if project else [], batches):
        nrows += b.length
        sel = np.flatnonzero(m)
        ids.append(sel + base[bi])
        if pattr is not None:
            vals.append(pattr.codes[jrow[pleg][sel]] if len(pattr.codes) else
                        np.zeros(0, np.int32))
            valid.append(np.ones(len(sel), bool))
        if project:
            v, ok = data[project]
            if isinstance(v, tuple):
                offs, chars = v
                vals.append([chars[offs[i]:offs[i + 1]].tobytes() for i in sel])
            else:
                vals.append(np.asarray(v)[sel])
            valid.append(ok[sel] if ok is not None else np.ones(len(sel), bool))
    out = HostScanOut(nrows, np.concatenate(ids) if ids else np.zeros(0, np.int64),
                      exprs=list(getattr(meta, "progs", {}).values()))
    if pattr is not None:
        out.dictionary = pattr.values
    if project or pattr is not None:
        if vals and isinstance(vals[0], list):
            out.values = [x for v in vals for x in v]
        else:
            out.values = np.concatenate(vals) if vals else np.zeros(0, np.int32 if pattr else None)
        vv = np.concatenate(valid) if valid else np.zeros(0, bool)
        out.valid = None if vv.all() else vv
    return out


# ------------------------------------------------------------ aggregation
_AGG_FNS = {"count": A.COUNT, "sum": A.SUM, "min": A.MIN, "max": A.MAX, "mean": A.SUM}
_TEMPORAL = ("date", "time", "timestamp", "duration")


def _all_rows_bitmap(rows: np.ndarray) -> np.ndarray:
    """The bitmap that selects every row: each batch on fresh words, its
    last word bounded by its rows."""
    rows = np.asarray(rows, np.int64)
    words = (rows + 63) // 64
    out = np.full(int(words.sum()), 0xFFFFFFFFFFFFFFFF, np.uint64)
    last = np.cumsum(words) - 1
    tail = rows % 64
    m = (tail != 0) & (words > 0)
    out[last[m]] = (np.uint64(1) << tail[m].astype(np.uint64)) - np.uint64(1)
    return out.view(np.int64)


@dataclass
class _AggSpec:
    aggs: List[Tuple[str, Optional[str]]]
    by: Optional[str]
    layout: A.Layout
    entry_names: List[Optional[str]]        # entry 0: count(*), then one per column
    names: List[str]                        # columns the aggregation reads
    cols: Dict[str, Column]
    keyvals: Optional[list] = None          # key of each non-null slot
    entry_cols: Optional[List[Optional[int]]] = None    # plan column of each entry (GPU)
    key_col: Optional[int] = None
    slab_words: Dict[int, List[int]] = field(default_factory=dict)   # by group words
    join_attr: bool = False                 # ``by`` names a JoinTable attribute
    hashed: bool = False                    # by=HashBy(by): layout / keyvals per result
    hash_unsigned: bool = False             # its keys are uint64
    keyspec: Optional[G.KeySpec] = None     # by=HashBy([...]): how the components are packed
    key_attrs: Optional[list] = None        # per component: a join attribute's values, or None
    exprs: list = field(default_factory=list)   # the query's computed columns (Programs)


def _check_range(spec: G.KeySpec, misfit) -> None:
    """Raise for selected rows that a component's declared width could not
    hold (they were left out of every group)."""
    for c, n in zip(spec.comps, np.asarray(misfit).tolist()):
        if n:
            what = f"declared bits={c.bits}" + ("" if c.nullable else ", no nulls")
            raise RuntimeError(f"GROUP BY key component {c.name} ({what}): {int(n)} selected "
                               "row(s) with a value outside that range; scan again with a larger "
                               f"bits={{{c.name!r}: n}}")


def _check_groups(hb: HashBy, nkeys: int, overflow: int = 0) -> None:
    """Raise for a scan that met more distinct keys than ``hb.groups`` (or
    whose table had no slot left for ``overflow`` selected rows)."""
    if nkeys > hb.groups or overflow:
        seen = f"{nkeys} distinct keys seen" if not overflow else \
            f"the table is full ({nkeys} keys in it, {overflow} selected row(s) found no slot)"
        raise RuntimeError(f"GROUP BY HashBy({hb.col!r}): more than groups={hb.groups} "
                           f"distinct keys: {seen}; scan again with a larger groups=")


def _hash_key(schema: dict, name: str, shown: str, others: str = "") -> Column:
    """The column ``name`` as a HashBy key (``shown`` in the error's text,
    ``others``: where the refused kinds are grouped instead)."""
    if name not in schema:
        raise ValueError(f"no column {name!r}")
    k = schema[name]
    if k.dictionary is not None or k.kind not in ("int",) + _TEMPORAL or \
            k.storage not in G.KEY_CODE:
        kind = "dictionary-encoded" if k.dictionary is not None else k.kind
        raise NotImplementedError(
            f"GROUP BY HashBy({shown}): {kind} keys (integer and date / time / timestamp / "
            f"duration columns are hashed{others})")
    return k


def _key_spec(meta: ArrowFile, hb: HashBy) -> Tuple[G.KeySpec, list]:
    """The KeySpec of by=HashBy([...]) against the schema, and per component
    its join attribute's values (None for a column).  A column is nullable if
    any record batch of the file has nulls in it — the whole file, whatever
    range is scanned, so that results of its ranges pack alike and merge."""
    schema = {c.name: c for c in meta.schema}
    comps, attrs = [], []
    for c, shown in zip(hb.comps, hb.col):
        if isinstance(c, JoinAttr):
            nv = max(len(c.values), 1)
            # codes 0 .. nv - 1, never negative: an unsigned field over the
            # probe's int32 buffer
            # ``shown``: the attribute's name, qualified when another component
            # carries the same
            comps.append((shown, "u4", max(1, int(nv - 1).bit_length()), False))
            attrs.append(list(c.values))
            continue
        k = _hash_key(schema, c, f"..., {c}, ...")
        ci = meta.column_index(c)
        nullable = bool(meta.nbatches) and bool(np.any(np.asarray(meta.columns[ci].null_count)))
        comps.append((c, k.storage, hb.bits.get(c), nullable))
        attrs.append(None)
    return G.KeySpec(comps), attrs


def _agg_spec(meta: ArrowFile, aggs, by: Optional[str], dictionary,
              jattr: Optional[JoinAttr] = None, hb: Optional[HashBy] = None) -> _AggSpec:
    """Validate ``aggs`` / ``by`` against the schema and lay the accumulator
    block out: entry 0 counts the selected rows per slot, then one entry per
    aggregated column with COUNT and whatever of SUM / MIN / MAX is asked."""
    schema = {c.name: c for c in meta.schema}
    aggs = [(str(fn), col) for fn, col in aggs]
    if not aggs:
        raise ValueError("at least one aggregate")
    ops: Dict[str, int] = {}
    for fn, col in aggs:
        if fn not in _AGG_FNS:
            raise ValueError(f"aggregate {fn!r}: one of {sorted(_AGG_FNS)}")
        if col is None:
            if fn != "count":
                raise ValueError(f"{fn} needs a column")
            continue
        if col not in schema:
            raise ValueError(f"no column {col!r}")
        c = schema[col]
        if not c.supported:
            raise NotImplementedError(f"column {col}: {c.kind} columns are not scanned on the GPU")
        if fn != "count":
            kind = "dictionary-encoded" if c.dictionary is not None else c.kind
            if c.dictionary is not None or c.kind in ("utf8", "binary", "bool", "decimal") or \
                    c.storage not in A.VALUE_CODE:
                raise NotImplementedError(f"{fn}({col}): {kind} columns have count only")
            if c.kind in _TEMPORAL and fn in ("sum", "mean"):
                raise NotImplementedError(f"{fn}({col}): {c.kind} columns have min, max and count")
        ops[col] = ops.get(col, A.COUNT) | _AGG_FNS[fn]
    nslots, key_code, keyvals = 1, 0, None
    if by is not None:
        if by not in schema:
            raise ValueError(f"no column {by!r}")
        k = schema[by]
        if k.dictionary is not None:
            vals, dvalid = dictionary(by)
            if isinstance(vals, tuple):
                offs, chars = vals
                raw = [chars[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1)]
                keyvals = [r.decode() for r in raw] if k.kind == "utf8" else raw
            else:
                keyvals = np.asarray(vals).tolist()
            if dvalid is not None:
                keyvals = [v if ok else None for v, ok in zip(keyvals, dvalid)]
            key_code = COL_CODE[k.storage]
        elif k.kind == "bool":
            keyvals, key_code = [False, True], A.COL_BOOL
        elif k.kind == "int" and k.bit_width == 8:
            # the slot is the value's byte
            b = np.arange(256, dtype=np.uint8)
            keyvals = (b.view(np.int8) if k.signed else b).tolist()
            key_code = COL_CODE["u1"]
        else:
            raise NotImplementedError(
                f"GROUP BY {by}: {k.kind} keys (dictionary-encoded, bool and 8-bit integer "
                "columns are grouped on the GPU by name; by=HashBy(column) groups an integer "
                "or temporal column of any width)")
        nslots = len(keyvals) + 1
    keyspec = key_attrs = None
    if hb is not None and jattr is not None:
        raise ValueError("by=: a JoinTable attribute or HashBy, not both")
    if hb is not None and hb.comps is not None:
        keyspec, key_attrs = _key_spec(meta, hb)
    elif hb is not None:
        _hash_key(schema, hb.col, hb.col, "; dictionary-encoded, bool and 8-bit columns are "
                                          "grouped by name")
    if jattr is not None:
        # the key column is the probe's int32 code buffer; every selected row
        # matched, so the null slot stays empty (the kernels want two slots)
        keyvals, key_code = list(jattr.values), COL_CODE["i4"]
        nslots = max(len(keyvals), 1) + 1
    exprs = list(getattr(meta, "progs", {}).values())
    entries = [A.Entry(A.COUNT | A.ALL)]
    entry_names: List[Optional[str]] = [None]
    for col, o in ops.items():
        entries.append(A.Entry(o, schema[col].storage if o != A.COUNT else None, col))
        entry_names.append(col)
    names = [n for n in entry_names[1:]]
    if by is not None and by not in names:
        names.append(by)
    if hb is not None:
        for c in [hb.col] if keyspec is None else hb.comps:
            if not isinstance(c, JoinAttr) and c not in names:
                names.append(c)
        return _AggSpec(aggs, hb.col, A.Layout(entries), entry_names, names,
                        {n: schema[n] for n in names}, None, hashed=True,
                        hash_unsigned=keyspec is not None or schema[hb.col].storage[0] == "u",
                        keyspec=keyspec, key_attrs=key_attrs, exprs=exprs)
    return _AggSpec(aggs, by if jattr is None else jattr.name,
                    A.Layout(entries, nslots, key_code), entry_names, names,
                    {n: schema[n] for n in names}, keyvals, join_attr=jattr is not None,
                    exprs=exprs)


@dataclass
class AggOut:
    """Result of ArrowScan.aggregate / host_aggregate (host side, numpy).

    One row per group that selected anything, in slot order (dictionary
    index / False, True / byte value), the null-key group last; without
    ``by`` exactly one row; with ``by=HashBy(col)`` ``keys`` are Python ints
    (ticks for a temporal column) ascending by value, signed or unsigned as
    the column is, the null group last.  ``values[i]`` / ``valid[i]`` belong to
    ``aggs[i]``: sums are int64 / uint64 / float64, min and max have the
    column's storage dtype (ticks for temporal columns: ``columns[i]`` holds
    the type), mean is float64(sum) / count; a group whose column counted
    nothing has an invalid sum, min, max and mean."""
    rows: int
    selected: int
    aggs: List[Tuple[str, Optional[str]]]
    by: Optional[str]
    keys: Optional[list]
    count_all: np.ndarray
    values: List[np.ndarray]
    valid: List[np.ndarray]
    columns: List[Optional[Column]]
    seconds: Dict[str, float]
    bytes_read: int = 0
    column_bytes: int = 0
    groups: int = 0
    _spec: Optional[_AggSpec] = None
    _block: Optional[np.ndarray] = None
    _found: Optional[G.Groups] = None       # by=HashBy: key -> accumulators
    # by=HashBy([...]): per component (values, valid) over the rows of the
    # result — a column's values in its storage dtype (ticks for temporal
    # ones), an attribute's as objects; ``keys`` are then tuples of them with
    # None for a null.  None for every other by=
    key_columns: Optional[List[Tuple[np.ndarray, np.ndarray]]] = None

    @property
    def exprs(self) -> list:
        """The computed columns of the query (ops/colexpr.Program), each
        distinct expression once."""
        return self._spec.exprs if self._spec is not None else []

    def get(self, fn: str, col: Optional[str] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(values, valid) of one requested aggregate (``col``: the name
        or the expression it was asked with)."""
        i = self.aggs.index((fn, name_of(col)))
        return self.values[i], self.valid[i]

    def merge(self, other: "AggOut") -> "AggOut":
        """This result combined with another over the same ``aggs`` and
        ``by`` of the same file (other record batches, another rank):
        counts and sums add, min and max combine."""
        a, b = self._spec, other._spec
        secs = {"total_s": self.seconds.get("total_s", 0.0) + other.seconds.get("total_s", 0.0)}
        if a.hashed or b.hashed:
            # by=HashBy: the union of the keys, whatever groups= each scan had
            if not (a.hashed and b.hashed):
                raise ValueError("merge: a HashBy result merges with HashBy results only")
            if a.aggs != b.aggs or a.by != b.by or a.hash_unsigned != b.hash_unsigned:
                raise ValueError("merge: different aggregates or HashBy column")
            if a.keyspec != b.keyspec or a.key_attrs != b.key_attrs:
                raise ValueError(f"merge: composite keys packed differently ({a.keyspec} and "
                                 f"{b.keyspec}) or other attribute values")
            return _hash_out(a, G.merge(self._found, other._found), self.rows + other.rows, secs,
                             bytes_read=self.bytes_read + other.bytes_read,
                             column_bytes=self.column_bytes + other.column_bytes,
                             groups=self.groups + other.groups)
        if a.aggs != b.aggs or a.by != b.by or a.layout.nslots != b.layout.nslots or \
                a.keyvals != b.keyvals or a.join_attr != b.join_attr:
            raise ValueError("merge: different aggregates, key, dictionary or join attribute")
        return _agg_out(a, A.merge_blocks(a.layout, self._block, other._block),
                        self.rows + other.rows, secs,
                        bytes_read=self.bytes_read + other.bytes_read,
                        column_bytes=self.column_bytes + other.column_bytes,
                        groups=self.groups + other.groups)


def _agg_out(spec: _AggSpec, block: np.ndarray, rows: int, seconds: Dict[str, float],
             bytes_read: int = 0, column_bytes: int = 0, groups: int = 0) -> AggOut:
    lay = spec.layout
    bad = int(block[0])
    if bad:
        raise RuntimeError(f"key column {spec.by}: {bad} selected row(s) with an index outside "
                           f"its dictionary of {lay.nslots - 1} entries")
    count_all = A.entry_arrays(lay, block, 0)["count"]
    if spec.by is None:
        show = np.zeros(1, np.int64)
        keys = None
    else:
        show = np.flatnonzero(count_all > 0)
        if spec.hashed:
            # possibly millions of groups: no Python per key
            nn = show[show < lay.nslots - 1]
            keys = spec.keyvals[nn].tolist() + [None] * (len(show) - len(nn))
        else:
            keys = [spec.keyvals[s] if s < lay.nslots - 1 else None for s in show.tolist()]
    ent = {n: A.entry_arrays(lay, block, e) for e, n in enumerate(spec.entry_names) if e}
    values, valid, columns = [], [], []
    for fn, col in spec.aggs:
        if col is None:
            values.append(count_all[show])
            valid.append(np.ones(len(show), bool))
            columns.append(None)
            continue
        a = ent[col]
        cnt = a["count"][show]
        has = cnt > 0
        if fn == "count":
            v, ok = cnt, np.ones(len(show), bool)
        elif fn == "mean":
            v = np.full(len(show), np.nan)
            np.divide(a["sum"][show].astype(np.float64), cnt, out=v, where=has)
            ok = has
        else:
            v, ok = a[fn][show], has
        values.append(v)
        valid.append(ok)
        columns.append(spec.cols[col])
    return AggOut(rows, int(count_all.sum()), spec.aggs, spec.by, keys, count_all[show], values,
                  valid, columns, seconds, bytes_read, column_bytes, groups, spec, block)


def _hash_out(spec: _AggSpec, found: G.Groups, rows: int, seconds: Dict[str, float],
              **kw) -> AggOut:
    """The AggOut of a by=HashBy result: ``found``'s keys (ascending by
    value) are the slots of a block of its own layout."""
    per = replace(spec, layout=found.layout, keyvals=found.keys)
    out = _agg_out(per, found.block, rows, seconds, **kw)
    out._found = found
    if spec.keyspec is not None:
        # the packed words (ascending: lexicographic) back into components;
        # the null keys' slot is never used on this path.  Possibly millions
        # of groups: numpy per component, Python only for the tuples
        count = A.entry_arrays(found.layout, found.block, 0)["count"][:-1]
        vals, oks = spec.keyspec.unpack(found.keys[count > 0])
        cols, lists = [], []
        for v, ok, attr in zip(vals, oks, spec.key_attrs):
            if attr is not None:
                # a code's value; None is a value of the attribute like any other
                table = np.empty(len(attr) + 1, object)
                table[:len(attr)] = attr
                v = table[np.minimum(v.astype(np.int64), len(attr))]
                ok = np.array([x is not None for x in attr] + [False], bool)[
                    np.minimum(vals[len(cols)].astype(np.int64), len(attr))]
                lists.append(v.tolist())
            elif ok.all():
                lists.append(v.tolist())
            else:
                o = v.astype(object)
                o[~ok] = None
                lists.append(o.tolist())
            cols.append((v, ok))
        # a million tuples: the cyclic collector would walk them again and
        # again while the list grows (half the time of this step)
        paused = gc.isenabled()
        gc.disable()
        try:
            out.keys = list(zip(*lists)) if len(count) else []
        finally:
            if paused:
                gc.enable()
        out.key_columns = cols
    return out


def host_aggregate(path: str, quals, aggs, by=None,
                   batches: Optional[Tuple[int, int]] = None, meta: Optional[ArrowFile] = None,
                   dicts: Optional[dict] = None, join: Union[Join, StarJoin, None] = None) -> AggOut:
    """ArrowScan.aggregate on the CPU: buffers read with pread and decoded
    by the decoders' host twins, the qualifiers by colpred's numpy twin, the
    aggregates by colagg's.  The reference point for the GPU path and the
    same answer on machines without one."""
    t0 = time.perf_counter()
    meta = meta if meta is not None else read_metadata(path)
    dicts = dicts if dicts is not None else {}
    cl = _named_clauses(quals) if quals else []
    battr = by if isinstance(by, JoinAttr) else None
    hb = by if isinstance(by, HashBy) else None
    join = _check_join(meta, join, battr if hb is None else hb.attrs)
    if battr is not None or hb is not None:
        by = None
    aggs, meta = _agg_exprs(meta, cl, aggs, by, hb)
    spec = _agg_spec(meta, aggs, by, lambda name: _dictionary(meta, path, dicts, name), battr, hb)
    found = G.empty_groups(spec.layout.entries, spec.hash_unsigned, spec.keyspec) \
        if hb is not None else None
    misfit = np.zeros(G.MAX_KEYS, np.int64)
    lay = spec.layout
    block = A.new_block(lay)
    nrows = 0
    keys = [by] if hb is None else ([hb.col] if hb.comps is None else hb.comps)
    # a column that is counted only: its validity is enough
    values = lambda n: n in keys or lay.entries[spec.entry_names.index(n)].dtype is not None
    for _, b, data, m, jrow in _host_batches(path, meta, dicts, cl, join, spec.names, batches,
                                             values):
        nrows += b.length
        key = None
        if battr is not None:
            key = (np.where(m, battr.codes[jrow[_leg_of(join, battr)]] if len(battr.codes)
                            else 0, 0).astype(np.int32), None)
        if by is not None:
            kv, kok = data[by]
            kv = np.asarray(kv)
            if kv.dtype == np.int8 and spec.cols[by].dictionary is None:
                kv = kv.view(np.uint8)        # 8-bit key: the slot is the byte
            key = (kv, kok)
        ecols = [(None, None) if name is None else data[name] for name in spec.entry_names]
        if spec.keyspec is not None:
            # the composite path's twin: packed by the same KeySpec
            kcols, koks = [], []
            for c in hb.comps:
                if isinstance(c, JoinAttr):
                    kcols.append(np.where(m, c.codes[jrow[_leg_of(join, c)]] if len(c.codes)
                                          else 0, 0).astype(np.uint32))
                    koks.append(None)
                else:
                    kcols.append(np.asarray(data[c][0]))
                    koks.append(data[c][1])
            part, bad = G.host_group_agg_multi(lay.entries, m, spec.keyspec, kcols, koks, ecols)
            found = G.merge(found, part)
            misfit[:len(bad)] += bad
        elif hb is not None:
            # the hash path's twin: this batch's groups, united by key
            kv, kok = data[hb.col]
            found = G.merge(found, G.host_group_agg(lay.entries, m, kv, kok, ecols))
        else:
            for e, (v, ok) in enumerate(ecols):
                A.host_agg(lay, block, e, m, v, ok, key, count_bad=e == 0)
    if hb is not None:
        _check_groups(hb, len(found.keys))
        if spec.keyspec is not None:
            _check_range(spec.keyspec, misfit[:len(spec.keyspec)])
        return _hash_out(spec, found, nrows, {"total_s": time.perf_counter() - t0})
    return _agg_out(spec, block, nrows, {"total_s": time.perf_counter() - t0})


# ------------------------------------------------------------ ORDER BY ... LIMIT k
@dataclass
class _TopSpec:
    order_by: str
    k: int
    descending: bool
    column: Column                          # the order column
    nullable: bool                          # ... has nulls somewhere in the file
    project: Optional[str] = None           # the carried column's (or attribute's) name
    pcolumn: Optional[Column] = None
    pnullable: bool = False
    pattr: bool = False
    dictionary: object = None
    exprs: list = field(default_factory=list)   # the query's computed columns (Programs)

    def same(self, o: "_TopSpec") -> bool:
        return (self.order_by, self.k, self.descending, self.project, self.pattr) == \
            (o.order_by, o.k, o.descending, o.project, o.pattr) and \
            (not self.pattr or self.dictionary == o.dictionary)


def _file_nulls(meta: ArrowFile, name: str) -> bool:
    """Whether any record batch of the file has nulls in the column — the
    whole file, whatever range is scanned, so that results of ranges merge."""
    ci = meta.column_index(name)
    return bool(meta.nbatches) and bool(np.any(np.asarray(meta.columns[ci].null_count)))


def _top_spec(meta: ArrowFile, order_by: str, k: int, descending: bool, project: Optional[str],
              pattr: Optional[JoinAttr], dictionary) -> _TopSpec:
    """Validate the order and carried columns of ``top`` against the schema."""
    schema = {c.name: c for c in meta.schema}
    if not isinstance(order_by, str):
        raise NotImplementedError("ORDER BY one column (a list of order columns is not supported)")
    if order_by not in schema:
        raise ValueError(f"no column {order_by!r}")
    c = schema[order_by]
    if c.dictionary is not None or c.kind not in ("int", "float") + _TEMPORAL or \
            c.storage not in T.TYPE_CODE:
        kind = "dictionary-encoded" if c.dictionary is not None else c.kind
        raise NotImplementedError(f"ORDER BY {order_by}: {kind} columns are not ordered on the "
                                  "GPU (integer, float32/64, date, time, timestamp and duration "
                                  "columns are)")
    out = _TopSpec(order_by, k, bool(descending), c, _file_nulls(meta, order_by),
                   exprs=list(getattr(meta, "progs", {}).values()))
    if pattr is not None:
        out.project, out.pattr, out.dictionary = pattr.name, True, pattr.values
    elif project is not None:
        if project not in schema:
            raise ValueError(f"no column {project!r}")
        p = schema[project]
        if p.dictionary is None and (p.kind in ("utf8", "binary", "decimal", "bool") or
                                     p.storage not in _TORCH):
            raise NotImplementedError(f"top: projection of {project} ({p.kind}): one fixed-width "
                                      "column of at most 8 bytes or a dictionary-encoded "
                                      "column's indices is carried; the row ids serve the rest")
        out.project, out.pcolumn, out.pnullable = project, p, _file_nulls(meta, project)
        if p.dictionary is not None:
            out.dictionary = dictionary(project)
    return out


@dataclass
class TopOut:
    """Result of ArrowScan.top / host_top (host side, numpy), in result
    order: ``rows`` the int64 file-global row ids, ``values`` the order
    column in its storage dtype (ticks for temporal columns: ``column`` holds
    the type; NaN for a NaN of any payload, 0 for a null), ``valid`` its
    validity when the file has nulls in that column, else None.
    ``projected`` / ``projected_valid``: the carried column (indices for a
    dictionary-encoded one, codes for ``dim[attr]``: ``dictionary`` holds
    their values; 0 for a null) and its validity when the file has nulls in
    it.  ``nrows``: the rows scanned, ``selected``: the rows the qualifiers
    and the join selected."""
    rows: np.ndarray
    values: np.ndarray
    valid: Optional[np.ndarray]
    projected: Optional[np.ndarray]
    projected_valid: Optional[np.ndarray]
    nrows: int
    selected: int
    seconds: Dict[str, float]
    bytes_read: int = 0
    column_bytes: int = 0
    groups: int = 0
    column: Optional[Column] = None
    dictionary: object = None
    _spec: Optional[_TopSpec] = None
    _entries: Optional[np.ndarray] = None   # the candidates (ops/coltopk.py)

    @property
    def exprs(self) -> list:
        """The computed columns of the query (ops/colexpr.Program)."""
        return self._spec.exprs if self._spec is not None else []

    def merge(self, other: "TopOut") -> "TopOut":
        """The ``k`` best of this result and another of the same query over
        other record batches of the same file (another rank), on the host."""
        a, b = self._spec, other._spec
        if not a.same(b):
            raise ValueError("merge: results of another order column, direction, k or carried "
                             "column")
        secs = {"total_s": self.seconds.get("total_s", 0.0) + other.seconds.get("total_s", 0.0)}
        ent = T.best(np.concatenate([self._entries, other._entries]), a.k)
        return _top_out(a, ent, self.nrows + other.nrows, self.selected + other.selected, secs,
                        bytes_read=self.bytes_read + other.bytes_read,
                        column_bytes=self.column_bytes + other.column_bytes,
                        groups=self.groups + other.groups)


def _top_out(spec: _TopSpec, ent: np.ndarray, nrows: int, selected: int,
             seconds: Dict[str, float], **kw) -> TopOut:
    rows, vals, ok, pay, pok = T.decode(ent, spec.column.storage, spec.descending)
    proj = pvalid = None
    if spec.pattr:
        proj = T.payload_as(pay, np.int32)
    elif spec.project is not None:
        proj = T.payload_as(pay, spec.pcolumn.storage)
        pvalid = pok if spec.pnullable else None
    return TopOut(rows, vals, ok if spec.nullable else None, proj, pvalid, nrows, selected,
                  seconds, column=spec.column, dictionary=spec.dictionary, _spec=spec,
                  _entries=ent, **kw)


def host_top(path: str, quals, order_by: str, k: int, descending: bool = False, project=None,
             batches: Optional[Tuple[int, int]] = None, meta: Optional[ArrowFile] = None,
             dicts: Optional[dict] = None, join: Union[Join, StarJoin, None] = None) -> TopOut:
    """ArrowScan.top on the CPU: the host twins' scan, then numpy ``lexsort``
    on (class, key, row) of the candidates (ops/coltopk.py), batch by batch.
    The reference point for the GPU path and the same answer without one."""
    t0 = time.perf_counter()
    meta = meta if meta is not None else read_metadata(path)
    dicts = dicts if dicts is not None else {}
    k = T.check_k(k)
    pattr = project if isinstance(project, JoinAttr) else None
    join = _check_join(meta, join, pattr)
    if pattr is not None:
        project = None
    order_by, project = _order_name(order_by), name_of(project)
    cl = _named_clauses(quals) if quals else []
    meta = _with_exprs(meta, [p.col for c in cl for p in c] + [order_by] +
                       ([project] if project else []))
    spec = _top_spec(meta, order_by, k, descending, project, pattr,
                     lambda name: _dictionary(meta, path, dicts, name))
    base = np.concatenate([[0], np.cumsum(meta.rows)]).astype(np.int64)
    ent = np.zeros((0, T.ENTRY_WORDS), np.uint64)
    nrows = selected = 0
    for bi, b, data, m, jrow in _host_batches(path, meta, dicts, cl, join,
                                              [order_by] + ([project] if project else []),
                                              batches):
        nrows += b.length
        sel = np.flatnonzero(m)
        selected += len(sel)
        v, ok = data[order_by]
        pay = pok = None
        if pattr is not None:
            pay = pattr.codes[jrow[_leg_of(join, pattr)][sel]] if len(pattr.codes) else \
                np.zeros(0, np.int32)
        elif project:
            pv, pk = data[project]
            pay, pok = np.asarray(pv)[sel], (None if pk is None else pk[sel])
        e = T.entries(np.asarray(v)[sel], None if ok is None else ok[sel], sel + base[bi],
                      spec.descending, pay, pok)
        ent = T.best(np.concatenate([ent, e]), k)
    return _top_out(spec, ent, nrows, selected, {"total_s": time.perf_counter() - t0})
