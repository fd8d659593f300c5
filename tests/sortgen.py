"""Seeded key generators and the case lists of the ORDER BY tests
(tests/test_arrow_sort_cpu.py, tests/test_gpu_arrow_sort.py): the key shapes
the radix passes can go wrong on, multi-column keys with heavy ties, and the
table, qualifiers and order lists of the whole-scan tests."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

import projgen as G  # noqa: F401  (the whole-scan table and its helpers)
from nvme_strom_amd.ops import colsort as SO

TILE = SO.TILE
SIZES = (0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17)
INTS = ("i1", "i2", "i4", "i8", "u1", "u2", "u4", "u8")
FLOATS = ("f4", "f8")
STORAGE = INTS + FLOATS


def _nan(dt: str, payload: int, neg: bool = False) -> float:
    """A NaN of ``dt`` with ``payload`` in its mantissa."""
    if dt == "f4":
        bits = np.array([0x7FC00000 | (payload & 0x3FFFFF) | (0x80000000 if neg else 0)], "<u4")
        return bits.view("<f4")[0]
    bits = np.array([0x7FF8000000000000 | payload | ((1 << 63) if neg else 0)], "<u8")
    return bits.view("<f8")[0]


def special_floats(dt: str) -> np.ndarray:
    tiny = np.finfo(dt).smallest_subnormal
    return np.array([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, 3 * tiny, np.finfo(dt).tiny, 1.0,
                     -1.0, np.finfo(dt).max, np.finfo(dt).min, _nan(dt, 0), _nan(dt, 1),
                     _nan(dt, 0x1234, True)], dt)


def random_keys(dt: str, n: int, rng) -> np.ndarray:
    if dt in FLOATS:
        v = rng.normal(0, 1e3, n).astype(dt)
        sp = special_floats(dt)
        at = rng.random(n) < 0.2
        v[at] = sp[rng.integers(0, len(sp), int(at.sum()))]
        return v
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)


def nulls(n: int, share: float, rng) -> Optional[np.ndarray]:
    """A validity array (bool) with ``share`` of nulls; None for none."""
    if share == 0:
        return None
    return np.zeros(n, bool) if share >= 1 else rng.random(n) >= share


def key_cases(n: int, seed: int = 11) -> List[Tuple[str, np.ndarray, Optional[np.ndarray]]]:
    """(label, values, valid) of every key shape at n rows; each is sorted in
    both directions."""
    rng = np.random.default_rng(seed + n)
    pick = lambda vals, dt: np.array(vals, dt)[rng.integers(0, len(vals), n)]
    out = [("equal", np.full(n, 7, "i8"), None),
           ("alternate", np.where(np.arange(n) % 2 == 0, 5, -5).astype("i4"), None),
           ("ascending", np.arange(n, dtype="i8") - n // 2, None),
           ("descending", (n - np.arange(n, dtype="i8")) * 3, None),
           ("255/256", pick([255, 256, 254, 257], "u2"), None),
           ("65535/65536", pick([65535, 65536, 65534, 65537], "u4"), None),
           ("i64 extremes", pick([-2**63, 2**63 - 1, -1, 0, 1, -2**63 + 1], "i8"), None),
           ("u64 high", pick([2**63 - 1, 2**63, 2**64 - 1, 0, 2**63 + 1], "u8"), None),
           ("mostly one", np.where(rng.random(n) < 0.99, 42, rng.integers(-2**31, 2**31, n))
            .astype("i4"), None)]
    for b in range(8):
        # values that differ in byte b alone
        v = (rng.integers(0, 256, n).astype("u8") << np.uint64(8 * b)) | np.uint64(0x0101010101010101
                                                                                   & ~(0xFF << 8 * b))
        out.append((f"byte {b}", v, None))
        out.append((f"byte {b} signed", v.view("i8"), None))
    for dt in FLOATS:
        sp = special_floats(dt)
        out.append((f"{dt} specials", sp[rng.integers(0, len(sp), n)], None))
    for dt in STORAGE:
        out.append((f"{dt} random", random_keys(dt, n, rng), None))
    for share in (0.1, 1.0):
        for dt in ("i2", "f4", "u8", "f8"):
            out.append((f"{dt} nulls {share}", random_keys(dt, n, rng), nulls(n, share, rng)))
    return out


def tied_columns(nkeys: int, n: int, seed: int = 23) -> List[tuple]:
    """``nkeys`` order columns of 8-bit cardinality — (values, valid,
    descending) each, the most significant first — of every flavour: nulls,
    NaNs, both directions, several storage types."""
    rng = np.random.default_rng(seed + nkeys)
    f = np.array([0.0, -0.0, 1.5, -1.5, np.nan, np.inf], "f4")
    pool = [(rng.integers(0, 6, n).astype("i1"), nulls(n, 0.1, rng), True),
            (f[rng.integers(0, len(f), n)], nulls(n, 0.1, rng), False),
            (rng.integers(120, 136, n).astype("u8") << np.uint64(56), None, True),
            (rng.integers(-4, 4, n).astype("i2"), None, False)]
    return pool[:nkeys]


def sort_keys_of(names: Sequence[str], columns: Sequence[tuple]) -> list:
    """pyarrow's sort_keys of ``columns``."""
    return [(nm, "descending" if c[2] else "ascending") for nm, c in zip(names, columns)]


def arrow_table(names: Sequence[str], columns: Sequence[tuple]):
    import pyarrow as pa
    return pa.table({nm: pa.array(v, mask=None if ok is None else ~ok)
                     for nm, (v, ok, _) in zip(names, columns)})


# ---------------------------------------------------------------- whole scans
# (select list, order_by): every projected kind, order columns of several
# kinds and both directions, inside and outside the list
ORDERS = [(["i8", "s", "f64n", "dec", "b"], [("i8", "descending"), "f64n"]),
          (["dict", "ls", "u64", "idict", "lbin"], [("u8", "ascending"), ("f32", "descending"),
                                                    "i16"]),
          (["ts", "bin", "d32"], [("d32", "descending"), ("ts", "ascending"), "t32", "dur"]),
          (["s"], "u64")]
WINDOWS = [(None, 0), (10, 0), (25, 7), (None, 100), (5, 10**7), (0, 3)]


def pa_sort_keys(order_by) -> list:
    items = order_by if isinstance(order_by, list) else [order_by]
    return [(it, "ascending") if isinstance(it, str) else it for it in items]


def cut(tbl, limit, offset):
    """LIMIT / OFFSET of a pyarrow table."""
    off = min(offset, tbl.num_rows)
    return tbl.slice(off) if limit is None else tbl.slice(off, limit)
