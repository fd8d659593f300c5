"""Join tables and dimension tables shared by the CPU test of the coljoin
twin and the GPU test of the kernels (tests/test_arrow_join_cpu.py,
tests/test_gpu_arrow_join.py), and the pyarrow references of joined scans."""
from __future__ import annotations

import numpy as np

from nvme_strom_amd.ops import coljoin as J

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
SPECIAL = [0, -1, I64_MIN, I64_MAX]          # I64_MIN is the table's "empty" pattern


def keys_with_home(home: int, cap: int, count: int, start: int = 1) -> np.ndarray:
    """``count`` distinct keys whose home slot in a ``cap``-slot table is
    ``home``, found by search with the twin's hash."""
    out = []
    lo = start
    while len(out) < count:
        c = np.arange(lo, lo + (1 << 16), dtype=np.int64)
        out += c[(J.hash64(c) & np.uint64(cap - 1)) == np.uint64(home)].tolist()
        lo += 1 << 16
    return np.array(out[:count], np.int64)


def key_sets():
    """(label, keys): tables of 0, 1, 2, 37 and 5,000 keys with 0, -1,
    INT64_MIN (the empty pattern) and INT64_MAX among them; 200 keys on one
    home slot of a 512-slot table; keys whose home is the last slot."""
    rng = np.random.default_rng(41)
    rnd = lambda n: np.unique(rng.integers(-10**15, 10**15, 2 * n))[:n]
    sets = [("0", np.zeros(0, np.int64)), ("1", np.array([I64_MIN])), ("2", np.array([-1, 7])),
            ("37", np.concatenate([SPECIAL, rnd(33)])),
            ("5000", rng.permutation(np.concatenate([SPECIAL, rnd(4996)]))),
            ("chain", keys_with_home(300, 512, 200)),
            ("wrap", np.concatenate([keys_with_home(63, 64, 9), keys_with_home(62, 64, 3, 10**7)]))]
    for label, k in sets:
        assert len(np.unique(k)) == len(k), label
    return [(label, np.asarray(k, np.int64)) for label, k in sets]


def probe_values(keys: np.ndarray, n: int, seed: int = 0) -> np.ndarray:
    """``n`` int64 values: about half of them keys, the rest absent ones and
    the special values."""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([rng.integers(-10**15, 10**15, 64), np.array(SPECIAL, np.int64),
                           keys_with_home(300, 512, 8, 10**8)])
    v = rng.choice(pool, n)
    if len(keys):
        hit = rng.random(n) < 0.5
        v[hit] = rng.choice(keys, int(hit.sum()))
    return v


def dimension(col, seed: int = 3):
    """(keys int64, category strings with some None, region ints) for a fact
    column (pyarrow array): half of its distinct values plus as many absent
    keys, shuffled."""
    rng = np.random.default_rng(seed)
    vals = np.unique(np.asarray(col.drop_null()).astype(np.int64))
    have = rng.choice(vals, len(vals) // 2, replace=False)
    absent = np.setdiff1d(rng.integers(-2 * 10**12, 2 * 10**12, 2 * len(have)), vals)[:len(have)]
    keys = rng.permutation(np.concatenate([have, absent]))
    words = ["ash", "birch", "cedar", None, "elm", "fir", ""]
    cats = [words[i] for i in rng.integers(0, len(words), len(keys))]
    regs = rng.integers(-3, 4, len(keys)).astype(np.int64)
    return keys, cats, regs


def joined(tbl, fk: str, keys, attrs: dict, how: str):
    """pyarrow's answer: ``tbl`` (dictionary columns dropped) with a row-id
    column ``__id`` joined with the dimension on ``fk``."""
    import pyarrow as pa
    keep = [n for n in tbl.column_names if not pa.types.is_dictionary(tbl.schema.field(n).type)
            and not pa.types.is_decimal(tbl.schema.field(n).type)]
    left = tbl.select(keep).append_column("__id", pa.array(np.arange(tbl.num_rows, dtype=np.int64)))
    left = left.set_column(left.column_names.index(fk), fk, left.column(fk).cast(pa.int64()))
    dim = pa.table({"__k": pa.array(np.asarray(keys, np.int64)),
                    **{n: pa.array(v) for n, v in attrs.items()}})
    return left.join(dim, keys=fk, right_keys="__k", join_type=how, use_threads=False)


def joined_ids(tbl, fk, keys, how, mask_fn=None) -> np.ndarray:
    j = joined(tbl, fk, keys, {}, "left " + how)
    if mask_fn is not None:
        m = mask_fn(j)
        m = m.combine_chunks() if hasattr(m, "combine_chunks") else m
        j = j.filter(m.fill_null(False))
    return np.sort(np.asarray(j.column("__id").combine_chunks()))
