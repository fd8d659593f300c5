"""Files, expressions and references for the computed-column tests
(tests/test_arrow_expr_cpu.py, tests/test_gpu_arrow_expr.py): a table of
every source type an expression takes, some columns with nulls in some
record batches only, a uint64 and a timestamp column for the refusals; a
list of expressions; ``reference`` evaluating one with pyarrow.compute, and
checks of whole queries against pyarrow on the table with the computed column
appended."""
import math

import numpy as np

from nvme_strom_amd.ops.colexpr import E, NAN_BITS
from nvme_strom_amd.ops.colpred import Or, P

CODECS = [None, "lz4", "zstd"]
INT_COLS = ["i8", "i16", "i32", "i64", "u8", "u16", "u32"]
FLT_COLS = ["f32", "f64"]
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
_TABLES = {}


def table(n: int = 3000, batch_rows: int = 700, seed: int = 11):
    """Nulls: i16, u32 and f64 in every other record batch only, i64 in all,
    the others none.  i64 holds its extremes and values past 2^53, f64 zeros of
    both signs, i8 zeros (so ``f64 / i8`` gives inf and NaN)."""
    key = (n, batch_rows, seed)
    if key in _TABLES:
        return _TABLES[key]
    import pyarrow as pa
    rng = np.random.default_rng(seed)
    batch = np.arange(n) // batch_rows
    some = lambda p: (rng.random(n) < p) & (batch % 2 == 1)
    cols = {}
    for name, dt in (("i8", np.int8), ("i16", np.int16), ("i32", np.int32), ("u8", np.uint8),
                     ("u16", np.uint16), ("u32", np.uint32)):
        info = np.iinfo(dt)
        v = rng.integers(info.min, int(info.max) + 1, n).astype(dt)
        v[rng.random(n) < 0.02] = info.min
        v[rng.random(n) < 0.02] = info.max
        cols[name] = v
    cols["i8"][rng.random(n) < 0.1] = 0
    i64 = rng.integers(-10**12, 10**12, n)
    i64[rng.random(n) < 0.05] = I64_MIN
    i64[rng.random(n) < 0.05] = I64_MAX
    big = rng.random(n) < 0.1
    i64[big] = (1 << 53) + rng.integers(1, 1 << 20, int(big.sum())) * 3 + 1
    cols["i64"] = i64
    f32 = rng.normal(0, 10, n).astype(np.float32)
    f64 = rng.normal(0, 1000, n)
    f64[rng.random(n) < 0.08] = 0.0
    f64[rng.random(n) < 0.04] = -0.0
    cols["f32"], cols["f64"] = f32, f64
    arrays = {k: pa.array(v) for k, v in cols.items()}
    arrays["i16"] = pa.array(cols["i16"], mask=some(0.2))
    arrays["u32"] = pa.array(cols["u32"], mask=some(0.1))
    arrays["f64"] = pa.array(cols["f64"], mask=some(0.15))
    arrays["i64"] = pa.array(cols["i64"], mask=rng.random(n) < 0.05)
    # a timestamp in milliseconds as a plain int64 (some 60 distinct seconds),
    # small measures whose products stay exact, a join key
    arrays["ts_ms"] = pa.array(1_700_000_000_000 + rng.integers(0, 60_000, n))
    arrays["qty"] = pa.array(rng.integers(1, 50, n).astype(np.int32))
    arrays["price"] = pa.array(np.round(rng.uniform(1, 500, n), 2))
    arrays["disc"] = pa.array(rng.integers(0, 11, n).astype(np.float32) / np.float32(100))
    arrays["fk"] = pa.array(rng.integers(0, 40, n).astype(np.int32))
    arrays["u64"] = pa.array(rng.integers(0, 1 << 62, n).astype(np.uint64))
    arrays["ts"] = pa.array(1_700_000_000_000_000 + rng.integers(0, 10**9, n),
                            type=pa.timestamp("us"))
    arrays["b"] = pa.array(rng.random(n) < 0.5)
    arrays["s"] = pa.array([f"s{k % 7}" for k in range(n)])
    arrays["dict"] = pa.array([f"d{k % 5}" for k in range(n)]).dictionary_encode()
    arrays["dec"] = pa.array(rng.integers(-10**6, 10**6, n)).cast(pa.decimal128(23, 4))
    _TABLES[key] = pa.table(arrays)
    return _TABLES[key]


def exprs():
    """(label, expression, "int" / "float")."""
    return [
        ("mul add", E("i32") * E("i16") + E("i8"), "int"),
        ("wrap", E("i64") * 3 - E("u32"), "int"),
        ("neg abs", -E("i64") + abs(E("i64") - 1) - E("u16"), "int"),
        ("second", E("ts_ms") // 1000, "int"),
        ("div mod", (E("i64") // (1 << 40)) % 7 + E("i8") % 3, "int"),
        ("unsigned", E("u8") + E("u16") * E("u32") - 5, "int"),
        ("consts", 7 - (2 * E("i32") + 1) * -3, "int"),
        ("q1", E("price") * (1 - E("disc")), "float"),
        ("ratio", E("f64") / E("i8"), "float"),
        ("big", E("i64") + 0.5, "float"),
        ("mixed", 2 * E("f32") - abs(E("f64")) / 4 + E("u32"), "float"),
        ("int div", E("i32") / E("i16"), "float"),
    ]


def is_float(tbl, e: E) -> bool:
    """The domain rule, written again: a float source, a float constant or /."""
    def walk(k) -> bool:
        if k[0] == "col":
            import pyarrow as pa
            return pa.types.is_floating(tbl.schema.field(k[1]).type)
        if k[0] == "const":
            return isinstance(k[1], float)
        return k[0] == "/" or any(isinstance(x, tuple) and walk(x) for x in k[1:])
    return walk(e.key())


def reference(tbl, e: E):
    """``e`` over ``tbl`` with pyarrow.compute, op by op (``//`` and ``%``
    with numpy's floor_divide / remainder, the null mask carried): a
    pyarrow int64 or float64 array."""
    import pyarrow as pa
    import pyarrow.compute as pc
    flt = is_float(tbl, e)
    ty = pa.float64() if flt else pa.int64()

    def ev(k):
        if k[0] == "col":
            return pc.cast(tbl.column(k[1]).combine_chunks(), ty, safe=False)
        if k[0] == "const":
            return pa.scalar(float(k[1]) if flt else int(k[1]), ty)
        if k[0] == "neg":
            return pc.negate(ev(k[1]))
        if k[0] == "abs":
            return pc.abs(ev(k[1]))
        if k[0] in ("//", "%"):
            a = ev(k[1])
            v = a.fill_null(0).to_numpy(zero_copy_only=False)
            with np.errstate(all="ignore"):
                r = (np.floor_divide if k[0] == "//" else np.remainder)(v, np.int64(k[2]))
            return pa.array(r, mask=~np.asarray(a.is_valid()))
        f = {"+": pc.add, "-": pc.subtract, "*": pc.multiply, "/": pc.divide}[k[0]]
        return f(ev(k[1]), ev(k[2]))
    return ev(e.key())


def bits(values) -> np.ndarray:
    """The values' 64 bits, every NaN as the one the kernel stores."""
    v = np.ascontiguousarray(values)
    if v.dtype.kind == "f":
        v = v.astype(np.float64)
        out = v.view(np.uint64).copy()
        out[np.isnan(v)] = np.uint64(NAN_BITS)
        return out
    return v.astype(np.int64).view(np.uint64)


def ref_numpy(tbl, e: E):
    """(bits of the reference's values with 0 at nulls, validity)."""
    r = reference(tbl, e)
    ok = np.asarray(r.is_valid())
    v = bits(r.fill_null(0).to_numpy(zero_copy_only=False))
    v[~ok] = 0
    return v, ok


def np_of(x) -> np.ndarray:
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def with_column(tbl, name: str, e: E):
    return tbl.append_column(name, reference(tbl, e))


def mask_of(tbl, pred) -> np.ndarray:
    """A pyarrow boolean expression result as a numpy mask (null: False)."""
    m = pred.combine_chunks() if hasattr(pred, "combine_chunks") else pred
    return np.asarray(m.fill_null(False))


def float_sum_close(got: float, values: np.ndarray) -> bool:
    """|got - fsum| <= n 2^-52 sum|x| (the project's float-sum rule)."""
    if not len(values):
        return True
    if not np.isfinite(values).all():
        want = float(np.sum(values))
        return (math.isnan(got) and math.isnan(want)) or got == want
    return abs(got - math.fsum(values)) <= len(values) * 2.0 ** -52 * math.fsum(np.abs(values))


def check_agg(out, fn: str, e, ref, m: np.ndarray, where="") -> None:
    """One unkeyed aggregate of the expression ``e`` (reference array ``ref``)
    over the rows ``m`` against pyarrow."""
    import pyarrow as pa
    import pyarrow.compute as pc
    sel = ref.filter(pa.array(m))
    v, ok = out.get(fn, e)
    n = len(sel) - sel.null_count
    flt = pa.types.is_floating(ref.type)
    if fn == "count":
        assert int(v[0]) == n, (where, fn)
        return
    assert bool(ok[0]) == (n > 0), (where, fn)
    if not n:
        return
    x = sel.drop_null().to_numpy(zero_copy_only=False)
    if fn in ("min", "max"):
        r = pc.min_max(sel)[fn].as_py()
        if flt and np.isnan(x).all():
            return
        assert v[0] == r, (where, fn, v[0], r)
    elif fn == "sum":
        if flt:
            assert float_sum_close(float(v[0]), x), (where, fn, v[0])
        else:
            with np.errstate(all="ignore"):
                assert int(v[0]) == int(np.sum(x, dtype=np.int64)), (where, fn)
    elif flt and np.isfinite(x).all():
        # float64(sum) / count: the sum's bound over the count
        assert abs(v[0] - math.fsum(x) / n) <= 2.0 ** -52 * math.fsum(np.abs(x)) * (1 + 1e-9), \
            (where, fn, v[0])
    else:
        with np.errstate(all="ignore"):
            want = float(np.float64(np.sum(x, dtype=np.float64 if flt else np.int64)) / n)
        assert v[0] == want or (math.isnan(v[0]) and math.isnan(want)), (where, fn, v[0], want)


def check_grouped(out, tbl, key_names, e, ref, m: np.ndarray, fns=("count", "sum", "min", "max"),
                  where="") -> None:
    """A keyed result against pyarrow's group_by on the table with the
    computed column appended: the same groups, and per group every aggregate
    of ``e``."""
    import pyarrow as pa
    flt = pa.types.is_floating(ref.type)
    t = tbl.append_column("__x", ref).filter(pa.array(m))
    got_keys = [k if isinstance(k, tuple) else (k,) for k in out.keys]
    keys = np.empty(t.num_rows, object)
    cols = [t.column(k).to_pylist() for k in key_names]
    keys[:] = list(zip(*cols)) if cols else []
    xs = t.column("__x").to_numpy(zero_copy_only=False)
    okx = np.asarray(t.column("__x").combine_chunks().is_valid())
    groups = {}
    for i, k in enumerate(keys.tolist()):
        groups.setdefault(k, []).append(i)
    assert sorted(got_keys, key=repr) == sorted(groups, key=repr), where
    for gi, k in enumerate(got_keys):
        idx = np.asarray(groups[k])
        assert int(out.count_all[gi]) == len(idx), (where, k)
        x = xs[idx][okx[idx]]
        for fn in fns:
            v, ok = out.get(fn, e)
            if fn == "count":
                assert int(v[gi]) == len(x), (where, k)
                continue
            assert bool(ok[gi]) == (len(x) > 0), (where, k, fn)
            if not len(x):
                continue
            if fn == "sum" and flt:
                assert float_sum_close(float(v[gi]), x), (where, k, v[gi])
            elif fn == "sum":
                with np.errstate(all="ignore"):
                    assert int(v[gi]) == int(np.sum(x.astype(np.int64), dtype=np.int64)), (where, k)
            else:
                y = x[~np.isnan(x)] if flt else x
                if len(y):
                    assert v[gi] == (y.min() if fn == "min" else y.max()), (where, k, fn)


def top_reference(ref, m: np.ndarray, descending: bool, k: int) -> np.ndarray:
    """pc.sort_indices of the computed column over the selected rows (ties
    by row id), cut to k: the file-global row ids."""
    import pyarrow as pa
    import pyarrow.compute as pc
    ids = np.flatnonzero(m).astype(np.int64)
    t = pa.table({"v": ref.take(pa.array(ids)), "row": pa.array(ids)})
    order = pc.sort_indices(t, sort_keys=[("v", "descending" if descending else "ascending"),
                                          ("row", "ascending")])
    return ids[np.asarray(order)[:k]]


def join_dim():
    """(keys, attribute values) of the dimension ``fk`` joins."""
    keys = np.arange(0, 40, 3, dtype=np.int64)
    return keys, [f"g{int(k) % 4}" for k in keys]


# ------------------------------------------------------------ the kernel alone
ROWS = [1, 63, 64, 65, 127, 200]
PREFILL = 0xA5A5A5A5A5A5A5A5
GUARD = 16            # words in front of and behind each output buffer


class Case:
    """Hand-built record batches for one launch: per source column a flat
    value buffer (each batch 8-byte aligned) and, where ``has[c][b]``, the
    batch's validity words; the outputs are prefilled and guarded.  Bits past
    a batch's rows are set in the validity words: the kernel has to cut them."""

    def __init__(self, rows, vals, valid=None, has=None):
        self.rows = np.asarray(rows, np.int64)
        nb, nc = len(self.rows), len(vals)
        self.words = (self.rows + 63) // 64
        self.word_base = np.concatenate([[0], np.cumsum(self.words)[:-1]]).astype(np.int64)
        self.nwords = int(self.words.sum())
        pad = (self.rows + 7) // 8 * 8
        self.elem = np.concatenate([[0], np.cumsum(pad)[:-1]]).astype(np.int64)
        self.vals = []
        for v in vals:                     # v: per batch arrays of one dtype
            flat = np.zeros(int(pad.sum()), v[0].dtype)
            for b in range(nb):
                flat[self.elem[b]:self.elem[b] + self.rows[b]] = v[b]
            self.vals.append(flat)
        self.batch_vals = vals
        self.valid = valid if valid is not None else [None] * nc     # per column: per batch bools
        self.has = has if has is not None else [[valid is not None and self.valid[c] is not None] * nb
                                                for c in range(nc)]
        self.vwords = []
        for c in range(nc):
            w = np.full(self.nwords, 0xFFFFFFFFFFFFFFFF, np.uint64)
            if self.valid[c] is not None:
                for b in range(nb):
                    if not self.has[c][b]:
                        continue
                    ok = np.ones(int(self.words[b]) * 64, bool)
                    ok[:self.rows[b]] = self.valid[c][b]
                    w[self.word_base[b]:self.word_base[b] + self.words[b]] = \
                        np.packbits(ok, bitorder="little").view(np.uint64)
            self.vwords.append(w)

    def out_buffers(self):
        """(values, validity): nwords * 64 + guards / nwords + guards words."""
        return (np.full(self.nwords * 64 + 2 * GUARD, PREFILL, np.uint64),
                np.full(self.nwords + 2 * GUARD, PREFILL, np.uint64))

    def tables(self, val_ptrs, valid_ptrs, out_ptr: int, outv_ptr: int):
        """(src (ncols, nb, 5), out (nb, 5)) int64 over buffers at those addresses."""
        nb = len(self.rows)
        src = np.zeros((len(self.vals), nb, 5), np.int64)
        for c, flat in enumerate(self.vals):
            src[c, :, 0] = val_ptrs[c] + self.elem * flat.dtype.itemsize
            src[c, :, 1] = np.where(self.has[c], valid_ptrs[c] + self.word_base * 8, 0)
            src[c, :, 2], src[c, :, 3] = self.rows, self.word_base
        out = np.zeros((nb, 5), np.int64)
        out[:, 0] = out_ptr + (GUARD + self.word_base * 64) * 8
        out[:, 1] = outv_ptr + (GUARD + self.word_base) * 8
        out[:, 2], out[:, 3] = self.rows, self.word_base
        return src, out

    def expected(self, prog, host_expr, sel=None):
        """The output buffers as the twin leaves them."""
        vals, valid = self.out_buffers()
        for b in range(len(self.rows)):
            n = int(self.rows[b])
            v, ok = host_expr(prog, [x[b] for x in self.batch_vals],
                              [self.valid[c][b] if self.has[c][b] else None
                               for c in range(len(self.vals))], n)
            ok = np.ones(n, bool) if ok is None else ok
            full = np.zeros(int(self.words[b]) * 64, bool)
            full[:n] = ok
            w = np.packbits(full, bitorder="little").view(np.uint64).copy()
            o = GUARD + int(self.word_base[b]) * 64
            for k in range(int(self.words[b])):
                if sel is not None and sel[self.word_base[b] + k] == 0:
                    w[k] = 0
                    full[k * 64:(k + 1) * 64] = False
            valid[GUARD + self.word_base[b]:GUARD + self.word_base[b] + self.words[b]] = w
            idx = np.flatnonzero(full[:n])
            vals[o + idx] = bits(v)[idx]
        return vals, valid


def source_values(dtype: str, n: int, rng) -> np.ndarray:
    """Random values of a source type with its extremes and specials."""
    dt = np.dtype(dtype)
    if dt.kind == "f":
        v = rng.normal(0, 100, n).astype(dt)
        sp = [np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324 if dt.itemsize == 8 else 1e-45, 1e30]
    else:
        info = np.iinfo(dt)
        v = rng.integers(info.min, int(info.max) + 1, n, dtype=dt)
        sp = [info.min, info.max, 0, 1]
    k = rng.random(n) < 0.15
    v[k] = np.asarray(sp, dt)[rng.integers(0, len(sp), int(k.sum()))]
    return v


def case_of(dtypes, rows=ROWS, nulls="none", seed=0) -> Case:
    """``nulls``: "none", "one" (validity on the first source only), "some"
    (every source, on every other batch)."""
    rng = np.random.default_rng(seed)
    vals = [[source_values(dt, int(n), rng) for n in rows] for dt in dtypes]
    if nulls == "none":
        return Case(rows, vals)
    valid = [[rng.random(int(n)) < 0.7 for n in rows] for _ in dtypes]
    if nulls == "one":
        has = [[c == 0] * len(rows) for c in range(len(dtypes))]
    else:
        has = [[(b + c) % 2 == 0 for b in range(len(rows))] for c in range(len(dtypes))]
    return Case(rows, vals, valid, has)


def selections(nwords: int, seed: int = 0):
    """(label, selection words or None): absent, all ones, sparse, with zero words."""
    rng = np.random.default_rng(seed)
    r = lambda: rng.integers(0, 1 << 63, nwords, dtype=np.uint64) * np.uint64(2) + \
        rng.integers(0, 2, nwords, dtype=np.uint64)
    zeros = r() | np.uint64(1)
    zeros[::2] = 0
    return [("none", None), ("ones", np.full(nwords, 0xFFFFFFFFFFFFFFFF, np.uint64)),
            ("sparse", (r() & r() & r()) | np.uint64(1 << 17)), ("zero words", zeros)]


__all__ = ["E", "P", "Or"]
