"""The fact table, the dimensions and the pyarrow references of the star-join
tests (tests/test_arrow_star_cpu.py, tests/test_gpu_arrow_star.py), and the
hand-built batches the probe kernel and its twin are compared on."""
from __future__ import annotations

import numpy as np

from joingen import dimension, key_sets, probe_values

ROWS = 6000
FKS = ("f64", "f32", "f16", "f8")        # int64 with nulls, uint32, int16 with nulls, uint8
AGGS = [("count", None), ("sum", "m64"), ("min", "m32"), ("max", "m32"), ("count", "m32")]
# the storage types of J.FK_CODE
DTYPES = ("i8", "i4", "i2", "i1", "u8", "u4", "u2", "u1")


def table(n: int = ROWS, seed: int = 11):
    """Four fk columns (int64 and int16 with nulls, uint32, uint8), two
    measures (int64; int32 with nulls) and an int16 key column."""
    import pyarrow as pa
    rng = np.random.default_rng(seed)
    nulls = lambda p: rng.random(n) < p
    return pa.table({
        "f64": pa.array(rng.integers(-400, 400, n).astype(np.int64) * 10**9, mask=nulls(0.05)),
        "f32": pa.array(rng.integers(0, 300, n).astype(np.uint32) * 7919),
        "f16": pa.array(rng.integers(-200, 200, n).astype(np.int16), mask=nulls(0.1)),
        "f8": pa.array(rng.integers(0, 256, n).astype(np.uint8)),
        "m64": pa.array(rng.integers(-10**12, 10**12, n).astype(np.int64)),
        "m32": pa.array(rng.integers(-10**6, 10**6, n).astype(np.int32), mask=nulls(0.07)),
        "k16": pa.array(rng.integers(-3, 4, n).astype(np.int16)),
        "x": pa.array(rng.random(n)),
    })


def dimensions(tbl) -> dict:
    """Per fk column (keys, {attribute: values}) from joingen.dimension.  The
    attribute ``cat`` exists in the dimensions of f64 and f16 (the names
    collide), ``reg`` in those of f64 and f32, ``kind`` in f8's."""
    out = {}
    for i, fk in enumerate(FKS):
        keys, cats, regs = dimension(tbl.column(fk).combine_chunks(), seed=3 + i)
        attrs = {"f64": {"cat": cats, "reg": regs.tolist()}, "f32": {"reg": regs.tolist()},
                 "f16": {"cat": cats}, "f8": {"kind": cats}}[fk]
        out[fk] = (keys, attrs)
    return out


def reference(tbl, dims: dict, legs, attrs=()):
    """pyarrow's answer, Table.join chained leg by leg.  ``legs``: (fk, how)
    with how "semi" / "anti"; ``attrs``: (fk, attribute, column name in the
    result) brought along by an inner join on that (semi) leg.  Returns the
    table of the rows left with their row id ``__id``, sorted by it."""
    import pyarrow as pa
    left = tbl.append_column("__id", pa.array(np.arange(tbl.num_rows, dtype=np.int64)))
    for fk in FKS:
        left = left.set_column(left.column_names.index(fk), fk, left.column(fk).cast(pa.int64()))
    for fk, how in legs:
        keys, vals = dims[fk]
        mine = [(a, out) for f, a, out in attrs if f == fk]
        cols = {"__k": pa.array(np.asarray(keys, np.int64))}
        for a, out in mine:
            cols[out] = pa.array(vals[a])
        kind = "inner" if mine else "left " + how
        assert not (mine and how == "anti")
        left = left.join(pa.table(cols), keys=fk, right_keys="__k", join_type=kind,
                         use_threads=False)
    return left.sort_by("__id")


def ids(ref) -> np.ndarray:
    return np.asarray(ref.column("__id").combine_chunks())


def check_agg(out, ref, keys=None):
    """An AggOut over AGGS against pyarrow's group_by of the reference table:
    ``keys`` the reference's key columns (None: one group)."""
    import pyarrow as pa
    t = ref if keys else ref.append_column("__one", pa.array(np.zeros(ref.num_rows, np.int8)))
    by = list(keys) if keys else ["__one"]
    g = t.group_by(by, use_threads=False).aggregate(
        [([], "count_all"), ("m64", "sum"), ("m32", "min"), ("m32", "max"), ("m32", "count")])
    g = g.to_pydict()
    want = {}
    for i in range(len(g["count_all"])):
        k = tuple(g[b][i] for b in by)
        want[k if len(by) > 1 else k[0]] = (g["count_all"][i], g["m64_sum"][i], g["m32_min"][i],
                                            g["m32_max"][i], g["m32_count"][i])
    if not keys:
        if not ref.num_rows:
            assert out.selected == 0
            return
        want = {None: want[0]}
        got_keys = [None]
    else:
        got_keys = out.keys
    assert out.selected == ref.num_rows
    assert len(got_keys) == len(want) and set(got_keys) == set(want), (got_keys, list(want))
    for gi, k in enumerate(got_keys):
        w = want[k]
        assert int(out.count_all[gi]) == w[0], k
        assert int(out.values[0][gi]) == w[0] and int(out.values[1][gi]) == w[1], k
        assert int(out.values[4][gi]) == w[4], k
        for i, x in ((2, w[2]), (3, w[3])):
            assert bool(out.valid[i][gi]) == (x is not None), k
            if x is not None:
                assert int(out.values[i][gi]) == x, k


def check_top(out, ref, order_by: str, k: int, descending: bool, pcol=None):
    """A TopOut against pyarrow's sort of the reference table."""
    import pyarrow.compute as pc
    order = "descending" if descending else "ascending"
    idx = pc.sort_indices(ref, sort_keys=[(order_by, order), ("__id", "ascending")])
    best = ref.take(idx[:k])
    assert out.selected == ref.num_rows
    assert np.array_equal(out.rows, ids(best))
    if pcol is not None:
        assert [out.dictionary[c] for c in out.projected.tolist()] == best.column(pcol).to_pylist()


# ------------------------------------------------------------ kernel cases
BATCH_ROWS = (1, 63, 64, 65, 200)
PREFILL = -77


def star_case(nlegs: int, seed: int, tables=None, hows=None, kouts=None, source: str = "dense",
              valid_on=None, type0: int = 0):
    """One hand-built launch: batches of BATCH_ROWS rows, ``nlegs`` legs whose
    storage types cycle through DTYPES from ``type0``, whose tables are
    ``tables`` (labels of joingen.key_sets()).  ``valid_on``: the (leg, batch)
    pairs with a validity bitmap (default: some legs and batches only).
    ``source``: "dense", "alternate" (every other word zero) or "single" (one
    bit per word), always with garbage beyond each batch's rows.  Returns a dict:
    keys (per leg the table's keys), fks (per leg and batch (values, valid)),
    hows, kouts, src."""
    rng = np.random.default_rng(seed)
    sets = dict(key_sets())
    labels = list(sets)
    tables = tables or [labels[(seed + i) % len(labels)] for i in range(nlegs)]
    hows = hows or ["semi" if (seed >> i) & 1 == 0 else "anti" for i in range(nlegs)]
    if kouts is None:
        kouts, j = [], 0
        for h in hows:
            kouts.append(j if h == "semi" else -1)
            j += h == "semi"
    keys, fks = [], []
    for i in range(nlegs):
        dt = np.dtype(DTYPES[(type0 + i) % len(DTYPES)])
        k = sets[tables[i]]
        # keys the leg's storage type can hold, so that narrow types match too
        info = np.iinfo(dt)
        fit = k[(k >= info.min) & (k <= min(info.max, 2**63 - 1))]
        if dt.itemsize <= 2:
            # a narrow column: a table of keys in its range (plus the label's own)
            lo, hi = max(info.min, -100), min(info.max, 100)
            k = np.unique(np.concatenate([fit, rng.integers(lo, hi, max(len(k), 1) // 2 + 1)
                                          if len(k) else np.zeros(0, np.int64)])).astype(np.int64)
        keys.append(np.asarray(k, np.int64))
        per = []
        for b, n in enumerate(BATCH_ROWS):
            v = probe_values(keys[i], n, seed=seed * 131 + i * 17 + b)
            if dt.itemsize <= 2:
                lo, hi = max(info.min, -100), min(info.max, 100)
                v = rng.integers(lo, hi, n)
            elif dt == np.uint64:
                v = v.astype(np.uint64)
                v[rng.random(n) < 0.1] = np.uint64(2**63 + 5)        # matches nothing
            elif dt.itemsize == 4:
                inr = (v >= info.min) & (v <= info.max)
                v = np.where(inr, v, rng.integers(0, 1000, n))
            has = (i, b) in valid_on if valid_on is not None else (i + b + seed) % 3 == 0
            per.append((v.astype(dt), (rng.random(n) < 0.8) if has else None))
        fks.append(per)
    words = []
    for n in BATCH_ROWS:
        nw = (n + 63) // 64
        bits = np.ones(nw * 64, np.uint8)                            # garbage beyond the rows
        if source == "dense":
            bits[:n] = rng.random(n) < 0.9
        elif source == "alternate":
            bits[:n] = rng.random(n) < 0.9
            w = np.packbits(bits, bitorder="little").view(np.uint64)
            w[1::2] = 0
            words.append(w)
            continue
        else:
            bits[:n] = 0
            for w0 in range(0, n, 64):
                bits[w0 + int(rng.integers(0, min(64, n - w0)))] = 1
        words.append(np.packbits(bits, bitorder="little").view(np.uint64))
    return dict(keys=keys, fks=fks, hows=hows, kouts=kouts, src=np.concatenate(words),
                tables=tables)


def star_cases():
    """The kernel's cases: 1 to 4 legs, types cycling through all eight,
    every table label, the three sources, all semi / all anti / mixed, code
    output on all, some and no semi legs."""
    out = []
    seed = 0
    for nlegs in (1, 2, 3, 4):
        for source in ("dense", "alternate", "single"):
            for mix in ("semi", "anti", "mixed"):
                seed += 1
                hows = {"semi": ["semi"] * nlegs, "anti": ["anti"] * nlegs,
                        "mixed": ["semi" if (seed + i) % 2 else "anti" for i in range(nlegs)]}[mix]
                semis = [i for i, h in enumerate(hows) if h == "semi"]
                for outs in ("all", "some", "none"):
                    if outs == "some" and len(semis) < 2:
                        continue
                    take = {"all": semis, "some": semis[1:], "none": []}[outs]
                    # the code tables in another order than the legs
                    kouts = [-1] * nlegs
                    for j, i in enumerate(reversed(take)):
                        kouts[i] = j
                    c = star_case(nlegs, seed, hows=hows, kouts=kouts, source=source,
                                  type0=seed)
                    c["label"] = f"{nlegs}legs-{source}-{mix}-out:{outs}-" + "/".join(c["tables"])
                    out.append(c)
    return out


def unpack(words: np.ndarray, w0: int, n: int) -> np.ndarray:
    nw = (n + 63) // 64
    return np.unpackbits(words[w0:w0 + nw].view(np.uint8), bitorder="little")[:n].astype(bool)
