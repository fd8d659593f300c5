"""Config-5 benchmark: SSD -> HBM -> LZ4 / ZSTD decode -> filter of one
column of an Arrow IPC file (models/arrow_scan.py), against pyarrow on the CPU.

The file is written by pyarrow (LZ4_FRAME body compression, linked 64 KiB
blocks as pyarrow writes them; or ZSTD with ``--codec zstd``) with three columns — ``id`` (int64,
sequential), ``val`` (int64, uniform in [0, 1e6)) and ``x`` (float64, 5 %
nulls) — in record batches of ``--batch-rows``.  Each timed run starts with
the file evicted from the page cache.  Reported per scanned column:

  column_GBps   decoded column bytes / wall time of ArrowScan.scan
  file_GBps     file bytes moved storage -> HBM / wall time
  cpu_GBps      the same scan with pyarrow on the host (memory-mapped file,
                LZ4 decode + compute.and of two comparisons + indices)
  verified      GPU row ids == numpy row ids of the regenerated column

Every scan spec runs on a FRESH ArrowScan: the first run is the cold scan a
query actually pays (file open + footer/batch-header parse + plan + HBM slot
allocation + first kernel launches), reported as ``cold_ms`` /
``column_GBps_cold``; the remaining runs (file evicted each time) are warm
and reported by their median (``column_GBps`` = warm median, not the best).

The ``qual2`` row is a PG-Strom qualifier list: ``val`` and ``x`` ranges
(each column read and decoded once, bitmaps ANDed on the device) with ``id``
projected for the selected rows; rows AND projected values are verified
against numpy.

``--strings`` (default on) adds a second file (``--string-rows``) with a
utf8 ``name`` column (words of 3-24 bytes), a dictionary-encoded ``cat``
(1000 categories), a date32 ``day`` and a timestamp ``ts``, and rows for a
string-equality scan, a string prefix, contains, suffix and LIKE
(``str_contains`` / ``str_suffix`` / ``str_like``), a dictionary equality, a dictionary
range, and a date range AND an OR of timestamp ranges — each verified
against pyarrow.compute (row ids of Table.filter of the same expression),
whose time on the memory-mapped file is ``cpu_ms``.

``--agg`` adds the aggregate rows (``agg_rows``): ``ArrowScan.aggregate`` of
count(*), sum(id), min(x), max(x) under the ``val`` and ``x`` ranges, alternated
with ``scan_where(project="id")`` + a torch sum, and against four such scans.

``--join`` adds the join rows (``join_rows``): a scan whose last predicate
is a semi-join of ``val`` with a 4,096-key dimension alternated with the same
scan under ``P("val").isin(the same keys)``, and ``aggregate(join=,
by=dim[attr])`` against two projection scans plus a torch searchsorted /
gather / index_add.

``python -m nvme_strom_amd.tools.arrow_bench --out gpurun_out/arrow.json``
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np


def _log(*a):
    print(*a, file=sys.stderr, flush=True)


def make_file(path: str, rows: int, batch_rows: int, seed: int = 7, codec: str = "lz4") -> None:
    import pyarrow as pa
    import pyarrow.ipc as ipc
    if os.path.exists(path):
        return
    schema = pa.schema([("id", pa.int64()), ("val", pa.int64()), ("x", pa.float64())])
    rng = np.random.default_rng(seed)
    tmp = path + ".tmp"
    with ipc.new_file(tmp, schema, options=ipc.IpcWriteOptions(compression=codec)) as w:
        for b0 in range(0, rows, batch_rows):
            n = min(batch_rows, rows - b0)
            ids = np.arange(b0, b0 + n, dtype=np.int64)
            val = rng.integers(0, 1_000_000, n, dtype=np.int64)
            x = rng.random(n)
            mask = rng.random(n) < 0.05
            w.write_batch(pa.record_batch([pa.array(ids), pa.array(val),
                                           pa.array(x, mask=mask)], schema=schema))
            if (b0 // batch_rows) % 256 == 255:
                _log(f"writing {b0 + n}/{rows} rows")
    os.replace(tmp, path)


def column_np(path: str, name: str):
    import pyarrow as pa
    import pyarrow.ipc as ipc
    with pa.memory_map(path) as src:
        t = ipc.open_file(src).read_all()
    c = t.column(name).combine_chunks()
    vals = c.to_numpy(zero_copy_only=False)
    valid = ~np.asarray(c.is_null()) if c.null_count else None
    return vals, valid


def cpu_scan(path: str, name: str, lo, hi) -> tuple:
    import pyarrow as pa
    import pyarrow.compute as pc
    import pyarrow.ipc as ipc
    t0 = time.perf_counter()
    with pa.memory_map(path) as src:
        r = ipc.open_file(src)
        sel, base = [], 0
        for i in range(r.num_record_batches):
            col = r.get_batch(i).column(name)
            m = pc.and_(pc.greater_equal(col, lo), pc.less_equal(col, hi))
            idx = np.flatnonzero(np.asarray(m.fill_null(False)))
            sel.append(idx + base)
            base += len(col)
    n = int(sum(len(s) for s in sel))
    return time.perf_counter() - t0, n


def make_string_file(path: str, rows: int, batch_rows: int, seed: int = 9,
                     codec: str = "lz4") -> None:
    """name: utf8 words (a 20k vocabulary, 3-24 bytes), cat: dictionary of
    1000 categories, day: date32, ts: timestamp[us, UTC], sid: int64."""
    import pyarrow as pa
    import pyarrow.ipc as ipc
    if os.path.exists(path):
        return
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", np.uint8)
    vocab = []
    for k in range(20000):
        n = int(rng.integers(3, 25))
        vocab.append(letters[rng.integers(0, 26, n)].tobytes().decode())
    vocab = pa.array(vocab)
    cats = pa.array([f"cat_{k:05d}" for k in range(1000)])
    schema = pa.schema([("sid", pa.int64()), ("name", pa.string()),
                        ("cat", pa.dictionary(pa.int32(), pa.string())),
                        ("day", pa.date32()), ("ts", pa.timestamp("us", tz="UTC"))])
    ts0 = np.datetime64("2024-01-01T00:00:00", "us").astype(np.int64)
    tmp = path + ".tmp"
    with ipc.new_file(tmp, schema, options=ipc.IpcWriteOptions(compression=codec)) as w:
        for b0 in range(0, rows, batch_rows):
            n = min(batch_rows, rows - b0)
            name = pa.DictionaryArray.from_arrays(
                pa.array(rng.integers(0, len(vocab), n).astype(np.int32)), vocab).dictionary_decode()
            cat = pa.DictionaryArray.from_arrays(
                pa.array(rng.integers(0, 1000, n).astype(np.int32)), cats)
            day = pa.array(rng.integers(18000, 20000, n).astype(np.int32)).view(pa.date32())
            ts = pa.array(ts0 + rng.integers(0, 365 * 86400 * 10**6, n)).view(
                pa.timestamp("us", tz="UTC"))
            w.write_batch(pa.record_batch([pa.array(np.arange(b0, b0 + n, dtype=np.int64)), name,
                                           cat, day, ts], schema=schema))
            if (b0 // batch_rows) % 256 == 255:
                _log(f"writing {b0 + n}/{rows} string rows")
    os.replace(tmp, path)


def pc_expr(quals):
    """The qualifier list as a pyarrow compute Expression (Kleene OR: SQL)."""
    import pyarrow.compute as pc
    from nvme_strom_amd.ops.colpred import Or, as_pred

    def one(p):
        f = pc.field(p.col)
        v = p.value
        return {"==": lambda: f == v, "!=": lambda: f != v, "<": lambda: f < v,
                "<=": lambda: f <= v, ">": lambda: f > v, ">=": lambda: f >= v,
                "between": lambda: (f >= v[0]) & (f <= v[1]),
                "in": lambda: f.isin(list(v)),
                "prefix": lambda: pc.starts_with(f, pattern=v),
                "contains": lambda: pc.match_substring(f, pattern=v),
                "suffix": lambda: pc.ends_with(f, pattern=v),
                "like": lambda: pc.match_like(f, pattern=v)}[p.op]()
    e = None
    for q in quals:
        c = None
        for p in (q.preds if isinstance(q, Or) else [as_pred(q)]):
            c = one(p) if c is None else (c | one(p))
        e = c if e is None else (e & c)
    return e


def pc_scan(path: str, quals) -> tuple:
    """pyarrow on the host: memory-mapped file, the same expression -> row ids."""
    import pyarrow as pa
    import pyarrow.ipc as ipc
    t0 = time.perf_counter()
    with pa.memory_map(path) as src:
        t = ipc.open_file(src).read_all()
        t = t.append_column("__row", pa.array(np.arange(t.num_rows, dtype=np.int64)))
        ids = np.asarray(t.filter(pc_expr(quals)).column("__row"))
    return time.perf_counter() - t0, ids


def agg_rows(path: str, fd: int, a, col) -> dict:
    """``aggregate([val range, x range], [count(*), sum(id), min(x), max(x)])``
    alternated with what the same answer costs without it: for one of those
    aggregates, ``scan_where(same quals, project="id")`` + ``values.sum()`` in
    torch; for all four, four such scans (ids only for the count, ``id`` for
    the sum, ``x`` twice for min and max).  ``--agg-pairs`` alternated runs at
    the two selectivities of the scan rows, the order flipped every pair, the
    file evicted before every run; ratios are medians over the pairs."""
    import torch

    import nvme_strom_amd as S
    from nvme_strom_amd.models.arrow_scan import ArrowScan
    aggs = [("count", None), ("sum", "id"), ("min", "x"), ("max", "x")]
    rows = {}
    for label, quals in (("wide", [("val", 100_000, 599_999), ("x", 0.25, 0.75)]),
                         ("narrow", [("val", 100_000, 199_999), ("x", 0.25, 0.5)])):
        sc = ArrowScan(path, "cuda", slot_bytes=a.slot_mib << 20, nslots=a.nslots or None,
                       chunk_sz=(a.chunk_kib << 10) or None)

        def t_agg():
            S.evict_file(fd)
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = sc.aggregate(quals, aggs)
            return time.perf_counter() - t, out

        def t_proj(proj, reduce):
            S.evict_file(fd)
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = sc.scan_where(quals, project=proj)
            v = reduce(out)
            return time.perf_counter() - t, v, out

        def x_valid(out):
            return out.values if out.valid is None else out.values[out.valid.bool()]
        four = [(None, lambda o: o.selected), ("id", lambda o: int(o.values.sum().item())),
                ("x", lambda o: float(x_valid(o).min().item())),
                ("x", lambda o: float(x_valid(o).max().item()))]
        try:
            t_agg()                                   # cold runs: plans, slots, code objects
            t_proj("id", four[1][1])
            t_proj("x", four[2][1])
            agg_s, proj_s, four_s = [], [], []
            for k in range(max(1, a.agg_pairs)):
                order = ("agg", "proj") if k % 2 == 0 else ("proj", "agg")
                for what in order:
                    if what == "agg":
                        dt, out = t_agg()
                        agg_s.append(dt)
                    else:
                        dt, psum, pout = t_proj("id", four[1][1])
                        proj_s.append(dt)
                got4, dt4 = [], 0.0
                for proj, red in four:
                    dt, v, _ = t_proj(proj, red)
                    dt4 += dt
                    got4.append(v)
                four_s.append(dt4)
                _log(f"agg {label} pair {k}: aggregate {agg_s[-1] * 1e3:.1f} ms, project+sum "
                     f"{proj_s[-1] * 1e3:.1f} ms, four scans {dt4 * 1e3:.1f} ms")
        finally:
            sc.close()
        m = None
        for name, lo, hi in quals:
            vals, valid = col(name)
            mm = (vals >= lo) & (vals <= hi)
            if valid is not None:
                mm &= valid
            m = mm if m is None else m & mm
        xs = col("x")[0][m]
        want = [int(m.sum()), int(col("id")[0][m].sum()), float(xs.min()), float(xs.max())]
        got = [int(out.get("count")[0][0]), int(out.get("sum", "id")[0][0]),
               float(out.get("min", "x")[0][0]), float(out.get("max", "x")[0][0])]
        ratios = [x / y for x, y in zip(agg_s, proj_s)]
        rows[label] = dict(
            quals=[repr(q) for q in quals], aggs=[list(x) for x in aggs], selected=out.selected,
            verified=bool(got == want and got4 == want and psum == want[1]),
            bytes_read=out.bytes_read, proj_bytes_read=pout.bytes_read,
            column_bytes=out.column_bytes, groups=out.groups, pairs=len(agg_s),
            aggregate_ms=[round(x * 1e3, 2) for x in agg_s],
            project_sum_ms=[round(x * 1e3, 2) for x in proj_s],
            four_scans_ms=[round(x * 1e3, 2) for x in four_s],
            ratio_aggregate_over_project_sum=[round(r, 4) for r in ratios],
            median_ratio=round(float(np.median(ratios)), 4),
            median_ratio_vs_four_scans=round(float(np.median(
                [x / y for x, y in zip(agg_s, four_s)])), 4),
            column_GBps=round(out.column_bytes / float(np.median(agg_s)) / 1e9, 2))
        _log(json.dumps(rows[label]))
    return rows


def join_rows(path: str, fd: int, a, col) -> dict:
    """Scan row: ``scan_where([x range], join=Join("val", dim))`` alternated
    with ``scan_where([x range, P("val").isin(keys)])`` for the same 4,096
    keys — the largest list the qualifier kernels hold; both read and decode
    ``x`` and ``val``, only the last launch differs.  Query row:
    ``aggregate([x range], [count(*), sum(id)], by=dim["cat"], join=)`` over
    a 131,072-key dimension of 64 categories against what it takes without
    the join: ``scan_where(project="val")`` and ``scan_where(project="id")``,
    then searchsorted, gather and index_add in torch.  ``--join-pairs``
    alternated runs, the order flipped every pair, the file evicted before
    every run; ratios are medians over the pairs."""
    import torch

    import nvme_strom_amd as S
    from nvme_strom_amd.models.arrow_scan import ArrowScan, Join, JoinTable
    from nvme_strom_amd.ops.colpred import P
    rng = np.random.default_rng(17)
    quals = [("x", 0.25, 0.75)]
    all_keys = rng.choice(1_000_000, 4096, replace=False).astype(np.int64)
    bkeys = np.sort(rng.choice(1_000_000, 131_072, replace=False)).astype(np.int64)
    bcats = rng.integers(0, 64, len(bkeys))
    big = JoinTable(bkeys, attrs={"cat": bcats}, device="cuda")
    ncat = len(big["cat"].values)
    d_bkeys = torch.from_numpy(bkeys).cuda()
    d_bcodes = torch.from_numpy(big["cat"].codes.astype(np.int64)).cuda()
    sc = ArrowScan(path, "cuda", slot_bytes=a.slot_mib << 20, nslots=a.nslots or None,
                   chunk_sz=(a.chunk_kib << 10) or None)

    def timed(fn):
        S.evict_file(fd)
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        return time.perf_counter() - t, out

    def t_join():
        return timed(lambda: sc.scan_where(quals, join=Join("val", dim)))

    def t_isin():
        return timed(lambda: sc.scan_where(quals + [P("val").isin(keys.tolist())]))

    aggs = [("count", None), ("sum", "id")]

    def t_agg():
        return timed(lambda: sc.aggregate(quals, aggs, by=big["cat"], join=Join("val", big)))

    def two_scans():
        fk = sc.scan_where(quals, project="val")
        ids = sc.scan_where(quals, project="id")
        pos = torch.searchsorted(d_bkeys, fk.values).clamp_(max=len(bkeys) - 1)
        hit = d_bkeys[pos] == fk.values
        codes = d_bcodes[pos[hit]]
        cnt = torch.bincount(codes, minlength=ncat)
        sm = torch.zeros(ncat, dtype=torch.int64, device="cuda").index_add_(0, codes,
                                                                            ids.values[hit])
        return cnt.cpu().numpy(), sm.cpu().numpy(), fk.bytes_read + ids.bytes_read
    dim = None
    try:
        # cold runs: plans, slots, code objects.  The isin list is as long as
        # the qualifier kernel's LDS staging takes on this device
        for nk in (4096, 4064, 3072):
            keys = np.sort(all_keys[:nk])
            try:
                t_isin()
                break
            except RuntimeError as e:
                _log(f"isin of {nk} keys refused: {e}")
        dim = JoinTable(keys, device="cuda")
        t_join(), t_agg(), timed(two_scans)
        join_s, isin_s, agg_s, two_s = [], [], [], []
        for k in range(max(1, a.join_pairs)):
            for what in (("join", "isin") if k % 2 == 0 else ("isin", "join")):
                if what == "join":
                    dt, jout = t_join()
                    join_s.append(dt)
                else:
                    dt, iout = t_isin()
                    isin_s.append(dt)
            for what in (("agg", "two") if k % 2 == 0 else ("two", "agg")):
                if what == "agg":
                    dt, aout = t_agg()
                    agg_s.append(dt)
                else:
                    dt, (tcnt, tsum, tbytes) = timed(two_scans)
                    two_s.append(dt)
            _log(f"join pair {k}: join {join_s[-1] * 1e3:.1f} ms, isin {isin_s[-1] * 1e3:.1f} ms; "
                 f"aggregate {agg_s[-1] * 1e3:.1f} ms, two scans + torch {two_s[-1] * 1e3:.1f} ms")
    finally:
        sc.close()
        if dim is not None:
            dim.close()
        big.close()
    xv, xok = col("x")
    m = (xv >= 0.25) & (xv <= 0.75)
    if xok is not None:
        m &= xok
    val = col("val")[0]
    ref = np.flatnonzero(m & np.isin(val, keys))
    ok_scan = bool(np.array_equal(jout.indices.cpu().numpy(), ref) and
                   np.array_equal(iout.indices.cpu().numpy(), ref))
    mb = m & np.isin(val, bkeys)
    code = big["cat"].codes[np.searchsorted(bkeys, val[mb])]
    want_cnt = np.bincount(code, minlength=ncat)
    want_sum = np.zeros(ncat, np.int64)
    np.add.at(want_sum, code, col("id")[0][mb])
    order = [big["cat"].values.index(kv) for kv in aout.keys]
    ok_agg = bool(np.array_equal(aout.count_all, want_cnt[order]) and
                  np.array_equal(aout.get("sum", "id")[0], want_sum[order]) and
                  np.array_equal(tcnt, want_cnt) and np.array_equal(tsum, want_sum))
    r1 = [x / y for x, y in zip(join_s, isin_s)]
    r2 = [x / y for x, y in zip(agg_s, two_s)]
    rows = dict(
        scan=dict(quals=[repr(q) for q in quals], keys=len(keys), selected=jout.selected,
                  verified=ok_scan, bytes_read=jout.bytes_read, isin_bytes_read=iout.bytes_read,
                  groups=jout.groups, pairs=len(r1),
                  join_ms=[round(x * 1e3, 2) for x in join_s],
                  isin_ms=[round(x * 1e3, 2) for x in isin_s],
                  ratio_join_over_isin=[round(r, 4) for r in r1],
                  median_ratio=round(float(np.median(r1)), 4),
                  min_ratio=round(min(r1), 4), max_ratio=round(max(r1), 4)),
        query=dict(aggs=[list(x) for x in aggs], keys=len(bkeys), categories=ncat,
                   selected=aout.selected, verified=ok_agg, bytes_read=aout.bytes_read,
                   two_scans_bytes_read=int(tbytes), pairs=len(r2),
                   aggregate_ms=[round(x * 1e3, 2) for x in agg_s],
                   two_scans_torch_ms=[round(x * 1e3, 2) for x in two_s],
                   median_ratio=round(float(np.median(r2)), 4),
                   min_ratio=round(min(r2), 4), max_ratio=round(max(r2), 4)))
    _log(json.dumps(rows))
    return rows


def star_row(path: str, fd: int, a, col) -> dict:
    """``aggregate([x range], [count(*), sum(id)], by=HashBy([dimA["cat"],
    dimB["cat"]]), join=StarJoin(Join("val", dimA), Join("id", dimB)))`` — two
    dimensions probed in one pass, grouped by an attribute of each — against
    the same answer through one join per scan: ``scan_where(project="id",
    join=Join("val", dimA))`` and the same scan projecting ``val``, then
    searchsorted, gather, bincount and index_add in torch.  dimA: 131,072 keys
    of 64 categories; dimB: up to 2^20 of the file's ids, 16 categories.
    ``--join-pairs`` alternated runs, the order flipped every pair, the file
    evicted before every run; both verified against numpy."""
    import torch

    import nvme_strom_amd as S
    from nvme_strom_amd.models.arrow_scan import ArrowScan, HashBy, Join, JoinTable, StarJoin
    rng = np.random.default_rng(19)
    quals = [("x", 0.25, 0.75)]
    aggs = [("count", None), ("sum", "id")]
    akeys = np.sort(rng.choice(1_000_000, 131_072, replace=False)).astype(np.int64)
    bkeys = np.sort(rng.choice(a.rows, min(max(a.rows // 2, 1), 1 << 20),
                               replace=False)).astype(np.int64)
    dim_a = JoinTable(akeys, attrs={"cat": rng.integers(0, 64, len(akeys))}, device="cuda")
    dim_b = JoinTable(bkeys, attrs={"cat": rng.integers(0, 16, len(bkeys))}, device="cuda")
    na, nb = len(dim_a["cat"].values), len(dim_b["cat"].values)
    d_akeys, d_bkeys = torch.from_numpy(akeys).cuda(), torch.from_numpy(bkeys).cuda()
    d_acodes = torch.from_numpy(dim_a["cat"].codes.astype(np.int64)).cuda()
    d_bcodes = torch.from_numpy(dim_b["cat"].codes.astype(np.int64)).cuda()
    sc = ArrowScan(path, "cuda", slot_bytes=a.slot_mib << 20, nslots=a.nslots or None,
                   chunk_sz=(a.chunk_kib << 10) or None)
    star = StarJoin(Join("val", dim_a), Join("id", dim_b))
    by = HashBy([dim_a["cat"], dim_b["cat"]], groups=na * nb)

    def timed(fn):
        S.evict_file(fd)
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        return time.perf_counter() - t, out

    def one_pass():
        return sc.aggregate(quals, aggs, by=by, join=star)

    def two_scans():
        ids = sc.scan_where(quals, project="id", join=Join("val", dim_a))
        fk = sc.scan_where(quals, project="val", join=Join("val", dim_a))
        ca = d_acodes[torch.searchsorted(d_akeys, fk.values)]
        pos = torch.searchsorted(d_bkeys, ids.values).clamp_(max=len(bkeys) - 1)
        hit = d_bkeys[pos] == ids.values
        codes = ca[hit] * nb + d_bcodes[pos[hit]]
        cnt = torch.bincount(codes, minlength=na * nb)
        sm = torch.zeros(na * nb, dtype=torch.int64, device="cuda").index_add_(
            0, codes, ids.values[hit])
        return cnt.cpu().numpy(), sm.cpu().numpy(), fk.bytes_read + ids.bytes_read
    try:
        timed(one_pass), timed(two_scans)            # cold runs: plans, slots, code objects
        star_s, two_s = [], []
        for k in range(max(1, a.join_pairs)):
            for what in (("star", "two") if k % 2 == 0 else ("two", "star")):
                if what == "star":
                    dt, sout = timed(one_pass)
                    star_s.append(dt)
                else:
                    dt, (tcnt, tsum, tbytes) = timed(two_scans)
                    two_s.append(dt)
            _log(f"star pair {k}: one pass {star_s[-1] * 1e3:.1f} ms, two scans + torch "
                 f"{two_s[-1] * 1e3:.1f} ms")
    finally:
        sc.close()
        dim_a.close()
        dim_b.close()
    xv, xok = col("x")
    m = (xv >= 0.25) & (xv <= 0.75)
    if xok is not None:
        m &= xok
    val, ids = col("val")[0], col("id")[0]
    m &= np.isin(val, akeys) & np.isin(ids, bkeys)
    code = dim_a["cat"].codes[np.searchsorted(akeys, val[m])].astype(np.int64) * nb + \
        dim_b["cat"].codes[np.searchsorted(bkeys, ids[m])]
    want_cnt = np.bincount(code, minlength=na * nb)
    want_sum = np.zeros(na * nb, np.int64)
    np.add.at(want_sum, code, ids[m])
    order = [dim_a["cat"].values.index(ka) * nb + dim_b["cat"].values.index(kb)
             for ka, kb in sout.keys]
    ok = bool(len(order) == int((want_cnt > 0).sum()) and
              np.array_equal(sout.count_all, want_cnt[order]) and
              np.array_equal(sout.get("sum", "id")[0], want_sum[order]) and
              np.array_equal(tcnt, want_cnt) and np.array_equal(tsum, want_sum))
    r = [x / y for x, y in zip(star_s, two_s)]
    row = dict(aggs=[list(x) for x in aggs], keys=[len(akeys), len(bkeys)], categories=[na, nb],
               selected=sout.selected, groups_found=len(sout.keys), verified=ok,
               bytes_read=sout.bytes_read, two_scans_bytes_read=int(tbytes), pairs=len(r),
               star_ms=[round(x * 1e3, 2) for x in star_s],
               two_scans_torch_ms=[round(x * 1e3, 2) for x in two_s],
               median_star_ms=round(float(np.median(star_s)) * 1e3, 2),
               median_two_scans_torch_ms=round(float(np.median(two_s)) * 1e3, 2),
               median_ratio=round(float(np.median(r)), 4),
               min_ratio=round(min(r), 4), max_ratio=round(max(r), 4))
    _log(json.dumps(row))
    return row


def hashagg_row(path: str, fd: int, a, col) -> dict:
    """``aggregate([x range], [count(*), sum(id), max(x)], by=HashBy("val",
    groups=1 << 20))`` — ``val`` has a million distinct values, an id-like
    key — alternated with the same aggregates without a key (the same columns
    read and decoded; the hash step and the atomics are the difference).  The
    file is evicted before every run; verified against numpy."""
    import torch

    import nvme_strom_amd as S
    from nvme_strom_amd.models.arrow_scan import ArrowScan, HashBy
    quals = [("x", 0.25, 0.75)]
    aggs = [("count", None), ("sum", "id"), ("max", "x")]
    sc = ArrowScan(path, "cuda", slot_bytes=a.slot_mib << 20, nslots=a.nslots or None,
                   chunk_sz=(a.chunk_kib << 10) or None)

    def timed(fn):
        S.evict_file(fd)
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        return time.perf_counter() - t, out
    hash_s, flat_s = [], []
    try:
        by = HashBy("val", groups=1 << 20)
        timed(lambda: sc.aggregate(quals, aggs, by=by))           # cold: plans, slots, code
        timed(lambda: sc.aggregate(quals, aggs + [("count", "val")]))
        for k in range(max(1, a.agg_pairs)):
            for what in (("hash", "flat") if k % 2 == 0 else ("flat", "hash")):
                if what == "hash":
                    dt, out = timed(lambda: sc.aggregate(quals, aggs, by=by))
                    hash_s.append(dt)
                else:
                    dt, flat = timed(lambda: sc.aggregate(quals, aggs + [("count", "val")]))
                    flat_s.append(dt)
            _log(f"hashagg pair {k}: HashBy {hash_s[-1] * 1e3:.1f} ms, no key "
                 f"{flat_s[-1] * 1e3:.1f} ms")
    finally:
        sc.close()
    xv, xok = col("x")
    m = (xv >= 0.25) & (xv <= 0.75)
    if xok is not None:
        m &= xok
    val = col("val")[0][m]
    keys, inv = np.unique(val, return_inverse=True)
    want_sum = np.zeros(len(keys), np.int64)
    np.add.at(want_sum, inv, col("id")[0][m])
    want_max = np.full(len(keys), -np.inf)
    np.maximum.at(want_max, inv, xv[m])
    ok = bool(out.keys == keys.tolist() and
              np.array_equal(out.count_all, np.bincount(inv, minlength=len(keys))) and
              np.array_equal(out.get("sum", "id")[0], want_sum) and
              np.array_equal(out.get("max", "x")[0], want_max) and
              flat.selected == out.selected)
    ratios = [x / y for x, y in zip(hash_s, flat_s)]
    row = dict(quals=[repr(q) for q in quals], aggs=[list(x) for x in aggs], by="HashBy(val)",
               groups_param=1 << 20, distinct_keys=len(keys), selected=out.selected, verified=ok,
               bytes_read=out.bytes_read, column_bytes=out.column_bytes, groups=out.groups,
               hashby_ms=[round(x * 1e3, 2) for x in hash_s],
               no_key_ms=[round(x * 1e3, 2) for x in flat_s],
               median_ratio_hashby_over_no_key=round(float(np.median(ratios)), 4),
               hashby_breakdown_s={k: round(v, 4) for k, v in out.seconds.items()},
               column_GBps=round(out.column_bytes / float(np.median(hash_s)) / 1e9, 2))
    _log(json.dumps(row))
    return row


def expr_row(path: str, fd: int, a, col) -> dict:
    """``aggregate([], [sum(E("val") * E("x"))])`` — a computed column
    (colexpr.hip) aggregated — alternated with ``aggregate([], [sum(val),
    sum(x)])``: both read and decode the same two columns, so the difference is
    the expression stage (one launch per group, 8 bytes per row written and
    read again).  The file is evicted before every run; the sum is verified
    against numpy within the float-sum bound."""
    import math

    import torch

    import nvme_strom_amd as S
    from nvme_strom_amd.models.arrow_scan import ArrowScan
    from nvme_strom_amd.ops.colexpr import E
    e = E("val") * E("x")
    with_e, plain = [("sum", e)], [("sum", "val"), ("sum", "x")]
    sc = ArrowScan(path, "cuda", slot_bytes=a.slot_mib << 20, nslots=a.nslots or None,
                   chunk_sz=(a.chunk_kib << 10) or None)

    def timed(fn):
        S.evict_file(fd)
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        return time.perf_counter() - t, out
    expr_s, plain_s = [], []
    try:
        timed(lambda: sc.aggregate([], with_e))                   # cold: plans, slots, code
        timed(lambda: sc.aggregate([], plain))
        for k in range(max(1, a.agg_pairs)):
            for what in (("expr", "plain") if k % 2 == 0 else ("plain", "expr")):
                if what == "expr":
                    dt, out = timed(lambda: sc.aggregate([], with_e))
                    expr_s.append(dt)
                else:
                    dt, flat = timed(lambda: sc.aggregate([], plain))
                    plain_s.append(dt)
            _log(f"expr pair {k}: sum(val * x) {expr_s[-1] * 1e3:.1f} ms, sum(val), sum(x) "
                 f"{plain_s[-1] * 1e3:.1f} ms")
    finally:
        sc.close()
    (vv, vok), (xv, xok) = col("val"), col("x")
    m = np.ones(len(vv), bool)
    for okk in (vok, xok):
        if okk is not None:
            m &= okk
    prod = vv[m].astype(np.float64) * xv[m].astype(np.float64)
    got = float(out.get("sum", e)[0][0])
    ok = bool(abs(got - math.fsum(prod)) <= len(prod) * 2.0 ** -52 * math.fsum(np.abs(prod)) and
              out.selected == flat.selected and out.bytes_read == flat.bytes_read)
    ratios = [x / y for x, y in zip(expr_s, plain_s)]
    row = dict(aggs=["sum(val * x)"], against=["sum(val)", "sum(x)"], selected=out.selected,
               verified=ok, bytes_read=out.bytes_read, column_bytes=out.column_bytes,
               groups=out.groups, expr_ms=[round(x * 1e3, 2) for x in expr_s],
               plain_ms=[round(x * 1e3, 2) for x in plain_s],
               median_ratio_expr_over_plain=round(float(np.median(ratios)), 4),
               expr_breakdown_s={k: round(v, 4) for k, v in out.seconds.items()},
               column_GBps=round(out.column_bytes / float(np.median(expr_s)) / 1e9, 2))
    _log(json.dumps(row))
    return row


def order_row(path: str, fd: int, a, col) -> dict:
    """The select query (``project=["id", "x", "val"]``) with and without
    ``order_by=[("val", "descending"), "x"]`` on the same file, alternated,
    the file evicted before every scan and the device synchronized after it
    (the sort's launches are enqueued, not waited for, by the scan itself).
    Reports both medians and the sort stage's share of the ordered scan; the
    order is verified against numpy's lexsort."""
    import torch

    import nvme_strom_amd as S
    from nvme_strom_amd.models.arrow_scan import ArrowScan
    quals = [("val", 100_000, 599_999), ("x", 0.25, 0.75)]
    names = ["id", "x", "val"]
    order_by = [("val", "descending"), "x"]
    sc = ArrowScan(path, "cuda", slot_bytes=a.slot_mib << 20, nslots=a.nslots or None,
                   chunk_sz=(a.chunk_kib << 10) or None)

    def timed(**kw):
        S.evict_file(fd)
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = sc.scan_where(quals, project=names, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t, out
    plain_s, order_s = [], []
    try:
        timed()                                                  # cold: plans, slots, code
        timed(order_by=order_by)
        for k in range(max(1, a.agg_pairs)):
            for what in (("plain", "order") if k % 2 == 0 else ("order", "plain")):
                if what == "plain":
                    plain_s.append(timed()[0])
                else:
                    dt, out = timed(order_by=order_by)
                    order_s.append(dt)
            _log(f"order pair {k}: plain {plain_s[-1] * 1e3:.1f} ms, ordered "
                 f"{order_s[-1] * 1e3:.1f} ms")
    finally:
        sc.close()
    m = None
    for name, lo, hi in quals:
        vals, valid = col(name)
        mm = (vals >= lo) & (vals <= hi)
        if valid is not None:
            mm &= valid
        m = mm if m is None else m & mm
    ref = np.flatnonzero(m)
    ref = ref[np.lexsort((col("x")[0][ref], -col("val")[0][ref].astype(np.int64)))]
    ok = bool(np.array_equal(out.indices.cpu().numpy(), ref)) and \
        int(out.sort_errors.item()) == 0
    for n, c in zip(names, out.columns):
        ok = ok and bool(np.array_equal(c.values.cpu().numpy(), col(n)[0][ref]))
    mp, mo = float(np.median(plain_s)), float(np.median(order_s))
    row = dict(project=names, order_by=[list(o) if isinstance(o, tuple) else o for o in order_by],
               quals=[repr(q) for q in quals], selected=out.selected, verified=ok,
               plain_ms=[round(x * 1e3, 2) for x in plain_s],
               ordered_ms=[round(x * 1e3, 2) for x in order_s],
               plain_median_ms=round(mp * 1e3, 2), ordered_median_ms=round(mo * 1e3, 2),
               sort_share_of_ordered_scan=round(max(mo - mp, 0.0) / mo, 4),
               sort_enqueue_s=round(out.seconds.get("sort_s", 0.0), 5))
    _log(json.dumps(row))
    return row


def select_row(path: str, fd: int, a, col) -> dict:
    """``SELECT id, x, val WHERE val BETWEEN .. AND x BETWEEN ..`` as one
    select-list scan (``project=["id", "x", "val"]``: one emit pass,
    colproject.hip) alternated with the same three columns fetched by three
    single-column scans of the same file.  The file is evicted before every
    scan; every column of both forms is verified against numpy."""
    import torch

    import nvme_strom_amd as S
    from nvme_strom_amd.models.arrow_scan import ArrowScan
    quals = [("val", 100_000, 599_999), ("x", 0.25, 0.75)]
    names = ["id", "x", "val"]
    sc = ArrowScan(path, "cuda", slot_bytes=a.slot_mib << 20, nslots=a.nslots or None,
                   chunk_sz=(a.chunk_kib << 10) or None)

    def timed(fn):
        S.evict_file(fd)
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        return time.perf_counter() - t, out

    def three():
        return [sc.scan_where(quals, project=n) for n in names]
    list_s, three_s = [], []
    try:
        timed(lambda: sc.scan_where(quals, project=names))       # cold: plans, slots, code
        timed(three)
        for k in range(max(1, a.agg_pairs)):
            for what in (("list", "three") if k % 2 == 0 else ("three", "list")):
                if what == "list":
                    dt, out = timed(lambda: sc.scan_where(quals, project=names))
                    list_s.append(dt)
                else:
                    dt, singles = timed(three)
                    three_s.append(dt)
            _log(f"select pair {k}: list {list_s[-1] * 1e3:.1f} ms, three scans "
                 f"{three_s[-1] * 1e3:.1f} ms")
    finally:
        sc.close()
    m = None
    for name, lo, hi in quals:
        vals, valid = col(name)
        mm = (vals >= lo) & (vals <= hi)
        if valid is not None:
            mm &= valid
        m = mm if m is None else m & mm
    ref = np.flatnonzero(m)
    ok = bool(np.array_equal(out.indices.cpu().numpy(), ref))
    for n, c, one in zip(names, out.columns, singles):
        want = col(n)[0][ref]
        ok = ok and bool(np.array_equal(c.values.cpu().numpy(), want)) and \
            bool(np.array_equal(one.values.cpu().numpy(), want))
    ratios = [x / y for x, y in zip(list_s, three_s)]
    row = dict(project=names, quals=[repr(q) for q in quals], selected=out.selected,
               rows_verified=int(len(ref)) if ok else 0, verified=ok,
               bytes_read=out.bytes_read, column_bytes=out.column_bytes, groups=out.groups,
               list_ms=[round(x * 1e3, 2) for x in list_s],
               three_scans_ms=[round(x * 1e3, 2) for x in three_s],
               list_median_ms=round(float(np.median(list_s)) * 1e3, 2),
               three_scans_median_ms=round(float(np.median(three_s)) * 1e3, 2),
               list_spread_ms=[round(min(list_s) * 1e3, 2), round(max(list_s) * 1e3, 2)],
               three_scans_spread_ms=[round(min(three_s) * 1e3, 2), round(max(three_s) * 1e3, 2)],
               median_ratio_list_over_three=round(float(np.median(ratios)), 4),
               list_breakdown_s={k: round(v, 4) for k, v in out.seconds.items()
                                 if isinstance(v, float)})
    _log(json.dumps(row))
    return row


def topk_rows(path: str, fd: int, a, col) -> dict:
    """ORDER BY ... LIMIT k rows: ``top val k=100`` (the ``val`` row's range
    as qualifier, ORDER BY val LIMIT 100), the same under qual2's two-column
    qualifier list with ``id`` carried, and ``x`` descending under the ``x``
    row's range (5 % nulls).  Each is alternated A B A B ... (--topk-pairs
    pairs, the file evicted before every scan) with A = ``scan_where`` of the
    same qualifier list and projection, which reads the same columns — what a
    caller had to run before, without the torch.topk it then still needed —
    and verified against numpy on the host (lexsort on class, key, row over
    the selected rows)."""
    import torch

    import nvme_strom_amd as S
    from nvme_strom_amd.models.arrow_scan import ArrowScan
    from nvme_strom_amd.ops import coltopk as T
    val_q = [("val", 100_000, 199_999)]
    specs = [("top val k=100", val_q, "val", 100, False, None),
             ("top val k=100 qual2", [("val", 100_000, 599_999), ("x", 0.25, 0.75)], "val", 100,
              False, "id"),
             ("top x desc k=100", [("x", 0.25, 0.5)], "x", 100, True, None)]
    rows = {}
    for label, quals, order, k, desc, proj in specs:
        sc = ArrowScan(path, "cuda", slot_bytes=a.slot_mib << 20, nslots=a.nslots or None,
                       chunk_sz=(a.chunk_kib << 10) or None)
        try:
            def timed(fn):
                S.evict_file(fd)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                out = fn()
                return time.perf_counter() - t1, out
            scan = lambda: sc.scan_where(quals, project=proj)
            top = lambda: sc.top(quals, order, k, desc, project=proj)
            timed(scan), timed(top)                       # plans, slots, code objects
            ta, tb = [], []
            for _ in range(a.topk_pairs):
                dt, base = timed(scan)
                ta.append(dt)
                dt, out = timed(top)
                tb.append(dt)
        finally:
            sc.close()
        m = None
        for name, lo, hi in quals:
            vals, valid = col(name)
            mm = (vals >= lo) & (vals <= hi)
            if valid is not None:
                mm &= valid
            m = mm if m is None else m & mm
        ids = np.flatnonzero(m)
        ov, ovalid = col(order)
        want = T.best(T.entries(ov[ids], None if ovalid is None else ovalid[ids], ids, desc,
                                ids.astype(np.int64) if proj else None), k)   # id is the row id
        ok = bool(np.array_equal(out._entries, want) and out.selected == len(ids) and
                  base.selected == len(ids))
        ma, mb = float(np.median(ta)), float(np.median(tb))
        rows[label] = dict(
            quals=[repr(q) for q in quals], order_by=order, k=k, descending=desc, project=proj,
            verified=ok,
            selected=out.selected, groups=out.groups, column_bytes=out.column_bytes,
            bytes_read=out.bytes_read, scan_where_bytes_read=base.bytes_read,
            scan_where_ms=[round(x * 1e3, 2) for x in ta], top_ms=[round(x * 1e3, 2) for x in tb],
            scan_where_median_ms=round(ma * 1e3, 2), top_median_ms=round(mb * 1e3, 2),
            scan_where_spread_ms=round((max(ta) - min(ta)) * 1e3, 2),
            top_minus_scan_where_ms=round((mb - ma) * 1e3, 2),
            column_GBps=round(out.column_bytes / mb / 1e9, 2),
            last_breakdown_s={k_: (round(v, 4) if isinstance(v, float) else v)
                              for k_, v in out.seconds.items() if k_ != "timeline_ms"})
        _log(label, json.dumps(rows[label]))
    return rows


def make_pairs_file(path: str, rows: int, batch_rows: int, side: int = 1024, seed: int = 9,
                    codec: str = "lz4") -> None:
    """``id`` int64 (the row number), ``a`` and ``b`` int32 uniform over
    ``side`` values each, and ``k`` int64 = a * 2^32 + b: the same pairs as
    one column."""
    import pyarrow as pa
    import pyarrow.ipc as ipc
    if os.path.exists(path):
        return
    schema = pa.schema([("id", pa.int64()), ("a", pa.int32()), ("b", pa.int32()),
                        ("k", pa.int64())])
    rng = np.random.default_rng(seed)
    tmp = path + ".tmp"
    with ipc.new_file(tmp, schema, options=ipc.IpcWriteOptions(compression=codec)) as w:
        for b0 in range(0, rows, batch_rows):
            n = min(batch_rows, rows - b0)
            av = rng.integers(0, side, n).astype(np.int32)
            bv = rng.integers(0, side, n).astype(np.int32)
            w.write_batch(pa.record_batch(
                [pa.array(np.arange(b0, b0 + n, dtype=np.int64)), pa.array(av), pa.array(bv),
                 pa.array(av.astype(np.int64) * (1 << 32) + bv)], schema=schema))
    os.replace(tmp, path)


def hashagg2_row(path: str, a) -> dict:
    """``aggregate([], [count(*), sum(id)], by=HashBy(["a", "b"], groups=1 <<
    20))`` — two int32 key columns, a million distinct pairs — alternated
    with ``by=HashBy("k")``, the same pairs packed in one int64 column of the
    same file (8 key bytes a row either way).  The file is evicted before
    every run; the two-key result is verified against numpy."""
    import torch

    import nvme_strom_amd as S
    from nvme_strom_amd.models.arrow_scan import ArrowScan, HashBy
    aggs = [("count", None), ("sum", "id")]
    fd = os.open(path, os.O_RDONLY)
    sc = ArrowScan(path, "cuda", slot_bytes=a.slot_mib << 20, nslots=a.nslots or None,
                   chunk_sz=(a.chunk_kib << 10) or None)

    def timed(fn):
        S.evict_file(fd)
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        return time.perf_counter() - t, out
    two_s, one_s = [], []
    two_sync, one_sync = [], []       # up to the scan's sync: without the result's Python keys
    try:
        by2, by1 = HashBy(["a", "b"], groups=1 << 20), HashBy("k", groups=1 << 20)
        timed(lambda: sc.aggregate([], aggs, by=by2))             # cold: plans, slots, code
        timed(lambda: sc.aggregate([], aggs, by=by1))
        for k in range(max(1, a.agg_pairs)):
            for what in (("two", "one") if k % 2 == 0 else ("one", "two")):
                if what == "two":
                    dt, out = timed(lambda: sc.aggregate([], aggs, by=by2))
                    two_s.append(dt)
                    two_sync.append(out.seconds["total_s"])
                else:
                    dt, one = timed(lambda: sc.aggregate([], aggs, by=by1))
                    one_s.append(dt)
                    one_sync.append(one.seconds["total_s"])
            _log(f"hashagg2 pair {k}: HashBy([a, b]) {two_s[-1] * 1e3:.1f} ms, HashBy(k) "
                 f"{one_s[-1] * 1e3:.1f} ms")
    finally:
        sc.close()
        os.close(fd)
    kv = column_np(path, "k")[0]
    keys, inv = np.unique(kv, return_inverse=True)
    want_sum = np.zeros(len(keys), np.int64)
    np.add.at(want_sum, inv, column_np(path, "id")[0])
    ok = bool(out.keys == list(zip((keys >> 32).tolist(), (keys & 0xFFFFFFFF).tolist())) and
              np.array_equal(out.count_all, np.bincount(inv, minlength=len(keys))) and
              np.array_equal(out.get("sum", "id")[0], want_sum) and
              one.keys == keys.tolist() and np.array_equal(one.count_all, out.count_all))
    ratios = [x / y for x, y in zip(two_s, one_s)]
    row = dict(aggs=[list(x) for x in aggs], by="HashBy([a, b])", against="HashBy(k)",
               groups_param=1 << 20, distinct_keys=len(keys), selected=out.selected, verified=ok,
               bytes_read=out.bytes_read, column_bytes=out.column_bytes, groups=out.groups,
               two_keys_ms=[round(x * 1e3, 2) for x in two_s],
               one_key_ms=[round(x * 1e3, 2) for x in one_s],
               median_ratio_two_over_one=round(float(np.median(ratios)), 4),
               two_keys_to_sync_ms=[round(x * 1e3, 2) for x in two_sync],
               one_key_to_sync_ms=[round(x * 1e3, 2) for x in one_sync],
               median_ratio_to_sync=round(float(np.median(two_sync) / np.median(one_sync)), 4),
               two_keys_breakdown_s={k: round(v, 4) for k, v in out.seconds.items()})
    _log(json.dumps(row))
    return row


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 27)
    ap.add_argument("--batch-rows", type=int, default=1 << 16)
    ap.add_argument("--dir", default="/tmp/strom_arrow")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slot-mib", type=int, default=256)
    ap.add_argument("--chunk-kib", type=int, default=0,
                    help="the scan's read chunk (buffers are read as whole chunks; 0: by codec)")
    ap.add_argument("--nslots", type=int, default=0,
                    help="HBM slots of the scan's ring (reads in flight: nslots - 1 groups)")
    ap.add_argument("--columns", default="val,x")
    ap.add_argument("--codec", default="lz4", choices=["lz4", "zstd"],
                    help="Arrow IPC body compression pyarrow writes the file with")
    ap.add_argument("--no-qual2", dest="qual2", action="store_false",
                    help="skip the two-column qualifier list + projection row")
    ap.add_argument("--no-strings", dest="strings", action="store_false",
                    help="skip the utf8 / dictionary / date / timestamp file and rows")
    ap.add_argument("--string-rows", type=int, default=1 << 26)
    ap.add_argument("--agg", action="store_true",
                    help="add the aggregate rows: ArrowScan.aggregate alternated with "
                         "scan_where(project=) + a torch reduction")
    ap.add_argument("--agg-pairs", type=int, default=5)
    ap.add_argument("--join", action="store_true",
                    help="add the join rows: a semi-join scan alternated with the same scan "
                         "under isin(), aggregate(join=, by=) against two projection scans, and "
                         "a two-dimension StarJoin aggregate against one join per scan")
    ap.add_argument("--join-pairs", type=int, default=15)
    ap.add_argument("--hashagg", action="store_true",
                    help="add the row GROUP BY HashBy(val), a million distinct keys, alternated "
                         "with the same aggregates without a key (--agg-pairs pairs), and "
                         "the row GROUP BY HashBy([a, b]), a million pairs of two int32 "
                         "columns, alternated with HashBy of the pairs as one int64 column")
    ap.add_argument("--topk", action="store_true",
                    help="add the ORDER BY ... LIMIT k rows: ArrowScan.top alternated with "
                         "scan_where of the same qualifier list (--topk-pairs pairs)")
    ap.add_argument("--topk-pairs", type=int, default=4)
    ap.add_argument("--expr", action="store_true",
                    help="add the computed-column row: aggregate sum(E(val) * E(x)) alternated "
                         "with aggregate sum(val), sum(x) (--agg-pairs pairs)")
    ap.add_argument("--select", action="store_true",
                    help="add the select-list row: scan_where(qual2, project=[id, x, val]) "
                         "alternated with the three single-column scans (--agg-pairs pairs)")
    ap.add_argument("--order-by", action="store_true",
                    help="add the ORDER BY row: the select query with and without "
                         "order_by=[(val, descending), x], alternated")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    import torch

    import nvme_strom_amd as S
    from nvme_strom_amd.models.arrow_scan import ArrowScan

    os.makedirs(a.dir, exist_ok=True)
    tag = "" if a.codec == "lz4" else f"_{a.codec}"
    path = os.path.join(a.dir, f"t_{a.rows}_{a.batch_rows}{tag}.arrow")
    t0 = time.time()
    make_file(path, a.rows, a.batch_rows, codec=a.codec)
    fsize = os.path.getsize(path)
    _log(f"file {fsize / 2**30:.2f} GiB ({a.rows} rows, {a.batch_rows}/batch) in "
         f"{time.time() - t0:.1f}s")
    preds = {"val": (100_000, 199_999), "x": (0.25, 0.5), "id": (1000, 5_000_000)}
    specs = [(n, [(n, *preds[n])], None) for n in a.columns.split(",") if n]
    if a.qual2:
        specs.append(("qual2", [("val", 100_000, 599_999), ("x", 0.25, 0.75)], "id"))
    res = dict(file_bytes=fsize, rows=a.rows, batch_rows=a.batch_rows, codec=("lz4_frame" if a.codec == "lz4" else "zstd") + " (pyarrow)",
               slot_mib=a.slot_mib, nslots=a.nslots, chunk_kib=a.chunk_kib, reps=a.reps, columns={})
    fd = os.open(path, os.O_RDONLY)
    cols_np = {}
    # once per process: the first scan also loads the decoder/filter code
    # objects and the host allocators' first pinned blocks; a small file
    # takes that cost so each spec's cold run is the per-file (per-query) one
    warm_path = os.path.join(a.dir, f"warmup{tag}.arrow")
    make_file(warm_path, 1 << 16, 1 << 14, seed=1, codec=a.codec)
    t1 = time.perf_counter()
    w = ArrowScan(warm_path, "cuda")
    w.scan_where([("val", 0, 1 << 40), ("x", 0.0, 1.0)], project="id")
    w.close()
    res["process_first_scan_ms"] = round((time.perf_counter() - t1) * 1e3, 2)

    def col(name):
        if name not in cols_np:
            cols_np[name] = column_np(path, name)
        return cols_np[name]

    def run(path, fd, label, quals, proj, verify):
        runs = []
        sc = None
        try:
            for r in range(a.reps):
                S.evict_file(fd)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                if sc is None:                  # cold: open + plan + allocate
                    sc = ArrowScan(path, "cuda", slot_bytes=a.slot_mib << 20, nslots=a.nslots or None,
                                   chunk_sz=(a.chunk_kib << 10) or None)
                    t_open = time.perf_counter() - t1
                out = sc.scan_where(quals, project=proj)
                dt = time.perf_counter() - t1
                runs.append(dt)
                if r == 0:
                    cold_bd = dict(open_s=round(t_open, 4),
                                   **{k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.seconds.items()})
                _log(f"{label}{' cold' if r == 0 else ''}: {out.selected} rows, "
                     f"{dt * 1e3:.1f} ms, groups {out.groups}, "
                     f"{out.column_bytes / dt / 1e9:.1f} GB/s column, {out.seconds}")
        finally:
            if sc is not None:
                sc.close()
        ok, cpu_s, cpu_n = verify(out)
        warm = runs[1:] or runs
        med = float(np.median(warm))
        row = dict(
            quals=[repr(q) for q in quals], project=proj,
            selected=out.selected, verified=ok, cpu_selected=cpu_n,
            column_bytes=out.column_bytes, bytes_read=out.bytes_read, groups=out.groups,
            ms=[round(x * 1e3, 2) for x in runs],
            cold_ms=round(runs[0] * 1e3, 2), warm_median_ms=round(med * 1e3, 2),
            column_GBps=round(out.column_bytes / med / 1e9, 2),
            column_GBps_cold=round(out.column_bytes / runs[0] / 1e9, 2),
            file_GBps=round(out.bytes_read / med / 1e9, 2),
            last_breakdown_s={k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.seconds.items()},
            cold_breakdown_s=cold_bd)
        if cpu_s == cpu_s:
            row.update(cpu_ms=round(cpu_s * 1e3, 1),
                       cpu_GBps=round(out.column_bytes / cpu_s / 1e9, 2))
        res["columns"][label] = row
        _log(json.dumps(row))

    def verify_np(quals, proj):
        def f(out):
            m = None
            for name, lo, hi in quals:
                vals, valid = col(name)
                mm = (vals >= lo) & (vals <= hi)
                if valid is not None:
                    mm &= valid
                m = mm if m is None else m & mm
            ref = np.flatnonzero(m)
            got = out.indices.cpu().numpy()
            ok = bool(len(got) == len(ref) and np.array_equal(got, ref))
            if proj is not None:
                pv, _ = col(proj)
                ok = ok and bool(np.array_equal(out.values.cpu().numpy(), pv[ref]))
            cpu_s, cpu_n = (cpu_scan(path, quals[0][0], quals[0][1], quals[0][2])
                            if len(quals) == 1 else (float("nan"), -1))
            return ok, cpu_s, cpu_n
        return f

    try:
        for label, quals, proj in specs:
            run(path, fd, label, quals, proj, verify_np(quals, proj))
        if a.agg:
            res["agg"] = agg_rows(path, fd, a, col)
        if a.join:
            res["join"] = join_rows(path, fd, a, col)
            res["join"]["star"] = star_row(path, fd, a, col)
        if a.hashagg:
            res["hashagg"] = hashagg_row(path, fd, a, col)
        if a.topk:
            res["topk"] = topk_rows(path, fd, a, col)
        if a.expr:
            res["expr"] = expr_row(path, fd, a, col)
        if a.select:
            res["select"] = select_row(path, fd, a, col)
        if a.order_by:
            res["order_by"] = order_row(path, fd, a, col)
    finally:
        os.close(fd)
    if a.hashagg:
        # GROUP BY two key columns, on a file of its own (the main one has no
        # two integer columns of few values)
        ppath = os.path.join(a.dir, f"pairs_{a.rows}_{a.batch_rows}{tag}.arrow")
        make_pairs_file(ppath, a.rows, a.batch_rows, codec=a.codec)
        res["hashagg2"] = hashagg2_row(ppath, a)
    if a.strings:
        import datetime as _dt

        from nvme_strom_amd.ops.colpred import Or, P
        spath = os.path.join(a.dir, f"s_{a.string_rows}_{a.batch_rows}{tag}.arrow")
        t0 = time.time()
        make_string_file(spath, a.string_rows, a.batch_rows, codec=a.codec)
        res["string_file_bytes"] = os.path.getsize(spath)
        res["string_rows"] = a.string_rows
        _log(f"string file {res['string_file_bytes'] / 2**30:.2f} GiB in {time.time() - t0:.1f}s")
        import pyarrow as pa
        import pyarrow.ipc as ipc
        with pa.memory_map(spath) as src:
            word = ipc.open_file(src).get_batch(0).column(1)[7].as_py()
        t1 = _dt.datetime(2024, 3, 1, tzinfo=_dt.timezone.utc)
        t2 = _dt.datetime(2024, 11, 1, tzinfo=_dt.timezone.utc)
        sspecs = [
            ("str_eq", [P("name") == word], None),
            ("str_prefix", [P("name").startswith("ab")], None),
            ("str_contains", [P("name").contains("abc")], None),
            ("str_suffix", [P("name").endswith("ab")], None),
            ("str_like", [P("name").like("a%b_c%")], None),
            ("dict_eq", [P("cat") == "cat_00042"], "sid"),
            ("dict_range", [P("cat").between("cat_00100", "cat_00199")], None),
            ("date_ts", [P("day").between(_dt.date(2020, 1, 1), _dt.date(2021, 6, 30)),
                         Or(P("ts") < t1, P("ts") >= t2)], "sid"),
        ]
        sfd = os.open(spath, os.O_RDONLY)

        def verify_pc(quals, proj):
            def f(out):
                cpu_s, ref = pc_scan(spath, quals)
                got = out.indices.cpu().numpy()
                ok = bool(np.array_equal(got, ref))
                if proj == "sid":       # sid is the row id
                    ok = ok and bool(np.array_equal(out.values.cpu().numpy(), ref))
                return ok, cpu_s, len(ref)
            return f
        try:
            for label, quals, proj in sspecs:
                run(spath, sfd, label, quals, proj, verify_pc(quals, proj))
        finally:
            os.close(sfd)
    base_rows = [res["columns"][lb] for lb, _, _ in specs]
    if base_rows:
        res["arrow_scan_GBps"] = min(c["column_GBps"] for c in base_rows)
    res["verified"] = all(c["verified"] for c in res["columns"].values()) and \
        all(r["verified"] for r in res.get("agg", {}).values()) and \
        all(r["verified"] for r in res.get("join", {}).values()) and \
        all(r["verified"] for r in res.get("topk", {}).values()) and \
        res.get("hashagg", {}).get("verified", True) and \
        res.get("hashagg2", {}).get("verified", True) and \
        res.get("expr", {}).get("verified", True) and \
        res.get("select", {}).get("verified", True)
    js = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(js)
    print(js)
    return 0 if res["verified"] else 3


if __name__ == "__main__":
    sys.exit(main())
