"""Throughput of the CDNA4 post-read kernels at production sizes.

``python -m nvme_strom_amd.tools.kbench [--gib 1] [--only crc,scatter,...]``

Each kernel runs on an HBM-resident input (default 1 GiB), timed with HIP
events over several iterations after a warm-up; GB/s counts the bytes the
kernel must read + write.  Run it under ``rocprofv3 --kernel-trace --stats``
for per-kernel device time and under ``--pmc`` for counters.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch


def timed(fn, iters=5):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters / 1e3


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--only", default="crc,scatter,verify,heap,lz4,snappy,filter",
                    help="also: mvcc (snapshot check), par (LZ4 decoders by stream count), "
                         "agg (aggregate kernels next to column_filter_i64), "
                         "join (hash-join probe next to column_filter_i64), "
                         "join_star (star probe of 2-4 legs next to the chained probes), "
                         "hashagg (hash GROUP BY next to column_filter_i64 and the LDS path), "
                         "topk (ORDER BY ... LIMIT k select + merge next to column_filter_i64), "
                         "expr (computed columns next to column_filter_i64), "
                         "like (column_qual_like: LIKE / contains / endswith next to the string "
                         "equality and prefix qualifiers, short words and long rows), "
                         "rows_multi (bitmap_to_rows_multi: a select list in one emit pass next "
                         "to the single-column emit kernels once per column), "
                         "sort (the ORDER BY radix sort next to torch.sort, 2^24 and 2^26 keys)")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    only = set(a.only.split(","))
    from nvme_strom_amd.ops import decompress as D
    from nvme_strom_amd.ops import verify as V
    from nvme_strom_amd.ops.colfilter import bitmap_to_indices, column_filter
    from nvme_strom_amd.ops.heapscan import heap_scan
    from nvme_strom_amd.ops.reorder import chunk_scatter
    from nvme_strom_amd.utils import pgpage

    n = int(a.gib * (1 << 30))
    dev = torch.device("cuda")
    res = {}

    def log(k, sec, nbytes):
        res[k] = dict(ms=round(sec * 1e3, 3), GBps=round(nbytes / sec / 1e9, 1))
        print(k, res[k], file=sys.stderr, flush=True)

    buf = torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev)
    if "crc" in only:
        for ch in (8192, 1 << 16, 1 << 20):
            out = torch.empty((n + ch - 1) // ch, dtype=torch.int32, device=dev)
            log(f"crc32c_chunks_{ch}", timed(lambda: V.crc32c_chunks(buf, ch, out=out)), n)
        log("crc32c_full", timed(lambda: V.crc32c(buf)), n)
    if "scatter" in only:
        ch = 8192
        perm = np.random.default_rng(0).permutation(n // ch).astype(np.uint32)
        dst = torch.empty_like(buf)
        pos = torch.from_numpy(perm.view(np.int32)).to(dev)
        log("chunk_scatter_8k", timed(lambda: chunk_scatter(buf, dst, pos, ch)), 2 * n)
        del dst
    if "verify" in only:
        log("verify_pattern", timed(lambda: V.verify_pattern(buf, 0x41424344)), n)
        log("fill_pattern", timed(lambda: V.fill_pattern(buf, 0x41424344)), n)
    if "heap" in only:
        page = pgpage.build_table(np.arange(150 * 64, dtype=np.int64), per_page=150, width=8)
        reps = max(1, n // len(page))
        reps = min(reps, 0xFFFF // 64)          # item ids address <= 65535 pages
        pages = torch.from_numpy(np.frombuffer(page * reps, dtype=np.uint8).copy()).to(dev)
        nb = pages.numel()
        log("heap_scan", timed(lambda: heap_scan(pages, skip_invisible=True)), nb)
        log("heap_scan_checksum_filter",
            timed(lambda: heap_scan(pages, verify_checksum=True, attr_off=0, attr_width=8,
                                    lo=100, hi=5000)), nb)
        del pages
        # tuple descriptor + qualifier lists (strom_heap_scan2): 10 columns
        # with NULLs, short / long / TOASTed text before the predicated ones
        from nvme_strom_amd.ops.heapscan import Program, heap_scan2
        from nvme_strom_amd.utils import pgtuple as T
        desc, rows = T.synthetic(4000, seed=2)
        tmpl = T.build_pages(rows, desc)
        reps = max(1, min(n // len(tmpl), 0xFFFF // (len(tmpl) // 8192)))
        pages = torch.from_numpy(np.frombuffer(tmpl * reps, dtype=np.uint8).copy()).to(dev)
        nb = pages.numel()
        for name, qs in (("heap_scan2_1qual", [T.Qual("a", "between", (-200_000, 300_000))]),
                         ("heap_scan2_2qual", [T.Qual("a", "between", (-500_000, 200_000)),
                                               T.Qual("b", "between", (0.1, 0.6))]),
                         ("heap_scan2_text_eq", [T.Qual("name", "text_eq", ("k17",))]),
                         ("heap_scan2_4qual_last_col", [T.Qual("c", "in", ([1, 2, 3],)),
                                                        T.Qual("d", "notnull"),
                                                        T.Qual("e", "between", (-0.5, 0.5)),
                                                        T.Qual("tail", "between", (0, 50))])):
            # compiled once, as a scan plan is (the program mode uploads it once)
            P = Program(desc, qs)
            log(name, timed(lambda: heap_scan2(pages, desc, P, verify_checksum=True,
                                               skip_invisible=True)), nb)
            # the same list through the program mode (device-memory CNF)
            log(name.replace("heap_scan2_", "heap_scan2_prog_"),
                timed(lambda: heap_scan2(pages, desc, P, verify_checksum=True,
                                         skip_invisible=True, program=True)), nb)
        # a CNF only the program mode takes: (a in range OR c IS NULL) AND b < 0.6
        cnf = [T.Or(T.Qual("a", "between", (-200_000, 300_000)), T.Qual("c", "isnull")),
               T.Qual("b", "lt", (0.6,))]
        P = Program(desc, cnf)
        log("heap_scan2_prog_cnf2", timed(lambda: heap_scan2(pages, desc, P, verify_checksum=True,
                                                             skip_invisible=True)), nb)
        del pages
    if "mvcc" in only:
        _mvcc_rows(n, dev, log)
    rng = np.random.default_rng(1)
    words = [b"select", b"from", b"where", b"gpu", b"hbm", b"nvme", b"strom"]
    datasets = {
        "words": b" ".join(words[i] for i in rng.integers(0, len(words), 16000))[:64 << 10],
        # sorted int64 ids (a typical columnar payload)
        "ints": np.cumsum(rng.integers(0, 5, 8192)).astype(np.int64).tobytes(),
    }
    for codec in ("lz4", "snappy"):
        if codec not in only:
            continue
        for dname, blk in datasets.items():
            comp = D.lz4_compress(blk) if codec == "lz4" else D.snappy_compress(blk)
            nblk = max(1, min(n // len(blk), 16384))
            src = torch.from_numpy(np.frombuffer(comp * nblk, dtype=np.uint8).copy()).to(dev)
            dst = torch.empty(nblk * len(blk), dtype=torch.uint8, device=dev)
            descs = D.make_descs([(i * len(comp), len(comp), i * len(blk), len(blk)) for i in range(nblk)])
            cid = D.LZ4 if codec == "lz4" else D.SNAPPY
            st = D.decompress(cid, src, dst, descs)
            assert (st == len(blk)).all(), st[:4]
            assert bytes(dst[:len(blk)].cpu().numpy()) == blk
            tag = "64k" if dname == "words" else f"{dname}_64k"
            log(f"decompress_{codec}_{tag}_ratio{len(blk) / len(comp):.1f}",
                timed(lambda: D.decompress(cid, src, dst, descs), 3), nblk * len(blk))
            if codec == "lz4" and dname == "words":
                # the same streams under each geometry (streams per wave), and
                # a few-streams launch (an Arrow scan group: ~1k buffers)
                os.environ["STROM_DECOMP_PAR"] = "0"         # lane groups only
                for g in (16, 8, 4, 1):
                    os.environ["STROM_DECOMP_G"] = str(g)
                    log(f"decompress_lz4_64k_g{g}",
                        timed(lambda: D.decompress(cid, src, dst, descs), 3), nblk * len(blk))
                os.environ.pop("STROM_DECOMP_G", None)
                os.environ.pop("STROM_DECOMP_PAR", None)
                few = min(nblk, 1024)
                log(f"decompress_lz4_64k_{few}streams",
                    timed(lambda: D.decompress(cid, src, dst, descs[:few]), 3), few * len(blk))
            del src, dst
            # 61 different blocks (stream i decodes block i mod 61): the groups
            # of a wave diverge as on real data; the rows above decode copies
            # of one block, which keeps a wave's streams in lockstep
            from nvme_strom_amd.tools.decomp_ab import corpora
            blks = [corpora(1 + k)[dname] for k in range(61)]
            comps = [D.lz4_compress(b) if codec == "lz4" else D.snappy_compress(b) for b in blks]
            offs = np.cumsum([0] + [len(c) for c in comps])
            one = b"".join(comps)
            reps = (nblk + 60) // 61
            src = torch.from_numpy(np.frombuffer(one * reps, dtype=np.uint8).copy()).to(dev)
            dst = torch.empty(nblk * len(blk), dtype=torch.uint8, device=dev)
            descs = D.make_descs([((i // 61) * len(one) + int(offs[i % 61]), len(comps[i % 61]),
                                   i * len(blk), len(blk)) for i in range(nblk)])
            st = D.decompress(cid, src, dst, descs)
            assert (st == len(blk)).all(), st[:4]
            assert bytes(dst[len(blk):2 * len(blk)].cpu().numpy()) == blks[1 % 61]
            log(f"decompress_{codec}_{tag}_distinct61",
                timed(lambda: D.decompress(cid, src, dst, descs), 3), nblk * len(blk))
            del src, dst
    if "par" in only:
        _par_rows(D, dev, log)
    if "filter" in only:
        nv = n // 8
        v = torch.randint(-1000, 1000, (nv,), dtype=torch.int64, device=dev)
        log("column_filter_i64", timed(lambda: column_filter(v, -100, 100)), nv * 8)
        bm, cnt = column_filter(v, -100, 100)
        log("bitmap_to_indices", timed(lambda: bitmap_to_indices(bm, nv, cnt)), nv // 8 + cnt * 4)
    if "agg" in only:
        _agg_rows(n, dev, log, column_filter)
    if "join" in only:
        _join_rows(n, dev, log, column_filter)
    if "join_star" in only:
        _join_star_rows(n, dev, log, column_filter)
    if "hashagg" in only:
        _hashagg_rows(n, dev, log, column_filter)
    if "topk" in only:
        _topk_rows(n, dev, log, column_filter)
    if "expr" in only:
        _expr_rows(n, dev, log, column_filter)
    if "like" in only:
        _like_rows(n, dev, log)
    if "rows_multi" in only:
        _rows_multi_rows(dev, log, res)
    if "sort" in only:
        _sort_rows(dev, res)
    js = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(js)
    print(js)


def _sort_rows(dev, res, sizes=(1 << 24, 1 << 26), reps=5, hbm_peak=8.0e12):
    """The radix sort (colsort.hip: encode + one pass per key byte) next to
    ``torch.sort(keys, stable=True)`` on the same device, alternated, ``reps``
    repetitions each, median and spread: int32 / int64 / float64 uniform
    keys, int64 already sorted and all equal, and two columns (int8 with ties,
    then float64).  The permutation is checked against torch.sort's indices
    before anything is timed.  Bytes: 36 per row and pass (key and permutation
    read by the histogram and the scatter, written once), as a share of the
    HBM peak of 8 TB/s."""
    from nvme_strom_amd.ops import colsort as SO

    def once(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / 1e3

    g = torch.Generator(device=dev)
    g.manual_seed(3)
    for n in sizes:
        u = lambda dt: torch.randint(-2**31, 2**31 - 1, (n,), dtype=dt, device=dev, generator=g)
        i64 = u(torch.int64) * 2654435761
        cases = {"i32_uniform": [u(torch.int32)], "i64_uniform": [i64],
                 "f64_uniform": [torch.randn(n, dtype=torch.float64, device=dev, generator=g)],
                 "i64_sorted": [torch.arange(n, dtype=torch.int64, device=dev)],
                 "i64_equal": [torch.full((n,), 7, dtype=torch.int64, device=dev)],
                 "i8_ties+f64": [torch.randint(0, 6, (n,), dtype=torch.int8, device=dev,
                                               generator=g),
                                 torch.randn(n, dtype=torch.float64, device=dev, generator=g)]}
        st = SO.State(n, dev)
        for name, keys in cases.items():
            cols = [(SO.TYPE_CODE[f"{'f' if k.is_floating_point() else 'i'}{k.element_size()}"],
                     k, None, False) for k in keys]

            def ours():
                st.cur, st.fresh = 0, True
                return SO.order(st, cols)

            def theirs():
                # a stable sort by the last column, then by the first
                idx = None
                for k in reversed(keys):
                    j = torch.sort(k if idx is None else k[idx], stable=True)[1]
                    idx = j if idx is None else idx[j]
                return idx
            npass = ours()
            want = theirs()
            if not torch.equal(st.order.view(torch.int32).to(torch.int64) & 0xFFFFFFFF, want):
                raise RuntimeError(f"sort {name} n={n}: the permutation differs from torch.sort's")
            del want
            ta, tb = [], []
            for _ in range(reps):
                ta.append(once(ours))
                tb.append(once(theirs))
            med = lambda t: float(np.median(t))
            moved = 36 * n * npass
            res[f"sort_{name}_n{n}"] = dict(
                passes=npass, ms=round(med(ta) * 1e3, 3),
                ms_min_max=[round(min(ta) * 1e3, 3), round(max(ta) * 1e3, 3)],
                Mrows_s=round(n / med(ta) / 1e6, 1), GBps=round(moved / med(ta) / 1e9, 1),
                hbm_peak_share=round(moved / med(ta) / hbm_peak, 3),
                torch_ms=round(med(tb) * 1e3, 3),
                torch_ms_min_max=[round(min(tb) * 1e3, 3), round(max(tb) * 1e3, 3)],
                torch_Mrows_s=round(n / med(tb) / 1e6, 1))
            print(f"sort_{name}_n{n}", res[f"sort_{name}_n{n}"], file=sys.stderr, flush=True)
        del st, cases


def _rows_multi_rows(dev, log, res, rows=1 << 25):
    """bitmap_to_rows_multi (colproject.hip: a select list in one emit pass)
    next to the single-column emit kernels of colfilter.hip
    (bitmap_to_rows with a projection, bitmap_to_rows_str), called once per
    column: 33.5M rows in one batch at 1 / 10 / 50 / 100 % selected, for one
    and four 8-byte columns, eight columns of mixed widths and a utf8 column
    of 3-24-byte words.  Every row is the median of three timings of five
    calls, the two forms alternated (``spread_ms``: the three); GB/s counts, for both forms, the bytes
    the select list must move: the bitmap, the row ids, and per column the
    selected values read and written (strings: 8 B of offsets read and
    written per row + the characters twice).  ``<set>_<pct>_ratio``: the
    single-column kernels' time over the select list's."""
    from nvme_strom_amd.ops import colproject as PJ
    from nvme_strom_amd.ops.colfilter import bitmap_to_rows, bitmap_to_rows_str
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    nw = rows // 64
    bt = torch.tensor([[0, 0, rows, 0, 0]], dtype=torch.int64, device=dev)
    shifts = torch.arange(64, dtype=torch.int64, device=dev)
    widths = {"1x8": [8], "4x8": [8] * 4, "8mixed": [1, 2, 4, 8, 16, 8, 4, 0]}   # 0: bool
    srcs = {w: torch.randint(0, 256, (rows * max(w, 1) if w else rows // 8,), dtype=torch.uint8,
                             device=dev, generator=g) for w in (1, 2, 4, 8, 16, 0)}
    lens = torch.randint(3, 25, (rows,), device=dev, generator=g)
    offs = torch.zeros(rows + 1, dtype=torch.int32, device=dev)
    offs[1:] = torch.cumsum(lens, 0).to(torch.int32)
    nch = int(offs[-1].item())
    chars = torch.randint(97, 123, (nch,), dtype=torch.uint8, device=dev, generator=g)
    del lens

    def med2(a, b):
        """The two forms alternated: (median, the three timings) of each."""
        ta, tb = [], []
        for _ in range(3):
            ta.append(timed(a))
            tb.append(timed(b))
        return [(sorted(t)[1], [round(x * 1e3, 3) for x in t]) for t in (ta, tb)]

    for pct in (1, 10, 50, 100):
        if pct == 100:
            bm = torch.full((nw,), -1, dtype=torch.int64, device=dev)
        else:
            bits = (torch.rand(rows, device=dev, generator=g) < pct / 100).view(nw, 64)
            bm = (bits.to(torch.int64) << shifts).sum(1)
            del bits
        cap = rows                                  # every output sized for every row
        out = torch.empty(cap, dtype=torch.int64, device=dev)
        cur = torch.zeros(2, dtype=torch.int64, device=dev)
        for tag, ws in list(widths.items()) + [("utf8", None)]:
            if ws is None:
                kinds = [(PJ.STR32, 0)]
                tabs = torch.tensor([[[offs.data_ptr(), 0, rows, 0, 0, chars.data_ptr(), nch]]],
                                    dtype=torch.int64, device=dev)
                outs = [torch.empty(cap + 1, dtype=torch.int64, device=dev)]
                och = torch.empty(nch, dtype=torch.uint8, device=dev)
                per_row = 16 + 2 * nch / rows
            else:
                kinds = [(PJ.BOOL, 0) if w == 0 else (PJ.FIXED, w) for w in ws]
                tabs = torch.tensor([[[srcs[w].data_ptr(), 0, rows, 0, 0, 0, 0]] for w in ws],
                                    dtype=torch.int64, device=dev)
                outs = [torch.empty(cap * max(w, 1), dtype=torch.uint8, device=dev) for w in ws]
                och = None
                per_row = sum(2 * w if w else 1.125 for w in ws)
            cols = PJ.proj_cols([(k, w, o.data_ptr(), 0, och.data_ptr() if och is not None else 0,
                                  cur[1:].data_ptr() if och is not None else 0)
                                 for (k, w), o in zip(kinds, outs)])

            def new():
                cur.zero_()                         # the outputs hold one pass
                PJ.bitmap_to_rows_multi(bm, nw, bt, out, cur[:1], cols, tabs)

            # the single form's arguments: the 5-field tables and typed outputs
            # (it has no bool projection: that column is left out of its side)
            typed = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
            singles = [(tabs[i][:, :5].contiguous(),
                        o.view(torch.int64).view(-1, 2) if w == 16 else o.view(typed[w]))
                       for i, ((k, w), o) in enumerate(zip(kinds, outs)) if k == PJ.FIXED]

            def old():
                if och is not None:
                    cur.zero_()
                    bitmap_to_rows_str(bm, nw, bt, out, cur[:1], tabs[0], 4, outs[0], och, cur[1:])
                for t5, o in singles:
                    cur.zero_()
                    bitmap_to_rows(bm, nw, bt, out, cur[:1], proj=t5, proj_out=o)
            new()
            torch.cuda.synchronize()
            sel = int(cur[0].item())
            nbytes = nw * 8 + sel * (8 + per_row)
            (t_new, sp_new), (t_old, sp_old) = med2(new, old)
            log(f"rows_multi_{tag}_{pct}", t_new, nbytes)
            log(f"rows_proj_each_{tag}_{pct}", t_old, nbytes)
            res[f"rows_multi_{tag}_{pct}"].update(spread_ms=sp_new, selected=sel)
            res[f"rows_proj_each_{tag}_{pct}"].update(spread_ms=sp_old)
            res[f"rows_multi_{tag}_{pct}_ratio"] = round(t_old / t_new, 3)
            print(f"  {tag} {pct}%: {sel} rows, single-column kernels / select list = "
                  f"{t_old / t_new:.2f}", file=sys.stderr, flush=True)
            del outs, och, tabs
        del bm, out


def _like_rows(n, dev, log):
    """column_qual_like: the LIKE kernel (collike.hip) on a utf8 column of
    short words (3-24 random letters, the vocabulary of arrow_bench's string
    file) and on one of 200-2,000-byte rows, next to the string equality and
    prefix qualifiers (colfilter.hip) on the same words.  GB/s counts the
    column's data, offsets + characters.  The long-row rows carry the
    threshold in their name: run again with STROM_LIKE_LONG_ROW set past
    every row's length for the row-per-lane path alone."""
    from nvme_strom_amd.ops import colpred as CP
    from nvme_strom_amd.utils.arrow_ipc import Column
    col = Column("name", "utf8", nbuffers=3)
    thr = os.environ.get("STROM_LIKE_LONG_ROW", "256")
    g = torch.Generator(device=dev)
    g.manual_seed(7)

    def table(lo, hi, nbytes):
        rows = int(nbytes // ((lo + hi) / 2))
        lens = torch.randint(lo, hi + 1, (rows,), device=dev, generator=g)
        offs = torch.zeros(rows + 1, dtype=torch.int32, device=dev)
        offs[1:] = torch.cumsum(lens, 0).to(torch.int32)
        nch = int(offs[-1].item())
        chars = torch.randint(97, 123, ((nch + 7) // 8 * 8,), dtype=torch.uint8, device=dev,
                              generator=g)
        qtab = torch.tensor([[offs.data_ptr(), 0, rows, 0, 0, chars.data_ptr(), nch]],
                            dtype=torch.int64, device=dev)
        return rows, nch, offs, chars, qtab

    def rows_of(tag, tab, preds):
        rows, nch, offs, chars, qtab = tab
        nw = (rows + 63) // 64
        bm = torch.empty(nw, dtype=torch.int64, device=dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        for name, p in preds:
            c = CP.compile_pred(p, col)
            cnt.zero_()
            CP.qual_batched(c, qtab, nw, bm, cnt)
            sel = int(cnt.item())
            log(f"{name}_{tag}", timed(lambda: CP.qual_batched(c, qtab, nw, bm, cnt)),
                nch + 4 * (rows + 1))
            print(f"  {name}_{tag}: {rows} rows, {nch} bytes, {sel} selected", file=sys.stderr)

    P = CP.P
    short = table(3, 24, min(n, 1 << 30) // 2)
    rows_of("words", short, [
        ("column_qual_str_eq", P("name") == "abc"),
        ("column_qual_str_prefix", P("name").startswith("ab")),
        ("column_qual_like_contains", P("name").contains("abc")),
        ("column_qual_like_suffix", P("name").endswith("ab")),
        ("column_qual_like", P("name").like("a%b_c%")),
        ("column_qual_like_head", P("name").like("ab%")),
    ])
    del short
    long_ = table(200, 2000, min(n, 1 << 30) // 2)
    rows_of(f"long_t{thr}", long_, [
        ("column_qual_str_prefix", P("name").startswith("ab")),
        ("column_qual_like_contains", P("name").contains("abcd")),
        ("column_qual_like_suffix", P("name").endswith("ab")),
        ("column_qual_like", P("name").like("a%b_c%xyz%")),
    ])


def _agg_rows(n, dev, log, column_filter):
    """The aggregate kernels (colagg.hip: the launch over the column plus the
    slab reduce) on one HBM-resident record batch, at 100 % and 10 %
    selection; GB/s of the column bytes the query reads (values, and the
    int32 keys of a grouped row), next to column_filter_i64 of the same run —
    both stream a column once.  Grouped rows: uniform keys over G slots (the
    null slot included), and one fully skewed row (every row the same key)."""
    from nvme_strom_amd.ops import colagg as A
    nv = n // 8
    v = torch.randint(-1000, 1000, (nv,), dtype=torch.int64, device=dev)
    f = torch.rand(nv, dtype=torch.float64, device=dev)
    log("column_filter_i64", timed(lambda: column_filter(v, -100, 100)), nv * 8)
    nwords = (nv + 63) // 64

    def tab(t):
        return torch.tensor([[t.data_ptr(), 0, nv, 0, 0]], dtype=torch.int64, device=dev)
    tv, tf = tab(v), tab(f)
    sels = {"100": torch.full((nwords,), -1, dtype=torch.int64, device=dev),
            "10": column_filter(v, -100, 99)[0]}

    def row(name, lay, t, key, nbytes):
        block = A.alloc_block(lay, dev)
        for tag, bm in sels.items():
            slabs = torch.empty(A.slab_words(lay, 0, nwords), dtype=torch.int64, device=dev)

            def go():
                _, k = A.agg_launch(lay, 0, block, bm, nwords, t, key, slabs)
                A.agg_reduce(lay, 0, block, slabs, k)
            log(f"{name}_sel{tag}", timed(go), nbytes)
    row("column_agg_i64_sum", A.Layout([A.Entry(A.SUM, "i8")]), tv, None, nv * 8)
    row("column_agg_f64_sum_min_max", A.Layout([A.Entry(A.SUM | A.MIN | A.MAX, "f8")]), tf, None,
        nv * 8)
    for G in (3, 256, 4096):
        k = torch.randint(0, G - 1, (nv,), dtype=torch.int32, device=dev)
        row(f"column_agg_i64_sum_by{G}", A.Layout([A.Entry(A.SUM, "i8")], G, 1), tv, tab(k),
            nv * 12)
        if G == 256:
            row(f"column_agg_f64_sum_min_max_by{G}",
                A.Layout([A.Entry(A.SUM | A.MIN | A.MAX, "f8")], G, 1), tf, tab(k), nv * 12)
        del k
    k = torch.full((nv,), 7, dtype=torch.int32, device=dev)
    row("column_agg_i64_sum_by256_skewed", A.Layout([A.Entry(A.SUM, "i8")], 256, 1), tv, tab(k),
        nv * 12)


def _join_rows(n, dev, log, column_filter):
    """The hash-join probe (coljoin.hip) alone on one HBM-resident record
    batch of int64 foreign keys, half of them keys of the table: GB/s of the
    fk bytes, next to column_filter_i64 of the same run on the same bitmap
    geometry.  Table footprints of 64 KiB, 2 MiB, 64 MiB and 1 GiB (in an
    XCD's L2, at its edge, in the Infinity Cache, in HBM) at 100 % and 1 %
    (random) source selection; the ratio to the filter row says whether the
    walk or the gather bounds the probe."""
    from nvme_strom_amd.ops import coljoin as J
    nv = n // 8
    nwords = (nv + 63) // 64
    v = torch.randint(-1000, 1000, (nv,), dtype=torch.int64, device=dev)
    log("column_filter_i64", timed(lambda: column_filter(v, -100, 100), 20), nv * 8)
    sels = {"100": torch.full((nwords,), -1, dtype=torch.int64, device=dev),
            "1": column_filter(v, -10, 9)[0]}
    del v
    dst = torch.empty(nwords, dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    for tag, nbytes in (("64KiB", 64 << 10), ("2MiB", 2 << 20), ("64MiB", 64 << 20),
                        ("1GiB", 1 << 30)):
        nk = nbytes // 32                       # 16-byte slots, capacity = 2n
        keys = torch.arange(nk, dtype=torch.int64, device=dev) * 2
        table = J.build(keys, None)
        del keys
        fk = torch.randint(0, 2 * nk, (nv,), dtype=torch.int64, device=dev)
        tab = torch.tensor([[fk.data_ptr(), 0, nv, 0, 0]], dtype=torch.int64, device=dev)
        hdr = table.header()
        assert int(hdr[J.H_NKEYS]) == nk and table.capacity * 16 == nbytes
        for sel, bm in sels.items():
            cnt.zero_()
            log(f"column_join_i64_table{tag}_sel{sel}",
                timed(lambda: J.probe(table, J.FK_CODE["i8"], tab, nwords, bm, dst, cnt), 20),
                nv * 8)
        print(f"column_join table {tag}: {nk} keys, largest displacement {int(hdr[J.H_MAXDISP])}",
              file=sys.stderr, flush=True)
        del fk, table


def _join_star_rows(n, dev, log, column_filter):
    """The star probe (strom_column_join_star: 2, 3 and 4 legs in one walk of
    the bitmap) next to the same legs as a chain of strom_column_join launches,
    the first from the source bitmap and the rest in place, over the same
    inputs in the same run: fk columns int64, int32, int64, int32 on one
    HBM-resident record batch, each leg with a table of its own that keeps
    about half of what reaches it; tables of 64 KiB and 64 MiB each; 100 % and
    1 % (random) source selection.  GB/s of the legs' fk bytes.  The two
    results are compared before they are timed."""
    from nvme_strom_amd.ops import coljoin as J
    nv = n // 8
    nwords = (nv + 63) // 64
    v = torch.randint(-1000, 1000, (nv,), dtype=torch.int64, device=dev)
    log("column_filter_i64", timed(lambda: column_filter(v, -100, 100), 20), nv * 8)
    sels = {"100": torch.full((nwords,), -1, dtype=torch.int64, device=dev),
            "1": column_filter(v, -10, 9)[0]}
    del v
    dst = torch.empty(nwords, dtype=torch.int64, device=dev)
    dst2 = torch.empty(nwords, dtype=torch.int64, device=dev)
    cnt = torch.zeros(3, dtype=torch.int64, device=dev)
    kinds = [("i8", torch.int64), ("i4", torch.int32)] * 2
    for tag, nbytes in (("64KiB", 64 << 10), ("64MiB", 64 << 20)):
        nk = nbytes // 32                       # 16-byte slots, capacity = 2n
        tables, fks = [], []
        for i, (st, dt) in enumerate(kinds):
            # every leg its own keys: the odd or the even numbers, shifted
            keys = torch.arange(nk, dtype=torch.int64, device=dev) * 2 + (i & 1)
            tables.append(J.build(keys, None))
            fks.append(torch.randint(0, 2 * nk, (nv,), dtype=dt, device=dev))
            del keys
        tabs = torch.tensor([[[f.data_ptr(), 0, nv, 0, 0]] for f in fks], dtype=torch.int64,
                            device=dev)
        for nl in (2, 3, 4):
            legs = [(tables[i], J.FK_CODE[kinds[i][0]], J.SEMI, -1) for i in range(nl)]
            nb = sum(f.element_size() for f in fks[:nl]) * nv
            for sel, bm in sels.items():
                def chain():
                    for i in range(nl):
                        # only the last launch's count is the chain's
                        J.probe(tables[i], legs[i][1], tabs[i], nwords, bm if i == 0 else dst, dst,
                                cnt[:1] if i == nl - 1 else cnt[2:])

                def star():
                    J.probe_star(legs, tabs[:nl], nwords, bm, dst2, cnt[1:2])
                cnt.zero_()
                chain()
                star()
                both = cnt.tolist()
                if both[0] != both[1] or not torch.equal(dst, dst2):
                    raise RuntimeError(f"join_star {nl} legs, table {tag}, sel {sel}: the star "
                                       f"kept {both[1]} rows, the chain {both[0]}")
                log(f"join_chain_{nl}legs_table{tag}_sel{sel}", timed(chain, 20), nb)
                log(f"join_star_{nl}legs_table{tag}_sel{sel}", timed(star, 20), nb)
        del tables, fks, tabs


def _topk_rows(n, dev, log, column_filter):
    """ORDER BY ... LIMIT k (coltopk.hip: the select launch over the column
    plus the merge of its slabs into a state that starts empty, so no
    threshold from an earlier group helps) on one HBM-resident record batch,
    ascending: GB/s of the column bytes, next to column_filter_i64 of the same
    run.  int64 and float64 keys, uniform, sorted ascending (the first rows
    win: the workgroups' own thresholds prune the rest) and sorted descending
    (every row beats what its workgroup holds: it sorts and cuts at every
    trip), k = 10, 100 and 1,024, every row selected and 1 %.  Each row's
    result is checked against torch.topk of the keys."""
    from nvme_strom_amd.ops import coltopk as T
    nv = n // 8
    nwords = (nv + 63) // 64
    v = torch.randint(-1000, 1000, (nv,), dtype=torch.int64, device=dev)
    log("column_filter_i64", timed(lambda: column_filter(v, -100, 100), 20), nv * 8)
    sels = {"100": torch.full((nwords,), -1, dtype=torch.int64, device=dev),
            "1": column_filter(v, -10, 9)[0]}
    del v
    picked = {sel: torch.from_numpy(np.unpackbits(bm.cpu().numpy().view(np.uint8),
                                                  bitorder="little")[:nv].astype(bool)).to(dev)
              for sel, bm in sels.items()}
    for st, make in (("i8", lambda: torch.randint(-2**62, 2**62, (nv,), dtype=torch.int64,
                                                  device=dev)),
                     ("f8", lambda: torch.rand(nv, dtype=torch.float64, device=dev))):
        for shape in ("uniform", "asc", "desc"):
            col = make()
            if shape != "uniform":
                col = torch.sort(col, descending=shape == "desc")[0]
            tab = torch.tensor([[col.data_ptr(), 0, nv, 0, 0]], dtype=torch.int64, device=dev)
            for k in (10, 100, 1024):
                slabs = torch.empty(T.grid(nwords, k) * T.slab_words(k), dtype=torch.int64,
                                    device=dev)
                for sel, bm in sels.items():
                    state = T.init(k, dev)

                    def go():
                        T.init(k, dev, words=state.words)
                        _, g = T.select(state, T.TYPE_CODE[st], tab, nwords, bm, slabs=slabs)
                        T.merge(state, slabs, g)
                    log(f"column_topk_{st}_{shape}_k{k}_sel{sel}", timed(go, 10), nv * 8)
                    # verify: the k smallest selected keys
                    rows, vals, _, _, _ = T.decode(T.state_entries(state.to_host()), st)
                    want = torch.topk(col[picked[sel]], k, largest=False, sorted=True)[0]
                    assert np.array_equal(vals, want.cpu().numpy()), (st, shape, k, sel)
                    assert np.array_equal(col[torch.from_numpy(rows).to(dev)].cpu().numpy(), vals)
            del col, tab


def _expr_rows(n, dev, log, column_filter):
    """Computed columns (colexpr.hip) alone on one HBM-resident record batch,
    next to column_filter_i64 of the same run: one and three source columns,
    int64 and float64, without a selection, with every word selected and with
    nine words of ten skipped.  GB/s of the bytes a launch moves: 8 per source
    row in and 8 out, for the rows of the words it evaluates.  Each row's
    result is checked against torch."""
    from nvme_strom_amd.ops import colexpr as X
    from nvme_strom_amd.utils.arrow_ipc import Column
    nv = n // 8 // 4                       # three sources and the result: n bytes in all
    nwords = (nv + 63) // 64
    v = torch.randint(-1000, 1000, (nv,), dtype=torch.int64, device=dev)
    log("column_filter_i64", timed(lambda: column_filter(v, -100, 100), 20), nv * 8)
    ints = [v, torch.randint(-1000, 1000, (nv,), dtype=torch.int64, device=dev),
            torch.randint(1, 1000, (nv,), dtype=torch.int64, device=dev)]
    flts = [torch.rand(nv, dtype=torch.float64, device=dev) for _ in range(3)]
    E = X.E
    rows = (("i64_1col", E("a") * 3 + 1, ints, lambda a, b, c: a * 3 + 1),
            ("i64_3col", E("a") * E("b") + E("c"), ints, lambda a, b, c: a * b + c),
            ("i64_3col_floor", (E("a") * E("b")) // 7 + E("c") % 5, ints,
             lambda a, b, c: torch.div(a * b, 7, rounding_mode="floor") + torch.remainder(c, 5)),
            ("f64_1col", E("a") * 0.5 + 1.0, flts, lambda a, b, c: a * 0.5 + 1.0),
            ("f64_3col", E("a") * (1.0 - E("b")) + E("c"), flts, lambda a, b, c: a * (1.0 - b) + c),
            ("f64_3col_div", E("a") / (E("b") + 1.0) - E("c"), flts,
             lambda a, b, c: a / (b + 1.0) - c))
    tenth = torch.zeros(nwords, dtype=torch.int64, device=dev)
    tenth[::10] = -1
    sels = {"none": (None, 1.0), "all": (torch.full((nwords,), -1, dtype=torch.int64, device=dev),
                                         1.0), "tenth": (tenth, 0.1)}
    out = torch.empty(nwords * 64, dtype=torch.int64, device=dev)
    okw = torch.empty(nwords, dtype=torch.int64, device=dev)
    otab = torch.tensor([[out.data_ptr(), okw.data_ptr(), nv, 0, 0]], dtype=torch.int64, device=dev)
    for name, e, cols, ref in rows:
        flt = cols is flts
        sch = [Column(c, "float" if flt else "int", 64) for c in "abc"]
        prog = X.compile_expr(e, sch)
        stab = torch.tensor([[[cols["abc".index(c)].data_ptr(), 0, nv, 0, 0]]
                             for c in prog.columns], dtype=torch.int64, device=dev)
        for tag, (sel, part) in sels.items():
            log(f"column_expr_{name}_sel{tag}",
                timed(lambda: X.expr_batched(prog, stab, nwords, otab, sel), 20),
                int(part * nv * 8 * (len(prog.columns) + 1)))
        X.expr_batched(prog, stab, nwords, otab, None)
        got = out[:nv].view(torch.float64) if flt else out[:nv]
        assert torch.equal(got, ref(*cols)), name


def _hashagg_rows(n, dev, log, column_filter):
    """Hash GROUP BY (colgroup.hip) on one HBM-resident record batch, every
    row selected, next to column_filter_i64 and column_agg_i64_sum_by256 (the
    LDS path) of the same run on the same values.  Per key column: the
    find-or-insert alone (``codes``: GB/s of the int64 keys read), and codes +
    accumulate for i64 SUM and for f64 SUM|MIN|MAX (GB/s of the key and value
    columns, 16 bytes a row; the int32 code buffer in between is not counted).
    The timed launches run on a table that already holds every key (the
    warm-up inserted them).  ``_c0`` / ``_c1``: the accumulate launch alone
    without / with the in-word combining of the first row's code.  Keys:
    uniform over 256, 64 Ki, 1 Mi and 8 Mi values, a sorted column of 64 Ki
    values, and one with every other row on one key.  ``hashagg_codes2_*``:
    the composite-key find-or-insert on two int32 columns next to the
    single-key one on the same pairs as one int64 column."""
    from nvme_strom_amd.ops import colagg as A
    from nvme_strom_amd.ops import colgroup as G
    nv = n // 8
    nwords = (nv + 63) // 64
    v = torch.randint(-1000, 1000, (nv,), dtype=torch.int64, device=dev)
    f = torch.rand(nv, dtype=torch.float64, device=dev)
    log("column_filter_i64", timed(lambda: column_filter(v, -100, 100)), nv * 8)

    def tab(t):
        return torch.tensor([[t.data_ptr(), 0, nv, 0, 0]], dtype=torch.int64, device=dev)
    tv, tf = tab(v), tab(f)
    ones = torch.full((nwords,), -1, dtype=torch.int64, device=dev)
    if nv % 64:
        ones[-1] = (1 << (nv % 64)) - 1
    k32 = torch.randint(0, 255, (nv,), dtype=torch.int32, device=dev)
    lay = A.Layout([A.Entry(A.SUM, "i8")], 256, 1)
    block = A.alloc_block(lay, dev)
    slabs = torch.empty(A.slab_words(lay, 0, nwords), dtype=torch.int64, device=dev)
    t32 = tab(k32)

    def lds():
        _, k = A.agg_launch(lay, 0, block, ones, nwords, tv, t32, slabs)
        A.agg_reduce(lay, 0, block, slabs, k)
    log("column_agg_i64_sum_by256_sel100", timed(lds), nv * 12)
    del k32, t32, slabs
    kbuf = torch.empty(nwords * 64, dtype=torch.int32, device=dev)
    ctab = tab(kbuf)
    dst = torch.empty(nwords, dtype=torch.int64, device=dev)
    ents = [A.Entry(A.SUM, "i8"), A.Entry(A.SUM | A.MIN | A.MAX, "f8")]
    vals = (tv, tf)

    def keys(tag):
        if tag == "sorted64Ki":
            return torch.sort(torch.randint(0, 1 << 16, (nv,), dtype=torch.int64, device=dev))[0]
        if tag == "skewed64Ki":
            k = torch.randint(1, 1 << 16, (nv,), dtype=torch.int64, device=dev)
            k[::2] = 0
            return k
        return torch.randint(0, int(tag), (nv,), dtype=torch.int64, device=dev)
    for tag, d in (("256", 256), ("65536", 1 << 16), ("1048576", 1 << 20), ("8388608", 1 << 23),
                   ("sorted64Ki", 1 << 16), ("skewed64Ki", 1 << 16)):
        k = keys(tag)
        tk = tab(k)
        t = G.DeviceGroups(ents, d, dev)
        name = f"uniform{tag}" if tag.isdigit() else tag

        def codes():
            G.group_codes(t, G.KEY_CODE["i8"], tk, nwords, ones, dst, ctab)
        log(f"hashagg_codes_{name}", timed(codes, 3), nv * 8)
        for e, what in enumerate(("i64_sum", "f64_sum_min_max")):
            def both(e=e):
                codes()
                G.group_agg(t, e, dst, nwords, vals[e], ctab)
            log(f"hashagg_{what}_{name}", timed(both, 3), nv * 16)
            for c in (0, 1):
                log(f"hashagg_agg_{what}_{name}_c{c}",
                    timed(lambda: G.group_agg(t, e, dst, nwords, vals[e], ctab, combine=c), 3),
                    nv * 12)
        hdr = t.header()
        print(f"hashagg {name}: capacity {int(hdr[G.H_CAPACITY])}, {int(hdr[G.H_NKEYS])} keys, "
              f"{int(hdr[G.H_OVERFLOW])} overflowed rows", file=sys.stderr, flush=True)
        del k, tk, t
    # composite keys: strom_group_codes_multi on two int32 columns next to
    # strom_group_codes on one int64 column that holds the same pairs packed
    # (a * 2^32 + b: the same distinct count, 8 key bytes a row on both
    # sides), uniform over 64 Ki and 1 Mi pairs and sorted; the two launches
    # alternate, three rounds, and each row is its fastest round
    spec = G.KeySpec([("a", "i4", None, False), ("b", "i4", None, False)])
    for tag, side in (("uniform65536", 256), ("uniform1048576", 1024), ("sorted64Ki", 256)):
        a = torch.randint(0, side, (nv,), dtype=torch.int64, device=dev)
        b = torch.randint(0, side, (nv,), dtype=torch.int64, device=dev)
        k = a * (1 << 32) + b
        if tag.startswith("sorted"):
            k = torch.sort(k)[0]
            a, b = k >> 32, k & 0xFFFFFFFF
        a32, b32 = a.to(torch.int32), b.to(torch.int32)
        del a, b
        tk = tab(k)
        tab2 = torch.stack([tab(a32), tab(b32)]).contiguous()
        t1 = G.DeviceGroups(ents[:1], side * side, dev)
        t2 = G.DeviceGroups(ents[:1], side * side, dev, spec=spec)

        def single():
            G.group_codes(t1, G.KEY_CODE["i8"], tk, nwords, ones, dst, ctab)

        def multi():
            G.group_codes_multi(t2, tab2, nwords, ones, dst, ctab)
        best = {"single": [], "multi": []}
        for _ in range(3):
            best["single"].append(timed(single, 3))
            best["multi"].append(timed(multi, 3))
        s1, s2 = min(best["single"]), min(best["multi"])
        log(f"hashagg_codes2_{tag}_single_i64", s1, nv * 8)
        log(f"hashagg_codes2_{tag}", s2, nv * 8)
        h1, h2 = t1.header(), t2.header()
        print(f"hashagg_codes2 {tag}: multi / single = {s2 / s1:.3f}; {int(h1[G.H_NKEYS])} and "
              f"{int(h2[G.H_NKEYS])} keys, {int(h2[G.H_OVERFLOW])} overflowed, "
              f"{int(h2[G.H_RANGE:].sum())} out of range", file=sys.stderr, flush=True)
        del k, tk, tab2, a32, b32, t1, t2


def _mvcc_rows(n, dev, log):
    """The heap scan's snapshot check (heapscan.hip mvcc_visible) on
    HBM-resident pages of a bulk-loaded relation (no hint bits; committed,
    aborted and running inserters, 10 % deleted: tools.pg_bench
    snapshot_template), every page checked, against the same pages with
    the check off and with the hint-bit rule; and with a qualifier list."""
    from nvme_strom_amd.ops.heapscan import DeviceMvcc, Program, heap_scan, heap_scan2
    from nvme_strom_amd.tools.pg_bench import snapshot_template
    from nvme_strom_amd.utils import pgtuple as T
    tp = 2048
    tmpl, _, snap, clog = snapshot_template(tp, 150, 1.0)
    reps = max(1, min(n // len(tmpl), 0xFFFF // tp))
    pages = torch.from_numpy(np.frombuffer(tmpl * reps, dtype=np.uint8).copy()).to(dev)
    nb = pages.numel()
    dm = DeviceMvcc(snap, clog, device=dev)
    log("heap_scan_all", timed(lambda: heap_scan(pages)), nb)
    log("heap_scan_hints", timed(lambda: heap_scan(pages, skip_invisible=True)), nb)
    log("heap_scan_mvcc", timed(lambda: heap_scan(pages, mvcc=dm)), nb)
    log("heap_scan_mvcc_filter", timed(lambda: heap_scan(pages, mvcc=dm, attr_off=0, attr_width=8,
                                                         lo=-100, hi=2500)), nb)
    desc = T.TupleDesc.of([("v", "int8")])
    P = Program(desc, [T.Qual("v", "between", (-100, 2500))])
    log("heap_scan2_mvcc_1qual", timed(lambda: heap_scan2(pages, desc, P, mvcc=dm)), nb)
    r = heap_scan(pages, mvcc=dm)
    log_counts = dict(selected=r.count, removed=r.removed, recheck=r.recheck)
    print("mvcc counts", log_counts, file=sys.stderr, flush=True)
    del pages
    # a bulk-loaded relation: one inserting transaction per page (its rows'
    # commit-log lookups hit one line), the usual shape after COPY
    tmpl, _, snap, clog = snapshot_template(tp, 150, 1.0, seed=2, page_xid=True)
    pages = torch.from_numpy(np.frombuffer(tmpl * reps, dtype=np.uint8).copy()).to(dev)
    dm = DeviceMvcc(snap, clog, device=dev)
    log("heap_scan_mvcc_page_xid", timed(lambda: heap_scan(pages, mvcc=dm)), nb)
    del pages


def _par_rows(D, dev, log):
    """Lane-group vs block-parallel (lz4par.hip) LZ4 decoder by stream
    count: 61 distinct 64 KiB blocks per corpus, and config-5-shaped streams
    (pyarrow LZ4 frames of 512 KiB, eight linked 64 KiB blocks each)."""
    from nvme_strom_amd.tools.decomp_ab import corpora

    def run(tag, cid, comps, sizes, counts):
        offs = np.cumsum([0] + [len(c) for c in comps])
        one = b"".join(comps)
        osz = np.cumsum([0] + list(sizes))
        k = len(comps)
        for cnt in counts:
            reps = (cnt + k - 1) // k
            src = torch.from_numpy(np.frombuffer(one * reps, dtype=np.uint8).copy()).to(dev)
            dst = torch.empty(int(osz[-1]) * reps, dtype=torch.uint8, device=dev)
            descs = D.make_descs([((i // k) * len(one) + int(offs[i % k]), len(comps[i % k]),
                                   (i // k) * int(osz[-1]) + int(osz[i % k]), sizes[i % k])
                                  for i in range(cnt)])
            total = sum(sizes[i % k] for i in range(cnt))
            for g in ("lanes", "par"):
                os.environ["STROM_DECOMP_PAR"] = "1" if g == "par" else "0"
                st = D.decompress(cid, src, dst, descs)
                assert (st == np.array([sizes[i % k] for i in range(cnt)])).all(), (g, st[:4])
                j = cnt - 1
                lo = (j // k) * int(osz[-1]) + int(osz[j % k])
                assert bytes(dst[lo:lo + 4096].cpu().numpy()) == corpus_out[j % k][:4096]
                log(f"{g}_{tag}_{cnt}streams",
                    timed(lambda: D.decompress(cid, src, dst, descs), 3), total)
            os.environ.pop("STROM_DECOMP_PAR", None)
            del src, dst

    for codec in ("lz4",):
        for dname in ("words", "ints"):
            corpus_out = [corpora(1 + k)[dname] for k in range(61)]
            comps = [D.lz4_compress(b) if codec == "lz4" else D.snappy_compress(b) for b in corpus_out]
            run(f"{codec}_{dname}", D.LZ4 if codec == "lz4" else D.SNAPPY, comps,
                [len(b) for b in corpus_out], (1024, 2048, 4096, 16384))
    try:
        import pyarrow as pa
    except Exception:
        return
    rng = np.random.default_rng(3)
    corpus_out = [np.cumsum(rng.integers(0, 1 << 12, 65536)).astype(np.int64).tobytes()
                  for _ in range(8)]
    frames = [pa.compress(b, codec="lz4", asbytes=True) for b in corpus_out]
    info = D.parse_lz4_frame_header(frames[0])
    comps = [f[info.data_offset:] for f in frames]
    cid = D.LZ4_FRAME_BCS if info.block_checksum else D.LZ4_FRAME
    run("frame512k_ints", cid, comps, [len(b) for b in corpus_out], (512, 2048))


if __name__ == "__main__":
    main()
