"""The hand-built heap page corpus (tests/heapcorpus.py) through the GPU
kernels: every case against its hand-written expectation and against the host
copy of the same per-tuple code; the launch geometry at every page size, for
the three evaluators with and without a snapshot; output capacity; the seeded
mutants (the bytes the sanitizer fuzz has taken on the CPU); and one relation
long enough for the second trip of the scan's grid-stride loop."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import heapcorpus as HC  # noqa: E402
from test_heapcorpus_cpu import project_as_expected, same_value  # noqa: E402

from nvme_strom_amd import _native as N  # noqa: E402
from nvme_strom_amd.ops import heapscan as H  # noqa: E402
from nvme_strom_amd.ops._util import check, lib, ptr, stream_handle  # noqa: E402
from nvme_strom_amd.utils.pgmvcc import CommitLog, Snapshot  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = {c.name: c for c in HC.CASES}
GUARD = 64
GUARD_WORD = 0x5A5A5A5A


def dev_pages(data: bytes) -> torch.Tensor:
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def sorted_items(r) -> list:
    return r.sorted_items().tolist()


def guarded_scan2(pages, desc, quals, page_sz, cap, program, **flags):
    """strom_heap_scan2 with an item list of exactly ``cap`` entries and a
    guard region behind it: (items written, total, status, recheck)."""
    npages = pages.numel() // page_sz
    items = torch.full((cap + GUARD,), GUARD_WORD, dtype=torch.int32, device=pages.device)
    cnt = torch.zeros(3, dtype=torch.int32, device=pages.device)
    status = torch.full((npages + GUARD,), GUARD_WORD, dtype=torch.int32, device=pages.device)
    g = N.HeapScan2Args()
    g.base = N.HeapScanArgs(pages=ptr(pages), npages=npages, page_sz=page_sz,
                            flags=flags.get("flags", 0), attr_off=-1, attr_width=8, lo=0, hi=0,
                            out_items=ptr(items), out_cap=cap, out_count=ptr(cnt),
                            page_status=ptr(status), blkno_base=0, blknos=None)
    g.desc = H.tupdesc_struct(desc)
    prog = H.Program(desc, quals)
    keep = None
    if program:
        keep = prog.device_arrays(pages.device, torch.cuda.current_stream())
        raw, pool = prog.arrays()
        check(lib().strom_heap_prog_check(C.byref(g.desc), np.frombuffer(raw, np.uint8).ctypes.data,
                                          len(prog.quals), pool, len(pool)), "prog_check")
        g.prog, g.cpool, g.nprog, g.cpool_len = ptr(keep[0]), ptr(keep[1]), len(prog.quals), len(pool)
    else:
        fx = prog.fixed() if prog.quals else []
        assert fx is not None
        g.nquals = len(fx)
        for i, q in enumerate(fx):
            g.quals[i] = q
    g.recheck_count = ptr(cnt) + 4
    check(lib().strom_heap_scan2(C.byref(g), stream_handle(None)), "heap_scan2")
    torch.cuda.synchronize()
    c = cnt.cpu().tolist()
    assert (items[cap:] == GUARD_WORD).all() and (status[npages:] == GUARD_WORD).all()
    n = min(c[0], cap)
    return items[:n].cpu().numpy().view(np.uint32), c[0], status[:npages].cpu().tolist(), c[1]


def guarded_scan0(pages, page_sz, cap, **pred):
    """strom_heap_scan (gen 0) with guard regions behind items and status:
    (items written, total, status)."""
    npages = pages.numel() // page_sz
    items = torch.full((cap + GUARD,), GUARD_WORD, dtype=torch.int32, device=pages.device)
    cnt = torch.zeros(1 + GUARD, dtype=torch.int32, device=pages.device)
    status = torch.full((npages + GUARD,), GUARD_WORD, dtype=torch.int32, device=pages.device)
    a = N.HeapScanArgs(pages=ptr(pages), npages=npages, page_sz=page_sz, flags=0,
                       out_items=ptr(items), out_cap=cap, out_count=ptr(cnt),
                       page_status=ptr(status), blkno_base=0, blknos=None, **pred)
    check(lib().strom_heap_scan(C.byref(a), stream_handle(None)), "heap_scan")
    torch.cuda.synchronize()
    assert (items[cap:] == GUARD_WORD).all() and (status[npages:] == GUARD_WORD).all()
    assert (cnt[1:] == 0).all()
    total = int(cnt[0])
    n = min(total, cap)
    return items[:n].cpu().numpy().view(np.uint32), total, status[:npages].cpu().tolist()


def guarded_project(pages, page_sz, items, desc, names):
    """strom_heap_project_n with values / valid of exactly [ncol][n] entries
    and a guard region behind each: {column: (values int64, valid)}."""
    n = len(items)
    ks = [desc.attno(c) for c in names]
    d_items = torch.from_numpy(np.asarray(items, dtype=np.uint32).view(np.int32).copy()).cuda()
    d_count = torch.tensor([n], dtype=torch.int32).cuda()
    vals = torch.full((len(ks) * n + GUARD,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    valid = torch.full((len(ks) * n + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    fmask = sum(1 << j for j, k in enumerate(ks) if desc.kinds[k] == "float")
    att = (C.c_int32 * len(ks))(*ks)
    d = H.tupdesc_struct(desc)
    check(lib().strom_heap_project_n(ptr(pages), page_sz, ptr(d_items), ptr(d_count), n, C.byref(d),
                                     C.addressof(att), len(ks), fmask, ptr(vals), ptr(valid),
                                     stream_handle(None)), "heap_project_n")
    torch.cuda.synchronize()
    assert (vals[len(ks) * n:] == 0x5A5A5A5A5A5A5A5A).all() and (valid[len(ks) * n:] == 0x5A).all()
    v, ok = vals[:len(ks) * n].cpu().numpy().reshape(len(ks), n), \
        valid[:len(ks) * n].cpu().numpy().reshape(len(ks), n)
    return {c: (v[j], ok[j]) for j, c in enumerate(names)}


@pytest.mark.parametrize("name", list(CASES))
def test_corpus_case(name):
    case = CASES[name]
    data = case.data
    pages = dev_pages(data)
    bl = None if case.blknos is None else torch.tensor(case.blknos, dtype=torch.int32).cuda()
    kw = dict(page_sz=case.page_sz, verify_checksum=case.verify_checksum,
              blkno_base=case.blkno_base)
    for qs, g0 in case.gen0.items():
        items, status, _ = case.expected(qs)
        r = H.heap_scan(pages, blknos=bl, **g0, **kw)
        h = H.host_scan_native(data, blknos=case.blknos, **g0, **kw)
        assert sorted_items(r) == items == h.items.tolist(), (name, qs, "gen 0")
        assert r.page_status.tolist() == status == h.page_status.tolist(), (name, qs, "gen 0")
        assert (r.count, r.total) == (len(items), len(items))
    for qs, quals in case.qsets.items():
        items, status, rechecks = case.expected(qs)
        fits = not quals or H.Program(case.desc, quals).fixed() is not None
        for program in ([True] if quals else []) + ([False] if fits else []):
            r = H.heap_scan2(pages, case.desc, quals, blknos=bl, program=program, **kw)
            h = H.host_scan2_native(data, case.desc, quals, blknos=case.blknos, program=program,
                                    **kw)
            assert sorted_items(r) == items == h.items.tolist(), (name, qs, program)
            assert r.page_status.tolist() == status == h.page_status.tolist(), (name, qs, program)
            assert (r.count, r.total, r.recheck, r.removed) == (len(items), len(items), rechecks, 0)
            assert h.recheck == rechecks
    items, cols = case.projected()
    if items:
        names = list(cols)
        d_items = torch.tensor(items, dtype=torch.int64).to(torch.int32).cuda()
        d_count = torch.tensor([len(items)], dtype=torch.int32).cuda()
        many = H.heap_project_many(pages, d_items, d_count, case.desc, names,
                                   page_sz=case.page_sz)
        host = H.host_project_native(data, items, case.desc, names, page_sz=case.page_sz)
        for c in names:
            one = H.heap_project(pages, d_items, d_count, case.desc, c, page_sz=case.page_sz)
            for got in (one, many[c]):
                v = got[0].view(torch.int64).cpu().numpy()
                ok = got[1].cpu().numpy()
                hv = host[c][0].view(np.int64)
                assert (v == hv).all() and (ok == host[c][1]).all(), (name, c, "host copy")
                if case.desc.kinds[case.desc.attno(c)] == "float":
                    v = v.view(np.float64)
                g = project_as_expected(case, data, items, c, v, ok)
                for i, (want, have) in enumerate(zip(cols[c], g)):
                    assert want[1] == have[1] and same_value(want[0], have[0]), (name, c, i)


def geometry_snapshot():
    """A snapshot that removes some of the geometry relations' tuples (those
    without the xmin-committed hint: xmin 2 is frozen, so make it the hint
    bits' job) — and, on pages the check covers, nothing else."""
    clog = CommitLog(256)
    return Snapshot(xmin=100, xmax=200, xip=[150]), clog


@pytest.mark.parametrize("page_sz", HC.PAGE_SIZES)
def test_geometry_relations(page_sz):
    """npages around the pages-per-workgroup share, all three evaluators,
    with and without a snapshot, and the projection."""
    _, ppw = H.scan_geometry(page_sz, 1)
    share = 4 * ppw
    sizes = set(HC.GEOMETRY_NPAGES)
    if page_sz == 32768:
        sizes |= {share - 1, share, share + 1}
    snap, clog = geometry_snapshot()
    dm, hm = H.DeviceMvcc(snap, clog), H.DeviceMvcc(snap, clog, device="cpu")
    for npages in sorted(sizes):
        data, desc, quals, g0 = HC.geometry_relation(npages, page_sz)
        assert H.Program(desc, quals).fixed() is not None      # program=False is gen 1
        pages = dev_pages(data)
        for mv_d, mv_h in ((None, None), (dm, hm)):
            kw = dict(page_sz=page_sz, verify_checksum=True)
            r = H.heap_scan(pages, mvcc=mv_d, **g0, **kw)
            h = H.host_scan_native(data, mvcc=mv_h, **g0, **kw)
            assert sorted_items(r) == h.items.tolist() and r.total == h.total
            assert r.page_status.tolist() == h.page_status.tolist()
            assert (r.removed, r.recheck) == (h.removed, h.recheck)
            for program in (False, True):
                r = H.heap_scan2(pages, desc, quals, program=program, mvcc=mv_d, **kw)
                h = H.host_scan2_native(data, desc, quals, program=program, mvcc=mv_h, **kw)
                assert sorted_items(r) == h.items.tolist() and r.total == h.total
                assert r.page_status.tolist() == h.page_status.tolist()
                assert (r.removed, r.recheck) == (h.removed, h.recheck)
                if mv_d is not None:
                    assert h.removed > 0 or npages < 8
        # the projection of everything the last scan kept
        its = np.sort(r.items[:r.count].cpu().numpy().view(np.uint32))
        if not len(its):
            continue                     # an empty tensor has no address to pass
        d_items = torch.from_numpy(its.view(np.int32).copy()).cuda()
        d_count = torch.tensor([len(its)], dtype=torch.int32).cuda()
        got = H.heap_project_many(pages, d_items, d_count, desc, ["id", "v", "t"], page_sz=page_sz)
        host = H.host_project_native(data, its, desc, ["id", "v", "t"], page_sz=page_sz)
        for c in ("id", "v", "t"):
            assert (got[c][0].cpu().numpy() == host[c][0]).all()
            assert (got[c][1].cpu().numpy() == host[c][1]).all()


def test_out_cap():
    """A short item list: a subset of the expected items of size min(cap,
    count), the total still the full count, nothing written behind the list."""
    data, desc, quals, g0 = HC.geometry_relation(33, 8192)
    pages = dev_pages(data)
    full = H.host_scan2_native(data, desc, quals)
    want, count = set(full.items.tolist()), full.total
    assert count > 8
    for program in (False, True):
        for cap in (0, 1, count - 1, count):
            items, total, status, _ = guarded_scan2(pages, desc, quals, 8192, cap, program)
            assert total == count and len(items) == min(cap, count)
            assert len(set(items.tolist())) == len(items) and set(items.tolist()) <= want
            assert status == full.page_status.tolist()
            r = H.heap_scan2(pages, desc, quals, out_cap=cap, program=program)
            assert (r.count, r.total, r.truncated) == (min(cap, count), count, cap < count)
    r = H.heap_scan(pages, out_cap=3, **g0)
    h = H.host_scan_native(data, **g0)
    assert (r.count, r.total) == (3, h.total) and set(sorted_items(r)) <= set(h.items.tolist())


def test_mutants_kernel_equals_host_copy():
    """The seeded mutants — the bytes the sanitizer fuzz runs the host copy
    over — through the kernels: items, status and rechecks equal the host
    copy's, for every qualifier set of the page's case, and so does the
    projection of every column."""
    by_case = {}
    for pg, sz, name in HC.mutants():
        by_case.setdefault(name, []).append(pg)
    assert sum(len(v) for v in by_case.values()) == 400
    for name, pgs in by_case.items():
        case = CASES[name]
        data = b"".join(pgs)
        pages = dev_pages(data)
        cap = len(pgs) * ((8192 - 24) // 4)
        kept = None
        for qs, quals in case.qsets.items():
            fits = not quals or H.Program(case.desc, quals).fixed() is not None
            for program in ([True] if quals else []) + ([False] if fits else []):
                items, total, status, recheck = guarded_scan2(pages, case.desc, quals, 8192, cap,
                                                              program)
                h = H.host_scan2_native(data, case.desc, quals, program=program)
                assert np.sort(items).tolist() == h.items.tolist(), (name, qs, program)
                assert (total, status, recheck) == (h.total, h.page_status.tolist(), h.recheck)
                if not quals:
                    kept = h.items
        g0 = dict(attr_off=0, attr_width=4, lo=0, hi=1000)
        items, total, status = guarded_scan0(pages, 8192, cap, **g0)
        h0 = H.host_scan_native(data, **g0)
        assert np.sort(items).tolist() == h0.items.tolist() and total == h0.total
        assert status == h0.page_status.tolist()
        if kept is not None and len(kept):
            names = [c for c, L in zip(case.desc.names, case.desc.attlen) if L < 0 or L in (1, 2, 4, 8)]
            got = guarded_project(pages, 8192, kept, case.desc, names)
            host = H.host_project_native(data, kept, case.desc, names)
            for c in names:
                assert (got[c][0] == host[c][0].view(np.int64)).all(), (name, c)
                assert (got[c][1] == host[c][1]).all(), (name, c)


def test_second_grid_stride_trip():
    """More 8 KiB pages than one trip of the grid covers: first + stride, the
    prefetch across the trip and the reuse of the masks after the barrier.  A
    64-page block tiled on the device; blknos repeats the block's numbers, so
    the checksums verify; the expectation is the block's, replicated."""
    grid, ppw = H.scan_geometry(8192, 65535)
    npages = grid * 4 * ppw + 4 * ppw + 5
    assert grid * 4 * ppw < npages <= 65535
    data, desc, quals, g0 = HC.geometry_relation(64, 8192)
    block = dev_pages(data)
    reps = (npages + 63) // 64
    pages = block.repeat(reps)[:npages * 8192].contiguous()
    blknos = (torch.arange(npages, dtype=torch.int32, device="cuda") % 64).contiguous()
    pg = np.arange(npages, dtype=np.int64)

    def replicated(h):
        per = [[] for _ in range(64)]
        for it in h.items.tolist():
            per[it >> 16].append(it & 0xFFFF)
        out = [((pg[p::64, None] << 16) | np.array(l, dtype=np.int64)[None, :]).reshape(-1)
               for p, l in enumerate(per) if l]
        return np.sort(np.concatenate(out)), np.array(h.page_status.tolist())[pg % 64]

    for program in (False, True):
        h = H.host_scan2_native(data, desc, quals, verify_checksum=True, program=program)
        want, status = replicated(h)
        r = H.heap_scan2(pages, desc, quals, verify_checksum=True, blknos=blknos, program=program)
        assert r.total == len(want) == r.count
        assert (r.sorted_items().astype(np.int64) == want).all()
        assert (r.page_status.cpu().numpy() == status).all()
    h = H.host_scan_native(data, verify_checksum=True, **g0)
    want, status = replicated(h)
    r = H.heap_scan(pages, verify_checksum=True, blknos=blknos, **g0)
    assert r.total == len(want) and (r.sorted_items().astype(np.int64) == want).all()
    assert (r.page_status.cpu().numpy() == status).all()
