"""The hand-built heap page corpus (tests/heapcorpus.py) on the CPU: for every
case the hand-written expectation, the Python model, and the native host copy
of the kernels' per-tuple code (gen 1 where the qualifier list fits the fixed
AND list, gen 2 always, gen 0 against utils.pgpage.host_scan) must be exactly
equal.  Then the sanitizer fuzz of the host copy over the corpus pages and
their mutants (csrc/tests/heapscan_fuzz.cc)."""
import math
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import heapcorpus as HC  # noqa: E402

from nvme_strom_amd import _native as N  # noqa: E402
from nvme_strom_amd.ops import heapscan as H  # noqa: E402
from nvme_strom_amd.utils import pgpage as P  # noqa: E402
from nvme_strom_amd.utils import pgtuple as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c.name: c for c in HC.CASES}


def same_value(a, b) -> bool:
    if isinstance(a, float) and isinstance(b, float):
        return struct.pack("<d", a) == struct.pack("<d", b) or (math.isnan(a) and math.isnan(b))
    return a == b


def project_as_expected(case, data: bytes, items, col, values, valid):
    """The (values, valid) arrays of a projection in the corpus' terms."""
    k = case.desc.attno(col)
    out = []
    for v, ok in zip(values.tolist(), valid.tolist()):
        if ok == 0:
            out.append((0, 0))
        elif case.desc.attlen[k] < 0:
            o, n = (v >> 32) & 0xFFFFFFFF, v & 0xFFFFFFFF
            out.append((data[o:o + n], 1) if ok == 1 else (n, 2))
        else:
            out.append((v, ok))
    return out


def model_project(case, items, cols):
    """utils.pgtuple.project_tuple over ``items`` in the corpus' terms."""
    data, sz = case.data, case.page_sz
    out = {c: [] for c in cols}
    ks = [case.desc.attno(c) for c in cols]
    for it in items:
        pg, ln = it >> 16, it & 0xFFFF
        at = P.line_pointer(data[pg * sz:(pg + 1) * sz], ln, sz)
        if at is None:                       # the item names no tuple: NULLs
            for c in cols:
                out[c].append((0, 0))
            continue
        tup = data[pg * sz + at[0]:pg * sz + at[0] + at[1]]
        for c, k, (v, ok) in zip(cols, ks, T.project_tuple(tup, case.desc, ks)):
            if ok and case.desc.attlen[k] < 0:
                v = tup[v[0]:v[0] + v[1]] if ok == 1 else v[1]
            out[c].append((v, ok))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_corpus_case(name):
    case = CASES[name]
    data = case.data
    kw = dict(page_sz=case.page_sz, verify_checksum=case.verify_checksum,
              blkno_base=case.blkno_base, blknos=case.blknos)
    for qs, quals in case.qsets.items():
        items, status, rechecks = case.expected(qs)
        m_items, m_status, _ = T.host_scan2(data, case.desc, quals, **kw)
        assert (m_items, m_status) == (items, status), (name, qs, "model")
        prog = H.Program(case.desc, quals)
        modes = [True] if quals else []
        if not quals or prog.fixed() is not None:
            modes.append(False)
        for program in modes:
            r = H.host_scan2_native(data, case.desc, quals, program=program, **kw)
            assert r.items.tolist() == items, (name, qs, "host copy", program)
            assert r.page_status.tolist() == status, (name, qs, "host copy", program)
            assert (r.count, r.total, r.recheck) == (len(items), len(items), rechecks)
    for qs, g0 in case.gen0.items():
        items, status, _ = case.expected(qs)
        m = P.host_scan(data, attr_width=g0.get("attr_width", 4), attr_off=g0.get("attr_off", -1),
                        lo=g0.get("lo", -(1 << 63)), hi=g0.get("hi", (1 << 63) - 1), **kw)
        assert m == (items, status), (name, qs, "pgpage.host_scan")
        r = H.host_scan_native(data, **g0, **kw)
        assert (r.items.tolist(), r.page_status.tolist()) == (items, status), (name, qs, "gen 0")
    items, cols = case.projected()
    if items:
        names = list(cols)
        got = H.host_project_native(data, items, case.desc, names, page_sz=case.page_sz)
        model = model_project(case, items, names)
        for c in names:
            g = project_as_expected(case, data, items, c, *got[c])
            for i, (want, have, mod) in enumerate(zip(cols[c], g, model[c])):
                assert want[1] == have[1] and same_value(want[0], have[0]), (name, c, i, want, have)
                assert want[1] == mod[1] and same_value(want[0], mod[0]), (name, c, i, want, mod)


def test_corpus_covers_each_outcome():
    """Keep, drop and recheck all occur, and every page status."""
    seen, stat = set(), set()
    for c in HC.CASES:
        stat.update(c.status)
        for tl in c.tups:
            for t in tl:
                seen.update(t.expect.values())
    assert seen == {"K", "D", "R"} and stat == {0, HC.BAD_HEADER, HC.BAD_CHECKSUM, HC.EMPTY}


def test_geometry_export_matches_page_sizes():
    """One trip of an 8 KiB scan is 49,152 pages; 32 KiB pages leave LDS for
    fewer pages per wave."""
    grid, ppw = H.scan_geometry(8192, 65535)
    assert (grid, ppw, grid * 4 * ppw) == (1536, 8, 49152)
    g32, p32 = H.scan_geometry(32768, 65535)
    assert 1 <= p32 < 8 and g32 >= 256
    assert H.scan_geometry(8192, 9) == (1, 8) and H.scan_geometry(8192, 33) == (2, 8)
    rc = N.lib().strom_heap_scan_geometry(1000, 1, None, None)
    assert rc == -22


@pytest.mark.parametrize("page_sz", HC.PAGE_SIZES)
def test_geometry_relations_model_vs_host_copy(page_sz):
    kept = kept0 = 0
    for npages in HC.GEOMETRY_NPAGES:
        data, desc, quals, g0 = HC.geometry_relation(npages, page_sz)
        m = T.host_scan2(data, desc, quals, page_sz=page_sz, verify_checksum=True,
                         skip_invisible=True)
        for program in (False, True):
            r = H.host_scan2_native(data, desc, quals, page_sz=page_sz, verify_checksum=True,
                                    skip_invisible=True, program=program)
            assert (r.items.tolist(), r.page_status.tolist()) == (m[0], m[1])
        m0 = P.host_scan(data, page_sz, True, verify_checksum=True, **g0)
        r0 = H.host_scan_native(data, page_sz, verify_checksum=True, skip_invisible=True, **g0)
        assert (r0.items.tolist(), r0.page_status.tolist()) == m0
        kept, kept0 = kept + len(m[0]), kept0 + len(m0[0])
    assert kept and kept0


def test_out_cap_host_copy():
    data, desc, quals, _ = HC.geometry_relation(9, 8192)
    full = H.host_scan2_native(data, desc, quals)
    for cap in (0, 1, full.total - 1, full.total):
        r = H.host_scan2_native(data, desc, quals, out_cap=cap)
        assert (r.total, r.count) == (full.total, min(cap, full.total))
        assert r.items.tolist() == full.items.tolist()[:r.count]


def write_fuzz_input(path, nmutants: int = 400):
    """The fuzz program's input: the corpus pages and mutants(), each with its
    descriptor and the case's compiled qualifier sets.

    u32 magic, u32 nrecords; per record: u32 page_sz, u32 npages, u32 mutant, the pages,
    strom_heap_tupdesc, u32 nsets; per set: u32 nfixed (0xFFFFFFFF: none),
    8 strom_heap_qual, u32 nprog, the program, u32 pool bytes, the pool."""
    recs = []
    sets_of = {}
    for c in HC.CASES:
        if c.desc is None:
            continue
        sets = []
        for quals in c.qsets.values():
            prog = H.Program(c.desc, quals)
            fx = prog.fixed() if prog.quals else []
            raw, pool = prog.arrays()
            fixed = b"".join(bytes(q) for q in (fx or []))
            fixed += b"\0" * (C_SIZEOF_QUAL * N.HEAP_MAX_QUALS - len(fixed))
            sets.append(struct.pack("<I", 0xFFFFFFFF if fx is None else len(fx)) + fixed +
                        struct.pack("<I", len(prog.quals)) + raw +
                        struct.pack("<I", len(pool)) + pool)
        sets_of[c.name] = (bytes(H.tupdesc_struct(c.desc)), sets)
        recs.append((c.page_sz, c.pages, c.name, 0))
    for pg, sz, name in HC.mutants(n=nmutants):
        recs.append((sz, [pg], name, 1))
    with open(path, "wb") as f:
        f.write(struct.pack("<II", 0x50414548, len(recs)))
        for sz, pages, name, mutant in recs:
            d, sets = sets_of[name]
            f.write(struct.pack("<III", sz, len(pages), mutant) + b"".join(pages) + d +
                    struct.pack("<I", len(sets)) + b"".join(sets))
    return len(recs)


C_SIZEOF_QUAL = 56


def test_mutants_mostly_pass_the_header_check():
    """At least half of the mutated pages still reach the tuple code."""
    mut = HC.mutants()
    assert len(mut) == 400 and mut == HC.mutants()          # fixed and seeded
    ok = sum(P.host_scan(pg, sz)[1][0] == 0 for pg, sz, _ in mut)
    assert 2 * ok >= len(mut), ok


def test_heapscan_fuzz_asan(tmp_path):
    """The host copy under ASan + UBSan, as a stand-alone child process."""
    import ctypes
    assert ctypes.sizeof(N.HeapQual) == C_SIZEOF_QUAL
    subprocess.run(["make", "build/heapscan_fuzz"], cwd=ROOT, check=True, capture_output=True)
    path = tmp_path / "heapfuzz.bin"
    write_fuzz_input(path)
    p = subprocess.run([os.path.join(ROOT, "build", "heapscan_fuzz"), str(path), "50"],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    m = re.search(r"pages accepted (\d+) rejected (\d+), tuples kept (\d+) dropped (\d+) "
                  r"rechecked (\d+), projected (\d+); mutated pages (\d+) accepted (\d+)", p.stdout)
    assert m, p.stdout
    counts = list(map(int, m.groups()))
    assert all(counts), p.stdout
    assert 2 * counts[7] >= counts[6], p.stdout
