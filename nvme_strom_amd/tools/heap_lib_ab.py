"""strom_heap_scan of two builds of libstrom in ONE process, on the same pages
and outputs, launches alternating: the kernel's time without the Python
wrapper, its allocations and its device sync (kbench's heap rows include them).

  python -m nvme_strom_amd.tools.heap_lib_ab --a OTHER/libstrom.so [--b LIB] [--out FILE]

``--b`` defaults to this tree's library.  Rows: every tuple kept (kbench's
heap_scan_all) and the hint-bit rule (heap_scan_hints) over the snapshot
relation of tools.pg_bench, 8 KiB pages."""
from __future__ import annotations

import argparse
import ctypes as C
import json

import numpy as np
import torch

from .. import _native as N
from .pg_bench import snapshot_template


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", required=True, help="the other build's libstrom.so")
    ap.add_argument("--b", default=N.LIB_PATH)
    ap.add_argument("--samples", type=int, default=12)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    libs = {"a": C.CDLL(a.a), "b": C.CDLL(a.b)}
    for l in libs.values():
        l.strom_heap_scan.restype = C.c_int
        l.strom_heap_scan.argtypes = [C.POINTER(N.HeapScanArgs), C.c_void_p]
    tp = 2048
    tmpl, _, _, _ = snapshot_template(tp, 150, 1.0)
    reps = min((1 << 30) // len(tmpl), 0xFFFF // tp)
    pages = torch.from_numpy(np.frombuffer(tmpl * reps, dtype=np.uint8).copy()).cuda()
    npages = pages.numel() // 8192
    cap = npages * (8192 // 28 + 1)
    items = torch.empty(cap, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(3, dtype=torch.int32, device="cuda")
    status = torch.empty(npages, dtype=torch.int32, device="cuda")
    st = int(torch.cuda.current_stream().cuda_stream)
    rows = {}
    for name, flags in (("all", 0), ("hints", 2)):
        args = N.HeapScanArgs(pages=pages.data_ptr(), npages=npages, page_sz=8192, flags=flags,
                              attr_off=-1, attr_width=4, lo=0, hi=0, out_items=items.data_ptr(),
                              out_cap=cap, out_count=cnt.data_ptr(),
                              page_status=status.data_ptr(), blkno_base=0, blknos=None)
        res = {"a": [], "b": []}
        for rnd in range(a.samples):
            for k in (("a", "b") if rnd % 2 == 0 else ("b", "a")):
                fn = libs[k].strom_heap_scan
                for _ in range(5):
                    if fn(C.byref(args), st):
                        raise RuntimeError("strom_heap_scan failed")
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(a.launches):
                    fn(C.byref(args), st)
                e.record()
                torch.cuda.synchronize()
                res[k].append(round(s.elapsed_time(e) / a.launches * 1e3, 2))
        rows[name] = res
        print(name, "count", int(cnt[0]),
              {k: (min(v), sorted(v)[len(v) // 2], max(v)) for k, v in res.items()}, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"unit": "us per strom_heap_scan launch", "launches_per_sample": a.launches,
                       "bytes": int(pages.numel()), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
