"""A hand-built corpus of PostgreSQL heap pages for the heap scan kernels.

Every page here is assembled from raw fields — page header words, line
pointers (off, flags, len), tuple header fields (natts, infomask, hoff), the
null bitmap and attribute storage as literal bytes — so that a case can be
wrong on purpose, and every case carries its expectation WRITTEN BY HAND: the
page status, per tuple and qualifier set keep / drop / recheck ("K" / "D" /
"R"), and per projected column (value, valid).  No model computes them; the
tests hold the kernels, their host copy (strom_heap_scan2_host) and the Python
models (utils.pgpage.host_scan, utils.pgtuple.host_scan2) against them.

``mutants(seed, n)`` derives a fixed, seeded list of damaged pages from the
corpus pages for the sanitizer fuzz (csrc/tests/heapscan_fuzz.cc) and for the
kernel-against-host-copy test.
"""
from __future__ import annotations

import math
import struct
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from nvme_strom_amd.utils import pgpage as P
from nvme_strom_amd.utils import pgtuple as T

VIS = P.VISIBLE                    # xmin committed, xmax invalid
HASNULL = 0x0001
BAD_HEADER, BAD_CHECKSUM, EMPTY, RECHECK = 1, 2, 4, 8
Q, Or = T.Qual, T.Or


def lp_word(off: int, flags: int, length: int) -> int:
    return (off & 0x7FFF) | ((flags & 3) << 15) | ((length & 0x7FFF) << 17)


def tuple_raw(data: bytes = b"", natts: int = 1, infomask: int = VIS, hoff: int = 24,
              bits: bytes = b"", xmin: int = 2, xmax: int = 0) -> bytes:
    """A tuple from its raw fields: the 23-byte header, ``bits`` right behind
    it, zeroes up to ``hoff`` (when hoff lies behind them), then ``data``."""
    hdr = struct.pack("<IIIHHHHHB", xmin, xmax, 0, 0, 0, 0, natts & 0x7FF, infomask, hoff & 0xFF)
    body = hdr + bits
    body += b"\0" * max(0, hoff - len(body))
    return body + data


@dataclass
class Tup:
    """One line pointer and (usually) its tuple.  ``raw``: the tuple's bytes;
    ``flags`` / ``len`` / ``off``: the line pointer's fields (len defaults to
    len(raw), off to where the builder put the tuple: 8-aligned, from the
    page's end downwards).  ``expect``: qualifier set name -> "K" keep, "D"
    drop, "R" recheck.  ``proj``: column -> (value, valid); for a varlena or
    cstring column the value is the data bytes (valid 1) or the stored length
    behind the header (valid 2).  A tuple with ``proj`` is projected."""
    raw: bytes = b""
    expect: Dict[str, str] = field(default_factory=dict)
    proj: Optional[Dict[str, Tuple[Any, int]]] = None
    flags: int = 1
    len: Optional[int] = None
    off: Optional[int] = None
    same_as: Optional[int] = None        # a second pointer to tuple number same_as
    note: str = ""


@dataclass
class Case:
    name: str
    desc: Optional[T.TupleDesc]
    pages: List[bytes]
    tups: List[List[Tup]]                # per page, per line pointer
    status: List[int]                    # per page, without RECHECK
    qsets: Dict[str, list]               # name -> qualifier list (gen 1 where it fits, gen 2 always)
    page_sz: int = 8192
    verify_checksum: bool = False
    blkno_base: int = 0
    blknos: Optional[List[int]] = None
    # gen 0 (strom_heap_scan): name -> dict(attr_off, attr_width, lo, hi, skip_invisible)
    gen0: Dict[str, dict] = field(default_factory=dict)

    @property
    def data(self) -> bytes:
        return b"".join(self.pages)

    def expected(self, qs: str):
        """(items ascending, per-page status, rechecks) of qualifier set qs."""
        items, status, rechecks = [], [], 0
        for pg, (tl, st) in enumerate(zip(self.tups, self.status)):
            if st == 0:
                for i, t in enumerate(tl):
                    e = t.expect[qs]
                    assert e in ("K", "D", "R"), (self.name, qs, e)
                    if e == "K":
                        items.append((pg << 16) | (i + 1))
                    elif e == "R":
                        st |= RECHECK
                        rechecks += 1
            status.append(st)
        return items, status, rechecks

    def projected(self):
        """(items, {column: [(value, valid)...]}) of the tuples with ``proj``
        on accepted pages (a scan names no item of a rejected page)."""
        items, cols = [], {}
        for pg, tl in enumerate(self.tups):
            if self.status[pg]:
                continue
            for i, t in enumerate(tl):
                if t.proj is not None:
                    items.append((pg << 16) | (i + 1))
                    for c, v in t.proj.items():
                        cols.setdefault(c, []).append(v)
        assert all(len(v) == len(items) for v in cols.values()), self.name
        return items, cols


def build_page(tups: Sequence[Tup], page_sz: int = 8192, blkno: int = 0, checksum: bool = True,
               lower: Optional[int] = None, upper: Optional[int] = None,
               special: Optional[int] = None, flags: int = 0, psv: Optional[int] = None,
               fill: bytes = b"") -> bytes:
    """A page from line pointers and tuples; every header word can be
    overridden.  ``fill``: bytes written from offset 24 first (the line
    pointers go over them)."""
    page = bytearray(page_sz)
    page[24:24 + len(fill)] = fill
    at = page_sz
    offs: List[int] = []
    words = []
    for t in tups:
        if t.same_as is not None:
            off = offs[t.same_as]
        elif t.off is not None:
            off = t.off
            if t.raw and off + len(t.raw) <= page_sz:
                page[off:off + len(t.raw)] = t.raw
        else:
            at = (at - len(t.raw)) & ~7
            off = at
            page[off:off + len(t.raw)] = t.raw
        offs.append(off)
        words.append(lp_word(off, t.flags, len(t.raw) if t.len is None else t.len))
    for i, w in enumerate(words):
        struct.pack_into("<I", page, 24 + 4 * i, w)
    lo = 24 + 4 * len(words) if lower is None else lower
    up = at if upper is None else upper
    sp = page_sz if special is None else special
    ps = ((page_sz & 0xFF00) | 4) if psv is None else psv
    struct.pack_into("<QHHHHHHI", page, 0, 1, 0, flags, lo, up, sp & 0xFFFF, ps, 0)
    if checksum:
        struct.pack_into("<H", page, 8, P.checksum(bytes(page), blkno))
    return bytes(page)


# ------------------------------------------------------------ literal values
def i2(v): return struct.pack("<h", v)
def i4(v): return struct.pack("<i", v)
def i8(v): return struct.pack("<q", v)
def f4(v): return struct.pack("<f", v)
def f8(v): return struct.pack("<d", v)
def short(b: bytes) -> bytes:           # 1-byte varlena header
    return bytes([((len(b) + 1) << 1) | 1]) + b
def long4(b: bytes, flag: int = 0) -> bytes:   # 4-byte varlena header (flag 2: compressed)
    return struct.pack("<I", ((len(b) + 4) << 2) | flag) + b
def toast(tag: int = 18, n: Optional[int] = None) -> bytes:
    size = {18: 16, 1: 8, 2: 8, 3: 8}.get(tag, 16) if n is None else n
    return bytes([1, tag]) + bytes(range(0x40, 0x40 + size))
def digits(*d): return struct.pack(f"<{len(d)}h", *d)
def num_short(weight: int, d: Sequence[int], neg: bool = False, dscale: int = 0) -> bytes:
    return struct.pack("<H", 0x8000 | (0x2000 if neg else 0) | ((dscale & 0x3F) << 7) |
                       (0x40 if weight < 0 else 0) | (weight & 0x3F)) + digits(*d)
def num_long(weight: int, d: Sequence[int], neg: bool = False, dscale: int = 0) -> bytes:
    return struct.pack("<Hh", (0x4000 if neg else 0) | (dscale & 0x3FFF), weight) + digits(*d)


CASES: List[Case] = []


def _case(name, desc, pages_tups, qsets, status=None, page_sz=8192, page_kw=None, **kw):
    """A case of pages built from Tup lists (page_kw: per-page build_page
    overrides)."""
    page_kw = page_kw or [{} for _ in pages_tups]
    base = kw.get("blkno_base", 0)
    bl = kw.get("blknos")
    pages = [build_page(tl, page_sz, blkno=(bl[i] if bl else base + i), **page_kw[i])
             for i, tl in enumerate(pages_tups)]
    c = Case(name, desc, pages, [list(t) for t in pages_tups],
             status if status is not None else [0] * len(pages), qsets, page_sz, **kw)
    CASES.append(c)
    return c


# ====================================================================== pages
D1 = T.TupleDesc.of([("a", "int4")])
_ONE = lambda: [Tup(tuple_raw(i4(5)), {"all": "K", "a5": "K", "a6": "D"}, {"a": (5, 1)})]
_Q1 = {"all": [], "a5": [Q("a", "eq", (5,))], "a6": [Q("a", "eq", (6,))]}
_G0 = {"all": dict(), "a5": dict(attr_off=0, attr_width=4, lo=5, hi=5),
       "a6": dict(attr_off=0, attr_width=4, lo=6, hi=6)}


def _hdr_case(name, st, **page_kw):
    _case("hdr/" + name, D1, [_ONE()], _Q1, status=[st], page_kw=[page_kw], gen0=_G0)


_hdr_case("good", 0)
_hdr_case("upper0_empty", EMPTY, upper=0)                  # pd_upper == 0: a new page, whatever else is set
_hdr_case("lower_below_header", BAD_HEADER, lower=20)
_hdr_case("lower_above_upper", BAD_HEADER, lower=8168, upper=8160)
_hdr_case("upper_above_special", BAD_HEADER, special=8152)  # the tuple sits at 8160
_hdr_case("special_above_page", BAD_HEADER, special=8200)
_hdr_case("special_unaligned", BAD_HEADER, special=8188)
_hdr_case("unknown_flag", BAD_HEADER, flags=0x0008)
_hdr_case("known_flags", 0, flags=0x0003)                  # PD_HAS_FREE_LINES | PD_PAGE_FULL
_hdr_case("pagesize_byte_wrong", BAD_HEADER, psv=0x1004)
_hdr_case("version_other", 0, psv=0x2005)                  # only the size byte is compared
_c = _case("hdr/lower24", D1, [[]], _Q1, page_kw=[dict(lower=24, upper=8192)], gen0=_G0)
# pd_lower 26 and 27: (lower - 24) / 4 floors to no line pointer; 28..31 to one
_case("hdr/lower26", D1, [[]], _Q1, page_kw=[dict(lower=26, upper=8192)], gen0=_G0)
_case("hdr/lower27", D1, [[]], _Q1, page_kw=[dict(lower=27, upper=8192)], gen0=_G0)
_case("hdr/lower31", D1, [_ONE()], _Q1, page_kw=[dict(lower=31)], gen0=_G0)

# checksums: block numbers through blkno_base and through blknos
_case("ck/good_base", D1, [_ONE(), _ONE()], _Q1, verify_checksum=True, blkno_base=7, gen0=_G0)
_case("ck/good_blknos", D1, [_ONE(), _ONE()], _Q1, verify_checksum=True, blknos=[900, 3], gen0=_G0)
_c = _case("ck/wrong_block", D1, [_ONE()], _Q1, status=[BAD_CHECKSUM], verify_checksum=True,
           blkno_base=7, gen0=_G0)
_c.blkno_base = 8                                          # stamped for block 7, read as block 8
_c = _case("ck/bit_in_last_word", D1, [_ONE()], _Q1, status=[BAD_CHECKSUM], verify_checksum=True,
           gen0=_G0)
_c.pages[0] = _c.pages[0][:-1] + bytes([_c.pages[0][-1] ^ 0x80])
_c = _case("ck/bit_in_pd_checksum", D1, [_ONE()], _Q1, status=[BAD_CHECKSUM],
           verify_checksum=True, gen0=_G0)
_c.pages[0] = _c.pages[0][:8] + bytes([_c.pages[0][8] ^ 0x01]) + _c.pages[0][9:]
_c = _case("ck/not_verified", D1, [_ONE()], _Q1, gen0=_G0)  # a stale checksum nobody asked about
_c.pages[0] = _c.pages[0][:-1] + bytes([_c.pages[0][-1] ^ 0x80])

# lower == upper == special == page_sz: the line pointer array fills the page,
# nitems is at its maximum and the last chunk is the kernel's maxchunks-th.
# Only the last chunk holds LP_NORMAL pointers; they point at offset 24, into
# the (zero) LP_UNUSED words: gen 0 and the empty list keep them unread, a qual
# deforms 23 zero bytes (t_hoff 0: a bad header) and drops them.
for _sz in (1024, 8192, 32768):
    _n = (_sz - 24) // 4
    _tl = [Tup(flags=0, len=0, off=0, expect={"all": "D", "nn": "D"}) for _ in range(_n)]
    for _i in (_n - 1, _n - 2, ((_n - 1) // 64) * 64):     # the last two and the chunk's first
        _tl[_i] = Tup(flags=1, len=23, off=24, expect={"all": "K", "nn": "D"})
    _case(f"hdr/full_{_sz}", D1, [_tl], {"all": [], "nn": [Q("a", "notnull")]}, page_sz=_sz,
          page_kw=[dict(lower=_sz, upper=_sz, special=_sz)], gen0={"all": dict()})

# ============================================================== line pointers
_good = tuple_raw(i4(5))
_QL = {"all": [], "a5": [Q("a", "eq", (5,))]}
_G0L = {"all": dict(), "a5": dict(attr_off=0, attr_width=4, lo=5, hi=5)}
_KK, _DD = {"all": "K", "a5": "K"}, {"all": "D", "a5": "D"}
_case("lp/flags_and_bounds", D1, [[
    Tup(_good, _KK, {"a": (5, 1)}),
    # not LP_NORMAL: not followed, and an item naming one projects as NULL
    Tup(_good, _DD, {"a": (0, 0)}, flags=0, note="LP_UNUSED"),
    Tup(_good, _DD, {"a": (0, 0)}, flags=2, note="LP_REDIRECT"),
    Tup(_good, _DD, {"a": (0, 0)}, flags=3, note="LP_DEAD"),
    Tup(_good, _KK, {"a": (5, 1)}, same_as=0, note="a second pointer to tuple 0"),
    Tup(_good, _DD, len=22, note="lp_len below a tuple header"),
    # lp_len 23 with t_hoff 24: followed, but the header does not fit its own length
    Tup(_good, {"all": "K", "a5": "D"}, {"a": (0, 0)}, len=23),
    Tup(tuple_raw(b"", natts=0, hoff=23), {"all": "K", "a5": "D"}, {"a": (0, 0)}, len=23),
    Tup(tuple_raw(b"", natts=0, hoff=24), {"all": "K", "a5": "D"}, {"a": (0, 0)}, len=24),
    Tup(_good, _DD, off=16, note="inside the page header"),
    Tup(_good, _KK, {"a": (5, 1)}, len=64, note="lp_len longer than the tuple's data"),
    Tup(_good, _DD, off=8192 - 24, len=29, note="off + len == page_sz + 5"),
    Tup(_good, _DD, {"a": (0, 0)}, off=4100, note="lp_off not MAXALIGNed (4 mod 8)"),
    Tup(_good, _DD, off=4098, note="lp_off 2 mod 8"),
    Tup(_good, _DD, off=4097, note="lp_off odd"),
]], _QL, gen0=_G0L)
# tuples at the page's end (special == page_sz): one of length 29 whose last
# attribute lies in the page's last word, one whose lp_len reaches page_sz exactly
_end = tuple_raw(i4(5) + b"\x07", natts=2)
_case("lp/ends_at_page_end", T.TupleDesc.of([("a", "int4"), ("c", "char")]), [[
    Tup(_end, _KK, {"a": (5, 1), "c": (7, 1)}, off=8192 - 32, len=29),
    Tup(_end, _DD, off=8192 - 24, len=25, note="off + len == page_sz + 1"),
    Tup(_end, _KK, {"a": (5, 1), "c": (0, 0)}, off=8192 - 32, len=28, note="c cut off by lp_len"),
    Tup(_end, _KK, {"a": (5, 1), "c": (7, 1)}, off=8192 - 32, len=32, note="off + len == page_sz"),
]], _QL, page_kw=[dict(upper=8192 - 32)], gen0=_G0L)
# off 24: the tuple overlaps the line pointer array itself (followed unread)
_case("lp/off24", D1, [[Tup(flags=1, len=23, off=24, expect={"all": "K"})]], {"all": []},
      gen0={"all": dict()})

# item counts around the 64-lane chunk; 128 items with only lane 0 of chunk 0
# and only lane 63 of chunk 1 kept
for _n in (1, 63, 64, 65, 128):
    _tl = []
    for _i in range(_n):
        _v = 7 if _i in (0, 127) else 1000 + _i
        _tl.append(Tup(tuple_raw(i4(_v)), {"all": "K", "a7": "K" if _v == 7 else "D",
                                           "big": "D" if _v == 7 else "K"},
                       {"a": (_v, 1)} if _i % 31 == 0 else None))
    _case(f"lp/items_{_n}", D1, [_tl], {"all": [], "a7": [Q("a", "eq", (7,))],
                                        "big": [Q("a", "ge", (1000,))]},
          gen0={"all": dict(), "a7": dict(attr_off=0, attr_width=4, lo=7, hi=7),
                "big": dict(attr_off=0, attr_width=4, lo=1000, hi=(1 << 31) - 1)})

# ============================================================== tuple header
D4 = T.TupleDesc.of([("a", "int4"), ("b", "int4"), ("c", "int4"), ("d", "int4")])
_abcd = i4(1) + i4(2) + i4(3) + i4(4)
_QH = {"all": [], "a1": [Q("a", "eq", (1,))], "c3": [Q("c", "eq", (3,))],
       "cnull": [Q("c", "isnull")], "anull": [Q("a", "isnull")]}
_ok = {"all": "K", "a1": "K", "c3": "K", "cnull": "D", "anull": "D"}
_bad = {"all": "K", "a1": "D", "c3": "D", "cnull": "D", "anull": "D"}   # a bad header: NULL tests fail too
_P4 = lambda a, b, c, d: {"a": a, "b": b, "c": c, "d": d}
_v = lambda x: (x, 1)
_N = (0, 0)
_case("th/hoff_natts", D4, [[
    Tup(tuple_raw(_abcd, natts=4), _ok, _P4(_v(1), _v(2), _v(3), _v(4))),
    Tup(tuple_raw(_abcd, natts=4, hoff=22), _bad, _P4(_N, _N, _N, _N), note="t_hoff 22"),
    # t_hoff 23: PostgreSQL writes t_hoff MAXALIGNed and places attributes relative
    # to it (verify_heapam reports any other value as corruption): a bad header
    Tup(tuple_raw(b"\0" + _abcd, natts=4, hoff=23), _bad, _P4(_N, _N, _N, _N), note="t_hoff 23"),
    Tup(tuple_raw(b"\0" * 4 + _abcd, natts=4, hoff=28), _bad, _P4(_N, _N, _N, _N), note="t_hoff 28"),
    Tup(tuple_raw(_abcd, natts=4, hoff=32), _ok, _P4(_v(1), _v(2), _v(3), _v(4)), note="t_hoff 32"),
    Tup(tuple_raw(b"", natts=4, hoff=24), _bad, _P4(_N, _N, _N, _N), note="t_hoff == lp_len"),
    Tup(tuple_raw(b"", natts=0, hoff=24),
        {"all": "K", "a1": "D", "c3": "D", "cnull": "K", "anull": "K"}, _P4(_N, _N, _N, _N),
        note="t_hoff == lp_len, nothing stored"),
    Tup(tuple_raw(_abcd, natts=4, hoff=48), _bad, _P4(_N, _N, _N, _N), len=40, note="t_hoff > lp_len"),
    # HEAP_HASNULL, 9 attributes stored, t_hoff 24: the bitmap needs 2 bytes, 23 + 2 > 24
    Tup(tuple_raw(_abcd, natts=9, infomask=VIS | HASNULL, hoff=24, bits=b"\xff"), _bad,
        _P4(_N, _N, _N, _N)),
    # ... 8 attributes: one bitmap byte fits
    Tup(tuple_raw(_abcd, natts=8, infomask=VIS | HASNULL, hoff=24, bits=b"\x0f"), _ok,
        _P4(_v(1), _v(2), _v(3), _v(4))),
    Tup(tuple_raw(_abcd, natts=0), {"all": "K", "a1": "D", "c3": "D", "cnull": "K", "anull": "K"},
        _P4(_N, _N, _N, _N), note="stored natts 0: every attribute NULL"),
    Tup(tuple_raw(i4(1) + i4(2), natts=2),
        {"all": "K", "a1": "K", "c3": "D", "cnull": "K", "anull": "D"}, _P4(_v(1), _v(2), _N, _N),
        note="stored natts below the qual's attribute"),
    Tup(tuple_raw(_abcd, natts=2047), _ok, _P4(_v(1), _v(2), _v(3), _v(4)),
        note="stored natts 2047, 4-column descriptor"),
    # NULLs before and after: bitmap 0b1010 = b and d stored
    Tup(tuple_raw(i4(2) + i4(4), natts=4, infomask=VIS | HASNULL, bits=b"\x0a"),
        {"all": "K", "a1": "D", "c3": "D", "cnull": "K", "anull": "K"}, _P4(_N, _v(2), _N, _v(4))),
    Tup(tuple_raw(b"", natts=4, infomask=VIS | HASNULL, bits=b"\x00"),
        {"all": "K", "a1": "D", "c3": "D", "cnull": "K", "anull": "K"}, _P4(_N, _N, _N, _N),
        note="all NULL"),
    # c and d cut off by lp_len: a qual on a never gets that far
    Tup(tuple_raw(_abcd, natts=4), {"all": "K", "a1": "K", "c3": "D", "cnull": "D", "anull": "D"},
        _P4(_v(1), _v(2), _N, _N), len=24 + 10),
]], _QH)

# ================================================================== deformer
D6 = T.TupleDesc.of([("a", "int4"), ("t", "text"), ("b", "int8"), ("k", "bool"),
                     ("f", "float8"), ("s", "int2"), ("c", "char"), ("z", "int2")])
_QD = {"all": [], "a": [Q("a", "eq", (-7,))], "b": [Q("b", "eq", (-(1 << 63),))],
       "bmax": [Q("b", "eq", ((1 << 63) - 1,))], "z": [Q("z", "eq", (-2,))],
       "t": [Q("t", "text_eq", ("xy",))], "ab": [Q("a", "eq", (-7,)), Q("b", "le", (0,))],
       "back": [Q("f", "le", (0.0,)), Q("t", "notnull"), Or(Q("f", "gt", (5.0,)), Q("a", "eq", (-7,)))]}
_MIN8 = -(1 << 63)


def _row(t: bytes, pad_b: int, b: int = _MIN8, tail: bool = True) -> bytes:
    """a = -7, t, pad_b zero bytes, b, k = 1, pad, f = -0.5, s = -3, c = -1, pad, z = -2"""
    r = i4(-7) + t + b"\0" * pad_b + i8(b)
    if tail:
        r += b"\x01" + b"\0" * 7 + f8(-0.5) + i2(-3) + b"\xff" + b"\0" + i2(-2)
    return r


def _exp(**kw):
    e = {"all": "K", "a": "K", "b": "K", "bmax": "D", "z": "K", "t": "D", "ab": "K", "back": "K"}
    e.update(kw)
    return e


_full = lambda t: {"a": (-7, 1), "t": t, "b": (_MIN8, 1), "k": (1, 1), "f": (-0.5, 1),
                   "s": (-3, 1), "c": (-1, 1), "z": (-2, 1)}
# int8 after short text of 1, 2, 3 and 5 data bytes: a at 24, t's header at 28
_case("df/int8_after_text", D6, [[
    Tup(tuple_raw(_row(short(b"x"), 2), natts=8), _exp(), _full((b"x", 1))),            # 28..30, b at 32
    Tup(tuple_raw(_row(short(b"xy"), 1), natts=8), _exp(t="K"), _full((b"xy", 1))),      # 28..31
    Tup(tuple_raw(_row(short(b"xyz"), 0), natts=8), _exp(), _full((b"xyz", 1))),         # 28..32
    Tup(tuple_raw(_row(short(b"xyzuv"), 6), natts=8), _exp(), _full((b"xyzuv", 1))),     # 28..34, b at 40
    Tup(tuple_raw(_row(short(b""), 3), natts=8), _exp(), _full((b"", 1)), note="short header 0x03: empty"),
    Tup(tuple_raw(_row(short(b"xy"), 1, b=(1 << 63) - 1), natts=8),
        _exp(b="D", bmax="K", ab="D", t="K"),
        dict(_full((b"xy", 1)), b=((1 << 63) - 1, 1))),
    # the same values with one trailing NULL (z): the bitmap walk instead of attcacheoff
    Tup(tuple_raw(_row(short(b"xy"), 1)[:-2], natts=8, infomask=VIS | HASNULL, bits=b"\x7f"),
        _exp(z="D", t="K"), dict(_full((b"xy", 1)), z=(0, 0))),
    # a 126-byte short value (header 0xFF), b at 28 + 127 = 155 -> 160
    Tup(tuple_raw(_row(short(b"q" * 126), 5), natts=8), _exp(), _full((b"q" * 126, 1))),
]], _QD)

# 4-byte headers: 0..3 pad bytes in front (t follows a 4-aligned int4, so put
# a "char"-led descriptor in front to move it)
D5 = T.TupleDesc.of([("p", "char"), ("q", "char"), ("r", "char"), ("t", "text"), ("b", "int8")])
_QV = {"all": [], "t": [Q("t", "text_eq", ("hello",))], "b": [Q("b", "eq", (9,))],
       "tn": [Q("t", "notnull")], "pfx": [Q("t", "prefix", ("hel",))]}
_ev = lambda **kw: dict({"all": "K", "t": "K", "b": "K", "tn": "K", "pfx": "K"}, **kw)
_ebad = {"all": "K", "t": "D", "b": "D", "tn": "D", "pfx": "D"}
_pv = lambda t, b=(9, 1): {"p": (1, 1), "t": t, "b": b}
_h5 = long4(b"hello")                                   # 9 bytes
_b64 = b"h" * 60                                        # 4 + 60 = 64: the header's low byte is 0
_case("df/varlena_headers", D5, [[
    # p at 24; NULL bitmap moves t: stored {p,t,b} -> t wants 25: 3 pad bytes to 28
    Tup(tuple_raw(b"\x01\0\0\0" + _h5 + b"\0" * 3 + i8(9), natts=5, infomask=VIS | HASNULL,
                  bits=b"\x19"), _ev(), _pv((b"hello", 1))),
    # {p,q,t,b}: t wants 26, 2 pad bytes
    Tup(tuple_raw(b"\x01\x02\0\0" + _h5 + b"\0" * 3 + i8(9), natts=5, infomask=VIS | HASNULL,
                  bits=b"\x1b"), _ev(), _pv((b"hello", 1))),
    # {p,q,r,t,b}: t wants 27, 1 pad byte
    Tup(tuple_raw(b"\x01\x02\x03\0" + _h5 + b"\0" * 3 + i8(9), natts=5), _ev(), _pv((b"hello", 1))),
    # {t,b}: t at 24, no pad
    Tup(tuple_raw(_h5 + b"\0" * 7 + i8(9), natts=5, infomask=VIS | HASNULL, bits=b"\x18"),
        _ev(), {"p": (0, 0), "t": (b"hello", 1), "b": (9, 1)}),
    # a 4-byte header whose total length is 64: its first byte is 0, as a pad byte is,
    # and the datum starts aligned all the same
    Tup(tuple_raw(long4(_b64) + b"\0" * 0 + i8(9), natts=5, infomask=VIS | HASNULL, bits=b"\x18"),
        _ev(t="D", pfx="D"), {"p": (0, 0), "t": (_b64, 1), "b": (9, 1)}),
    # 4-byte header of length 4: empty; of length 3: shorter than itself, malformed
    Tup(tuple_raw(struct.pack("<I", 4 << 2) + b"\0" * 4 + i8(9), natts=5, infomask=VIS | HASNULL,
                  bits=b"\x18"), _ev(t="D", pfx="D"), {"p": (0, 0), "t": (b"", 1), "b": (9, 1)}),
    Tup(tuple_raw(struct.pack("<I", 3 << 2) + b"\0" * 4 + i8(9), natts=5, infomask=VIS | HASNULL,
                  bits=b"\x18"), _ebad, {"p": (0, 0), "t": (0, 0), "b": (0, 0)}),
    # TOAST pointers: tag 18 (18 bytes in all), tags 1..3 (10 bytes)
    Tup(tuple_raw(toast(18) + b"\0" * 6 + i8(9), natts=5, infomask=VIS | HASNULL, bits=b"\x18"),
        _ev(t="R", pfx="R"), {"p": (0, 0), "t": (16, 2), "b": (9, 1)}),
    Tup(tuple_raw(toast(1) + b"\0" * 6 + i8(9), natts=5, infomask=VIS | HASNULL, bits=b"\x18"),
        _ev(t="R", pfx="R"), {"p": (0, 0), "t": (8, 2), "b": (9, 1)}),
    Tup(tuple_raw(toast(2) + b"\0" * 6 + i8(9), natts=5, infomask=VIS | HASNULL, bits=b"\x18"),
        _ev(t="R", pfx="R"), {"p": (0, 0), "t": (8, 2), "b": (9, 1)}),
    Tup(tuple_raw(toast(3) + b"\0" * 6 + i8(9), natts=5, infomask=VIS | HASNULL, bits=b"\x18"),
        _ev(t="R", pfx="R"), {"p": (0, 0), "t": (8, 2), "b": (9, 1)}),
    # unknown tags 0, 4, 17: malformed
    Tup(tuple_raw(toast(0) + b"\0" * 6 + i8(9), natts=5, infomask=VIS | HASNULL, bits=b"\x18"),
        _ebad, {"p": (0, 0), "t": (0, 0), "b": (0, 0)}),
    Tup(tuple_raw(toast(4) + b"\0" * 6 + i8(9), natts=5, infomask=VIS | HASNULL, bits=b"\x18"),
        _ebad, {"p": (0, 0), "t": (0, 0), "b": (0, 0)}),
    Tup(tuple_raw(toast(17) + b"\0" * 6 + i8(9), natts=5, infomask=VIS | HASNULL, bits=b"\x18"),
        _ebad, {"p": (0, 0), "t": (0, 0), "b": (0, 0)}),
    # a TOAST pointer cut after the tag: {t} only, lp_len 26
    Tup(tuple_raw(b"\x01\x12", natts=5, infomask=VIS | HASNULL, bits=b"\x08"),
        {"all": "K", "t": "D", "b": "D", "tn": "D", "pfx": "D"},
        {"p": (0, 0), "t": (0, 0), "b": (0, 0)}),
    # ... and cut after its header byte: lp_len 25
    Tup(tuple_raw(b"\x01", natts=5, infomask=VIS | HASNULL, bits=b"\x08"),
        {"all": "K", "t": "D", "b": "D", "tn": "D", "pfx": "D"},
        {"p": (0, 0), "t": (0, 0), "b": (0, 0)}),
    # inline compressed: 4-byte header with bit 1 set, 8 payload bytes
    Tup(tuple_raw(long4(b"\x10\0\0\0abcd", flag=2) + b"\0" * 4 + i8(9), natts=5,
                  infomask=VIS | HASNULL, bits=b"\x18"),
        _ev(t="R", pfx="R"), {"p": (0, 0), "t": (8, 2), "b": (9, 1)}),
    # a varlena that ends exactly at lp_len, and one byte beyond it ({t} only)
    Tup(tuple_raw(short(b"hello"), natts=5, infomask=VIS | HASNULL, bits=b"\x08"),
        _ev(b="D"), {"p": (0, 0), "t": (b"hello", 1), "b": (0, 0)}),
    Tup(tuple_raw(short(b"hello"), natts=5, infomask=VIS | HASNULL, bits=b"\x08"),
        {"all": "K", "t": "D", "b": "D", "tn": "D", "pfx": "D"},
        {"p": (0, 0), "t": (0, 0), "b": (0, 0)}, len=24 + 5),
    # a malformed later attribute (b runs past lp_len), quals on earlier ones only
    Tup(tuple_raw(_h5 + b"\0" * 7 + i8(9), natts=5, infomask=VIS | HASNULL, bits=b"\x18"),
        _ev(b="D"), {"p": (0, 0), "t": (b"hello", 1), "b": (0, 0)}, len=24 + 16 + 7),
]], _QV)

# cstring with and without its NUL; fixed widths holding negative values after
# bool / "char"
DC = T.TupleDesc.of([("k", "bool"), ("f", "float8"), ("c", "char"), ("s", "int2"),
                     ("n", "cstring"), ("w", "int4")])
_QC = {"all": [], "f": [Q("f", "between", (-2.5, -2.5))], "s": [Q("s", "eq", (-300,))],
       "w": [Q("w", "eq", (-100000,))], "k": [Q("k", "eq", (1,))], "c": [Q("c", "eq", (-128,))]}
_rowc = b"\x01" + b"\0" * 7 + f8(-2.5) + b"\x80" + b"\0" + i2(-300)
_case("df/cstring_fixed", DC, [[
    # k 24, f 32, c 40, s 42, n 44.."ab\0" = 47, w at 48
    Tup(tuple_raw(_rowc + b"ab\0" + b"\0" + i4(-100000), natts=6),
        {"all": "K", "f": "K", "s": "K", "w": "K", "k": "K", "c": "K"},
        {"k": (1, 1), "f": (-2.5, 1), "c": (-128, 1), "s": (-300, 1), "n": (b"ab\0", 1),
         "w": (-100000, 1)}),
    # no NUL before lp_len: n and w malformed, the earlier columns are not
    Tup(tuple_raw(_rowc + b"abcd", natts=6),
        {"all": "K", "f": "K", "s": "K", "w": "D", "k": "K", "c": "K"},
        {"k": (1, 1), "f": (-2.5, 1), "c": (-128, 1), "s": (-300, 1), "n": (0, 0), "w": (0, 0)}),
]], _QC)

# ==================================================================== floats
DF = T.TupleDesc.of([("x", "float4"), ("y", "float8")])
_nan, _inf = math.nan, math.inf
_QF = {"xnan": [Q("x", "eq", (_nan,))], "xle": [Q("x", "le", (0.0,))], "xz": [Q("x", "eq", (0.0,))],
       "xinf": [Q("x", "ge", (_inf,))], "xden": [Q("x", "between", (1e-45, 2e-45))],
       "ynan": [Q("y", "between", (_nan, _nan))], "yz": [Q("y", "eq", (0.0,))],
       "yall": [Q("y", "between", (-_inf, _nan))], "ynone": [Q("y", "between", (1.0, -1.0))]}


def _fexp(k: str):
    return {n: ("K" if n in k.split() else "D") for n in _QF}


_fr = lambda x, y: tuple_raw(x + y, natts=2)
_den = struct.pack("<I", 1)                                # float4 denormal 1.4e-45
_case("fl/order", DF, [[
    # NaN equals NaN and sorts above everything, +inf included
    Tup(_fr(f4(_nan), b"\0" * 4 + f8(_nan)), _fexp("xnan xinf ynan yall"),
        {"x": (_nan, 1), "y": (_nan, 1)}),
    Tup(_fr(f4(-0.0), b"\0" * 4 + f8(-0.0)), _fexp("xle xz yz yall"), {"x": (-0.0, 1), "y": (-0.0, 1)}),
    Tup(_fr(f4(_inf), b"\0" * 4 + f8(0.0)), _fexp("xinf yz yall"), {"x": (_inf, 1), "y": (0.0, 1)}),
    Tup(_fr(f4(-_inf), b"\0" * 4 + f8(-_inf)), _fexp("xle yall"), {"x": (-_inf, 1), "y": (-_inf, 1)}),
    Tup(_fr(_den, b"\0" * 4 + f8(1.0)), _fexp("xden yall"),
        {"x": (struct.unpack("<f", _den)[0], 1), "y": (1.0, 1)}),
]], _QF)

# ===================================================================== quals
DQ = T.TupleDesc.of([("i", "int4"), ("t", "text"), ("j", "int2"), ("u", "text")])
_in40 = [3 * k for k in range(40)] + [9, 9]
_s33 = b"0123456789abcdefghijklmnopqrstuvw"                # 33 bytes
_QQ = {
    "lo": [Q("i", "between", (10, 20))], "empty": [Q("i", "between", (20, 10))],
    "in1": [Q("i", "in", ([10],))], "in4": [Q("i", "in", ([1, 20, 20, 15],))],
    # 2 and 4 distinct values (the fixed list's limit), 5 (the program only)
    "in2": [Q("i", "in", ([10, 15],))], "in4d": [Q("i", "in", ([1, 20, 15, 9],))],
    "in5": [Q("i", "in", ([10, 15, 20, 1, 9],))],
    "in40": [Q("i", "in", (_in40,))], "in0": [Q("i", "in", ([],))],
    "t0": [Q("t", "text_eq", ("",))], "t1": [Q("t", "text_eq", ("a",))],
    "t3": [Q("t", "text_eq", ("abc",))], "t4": [Q("t", "text_eq", ("abcd",))],
    "t5": [Q("t", "text_eq", ("abcde",))], "t8": [Q("t", "text_eq", ("abcdefgh",))],
    "t9": [Q("t", "text_eq", ("abcdefghi",))], "t32": [Q("t", "text_eq", (_s33[:32],))],
    "t33": [Q("t", "text_eq", (_s33,))],
    "p3": [Q("t", "prefix", ("abc",))], "p9": [Q("t", "prefix", ("abcdefghi",))],
    "tin": [Q("t", "text_in", (["abd", "abc", "xbc"],))],
    # clauses that go back to an earlier attribute: (u) (t) (u OR i)
    "back": [Q("u", "notnull"), Q("t", "prefix", ("a",)), Or(Q("u", "text_eq", ("zz",)), Q("i", "eq", (10,)))],
    "ext_or": [Or(Q("u", "text_eq", ("zz",)), Q("i", "ge", (10,)))],
    "ext": [Q("u", "text_eq", ("zz",))],
    "ext_false": [Q("u", "text_eq", ("zz",)), Q("i", "eq", (-1,))],
}


def _qexp(k: str, r: str = ""):
    return {n: ("K" if n in k.split() else "R" if n in r.split() else "D") for n in _QQ}


def _qrow(i: int, t: bytes, u: bytes = None) -> bytes:
    """i, t (short header), j = 1 aligned to 2, u"""
    r = i4(i) + short(t)
    r += b"\0" * (len(r) % 2) + i2(1)
    return r + (short(b"zz") if u is None else u)


_qt = lambda i, t, u=None: tuple_raw(_qrow(i, t, u), natts=4)
_case("ql/kinds", DQ, [[
    Tup(_qt(10, b""), _qexp("lo in1 in2 in5 t0 ext_or ext")),                      # range edge lo, in1
    Tup(_qt(20, b"a"), _qexp("lo in4 in4d in5 t1 back ext_or ext")),                # range edge hi; back: u zz
    Tup(_qt(9, b"abc"), _qexp("in4d in5 in40 t3 p3 tin back ext_or ext")),                 # 9 = 3*3 and the duplicate
    Tup(_qt(21, b"abcd"), _qexp("in40 t4 p3 back ext_or ext")),
    Tup(_qt(15, b"abcde"), _qexp("lo in4 in2 in4d in5 in40 t5 p3 back ext_or ext")),
    Tup(_qt(117, b"abcdefgh"), _qexp("in40 t8 p3 back ext_or ext")),       # 117 = 3*39, the last entry
    Tup(_qt(118, b"abcdefghi"), _qexp("t9 p3 p9 back ext_or ext")),
    Tup(_qt(0, _s33[:32]), _qexp("in40 t32 ext_or ext")),
    Tup(_qt(1, _s33), _qexp("in4 in4d in5 t33 ext_or ext")),
    # values that differ from the constant in the last byte only, at each length mod 4
    Tup(_qt(10, b"b"), _qexp("lo in1 in2 in5 ext_or ext")),
    Tup(_qt(10, b"abd"), _qexp("lo in1 in2 in5 tin back ext_or ext")),
    Tup(_qt(10, b"abce"), _qexp("lo in1 in2 in5 p3 back ext_or ext")),
    Tup(_qt(10, b"abcdf"), _qexp("lo in1 in2 in5 p3 back ext_or ext")),
    Tup(_qt(10, b"abcdefgx"), _qexp("lo in1 in2 in5 p3 back ext_or ext")),
    Tup(_qt(10, b"abcdefghx"), _qexp("lo in1 in2 in5 p3 back ext_or ext")),
    Tup(_qt(10, _s33[:31] + b"!"), _qexp("lo in1 in2 in5 ext_or ext")),
    Tup(_qt(10, _s33[:32] + b"!"), _qexp("lo in1 in2 in5 ext_or ext")),
    # a prefix equal to the value, and one longer than it
    Tup(_qt(-5, b"ab"), _qexp("back ext_or ext")),
    Tup(_qt(10, b"xbc"), _qexp("lo in1 in2 in5 tin ext_or ext")),
    # u out of line: EXT OR true keeps, EXT alone rechecks, EXT and a false clause drops
    Tup(_qt(10, b"abc", toast(18)), _qexp("lo in1 in2 in5 t3 p3 tin back ext_or", "ext")),
    Tup(_qt(5, b"abc", toast(18)), _qexp("t3 p3 tin", "back ext_or ext")),
    Tup(_qt(-1, b"zzz", toast(18)), _qexp("", "ext_or ext ext_false")),
    # u NULL: (u notnull) fails
    Tup(tuple_raw(_qrow(10, b"abc", b""), natts=4, infomask=VIS | HASNULL, bits=b"\x07"),
        _qexp("lo in1 in2 in5 t3 p3 tin ext_or")),
]], _QQ)
# the last-but-one row above: i = -1 makes ext_false's second clause TRUE, so
# the undecidable first clause stands: recheck.  A false later clause drops:
CASES[-1].tups[0].append(Tup(_qt(7, b"zzz", toast(18)), _qexp("", "ext_or ext")))
CASES[-1].pages[0] = build_page(CASES[-1].tups[0])

# =================================================================== numeric
DN = T.TupleDesc.of([("n", "numeric")])
_QN = {
    "eq1": [Q("n", "eq", (1,))], "ge1": [Q("n", "ge", (1,))], "gt1": [Q("n", "gt", (1,))],
    "le1": [Q("n", "le", (1,))], "lt1": [Q("n", "lt", (1,))], "z": [Q("n", "eq", (0,))],
    "nan": [Q("n", "eq", ("NaN",))], "genan": [Q("n", "ge", ("NaN",))],
    "ltnan": [Q("n", "lt", ("NaN",))], "leinf": [Q("n", "le", ("Infinity",))],
    "ltinf": [Q("n", "lt", ("Infinity",))], "geninf": [Q("n", "ge", ("-Infinity",))],
    "gtninf": [Q("n", "gt", ("-Infinity",))],
    "big": [Q("n", "eq", ("123456789012.3456",))],      # 1234 5678 9012 . 3456: four digits
    "pre": [Q("n", "gt", ("1234.5678",))],              # 1234 . 5678
    "small": [Q("n", "between", ("0.0001", "0.0001"))], "nn": [Q("n", "notnull")],
}


def _nexp(k: str):
    return {n: ("K" if n in k.split() + ["nn"] else "D") for n in _QN}


_nt = lambda payload, hdr4=False: tuple_raw(long4(payload) if hdr4 else short(payload), natts=1)
_fin = "leinf ltinf geninf gtninf ltnan"                    # what every finite value passes
_case("nm/forms", DN, [[
    Tup(_nt(num_short(0, [1])), _nexp("eq1 ge1 le1 " + _fin)),
    Tup(_nt(num_long(0, [1])), _nexp("eq1 ge1 le1 " + _fin), note="the same value, NumericLong"),
    Tup(_nt(num_short(0, [1], dscale=2)), _nexp("eq1 ge1 le1 " + _fin), note="1.00"),
    Tup(_nt(num_short(1, [0, 1])), _nexp("eq1 ge1 le1 " + _fin), note="a leading zero digit"),
    Tup(_nt(num_short(0, [1, 0, 0])), _nexp("eq1 ge1 le1 " + _fin), note="trailing zero digits"),
    Tup(_nt(num_short(0, [1], neg=True)), _nexp("le1 lt1 " + _fin), note="-1"),
    Tup(_nt(num_short(-1, [1])), _nexp("le1 lt1 small " + _fin), note="0.0001: weight -1"),
    Tup(_nt(num_short(-64, [1])), _nexp("le1 lt1 " + _fin), note="weight -64"),
    Tup(_nt(num_short(63, [1])), _nexp("ge1 gt1 pre " + _fin), note="weight 63"),
    Tup(_nt(num_long(200, [1])), _nexp("ge1 gt1 pre " + _fin), note="weight 200 needs the long form"),
    Tup(_nt(num_long(-200, [1], neg=True)), _nexp("le1 lt1 " + _fin)),
    # zero: no digits, under every sign; and "negative zero" with a zero digit
    Tup(_nt(num_short(0, [])), _nexp("z le1 lt1 " + _fin)),
    Tup(_nt(num_short(0, [], neg=True)), _nexp("z le1 lt1 " + _fin)),
    Tup(_nt(num_long(5, [], neg=True)), _nexp("z le1 lt1 " + _fin)),
    Tup(_nt(num_short(0, [0], neg=True)), _nexp("z le1 lt1 " + _fin)),
    # specials: NaN = NaN and above +inf; the strict bounds at equality
    Tup(_nt(struct.pack("<H", 0xC000)), _nexp("nan genan ge1 gt1 pre geninf gtninf")),
    Tup(_nt(struct.pack("<H", 0xD000)), _nexp("ge1 gt1 pre leinf geninf gtninf ltnan")),
    Tup(_nt(struct.pack("<H", 0xF000)), _nexp("le1 lt1 leinf ltinf geninf ltnan")),
    # no numerics: special 0xE000, an odd payload, a payload under 2 bytes
    Tup(_nt(struct.pack("<H", 0xE000)), _nexp("")),
    Tup(_nt(num_short(0, [1]) + b"\x00"), _nexp("")),
    Tup(_nt(b"\x80"), _nexp("")),
    Tup(_nt(b""), _nexp("")),
    Tup(_nt(num_long(0, [])[:3]), _nexp(""), note="NumericLong cut inside its weight"),
    # a 4-byte varlena header
    Tup(_nt(num_short(0, [1]), hdr4=True), _nexp("eq1 ge1 le1 " + _fin)),
    # 12 digits before the point: equal, and different in the last digit only
    Tup(_nt(num_short(2, [1234, 5678, 9012, 3456], dscale=4)), _nexp("big ge1 gt1 pre " + _fin)),
    Tup(_nt(num_short(2, [1234, 5678, 9012, 3457], dscale=4)), _nexp("ge1 gt1 pre " + _fin)),
    # a digit-prefix of the constant 1234.5678, and one digit more than it
    Tup(_nt(num_short(0, [1234])), _nexp("ge1 gt1 " + _fin)),
    Tup(_nt(num_short(0, [1234, 5678])), _nexp("ge1 gt1 " + _fin), note="equal: gt fails"),
    Tup(_nt(num_short(0, [1234, 5678, 1])), _nexp("ge1 gt1 pre " + _fin)),
    # out of line: undecidable
    Tup(tuple_raw(toast(18), natts=1), {n: ("K" if n == "nn" else "R") for n in _QN}),
]], _QN)


# NaN, +inf and -inf against every bound kind, the strict flags at equality.
# The order: -inf < every finite value < +inf < NaN, and NaN = NaN.  Rows:
# N (NaN), P (+Infinity), M (-Infinity), F (the finite 1); per qualifier set
# the rows it keeps.
_SP = {"N": struct.pack("<H", 0xC000), "P": struct.pack("<H", 0xD000),
       "M": struct.pack("<H", 0xF000), "F": num_short(0, [1])}
_SPQ = {
    "eq_nan": (Q("n", "eq", ("NaN",)), "N"), "ge_nan": (Q("n", "ge", ("NaN",)), "N"),
    "gt_nan": (Q("n", "gt", ("NaN",)), ""), "le_nan": (Q("n", "le", ("NaN",)), "NPMF"),
    "lt_nan": (Q("n", "lt", ("NaN",)), "PMF"),
    "eq_pinf": (Q("n", "eq", ("Infinity",)), "P"), "ge_pinf": (Q("n", "ge", ("Infinity",)), "NP"),
    "gt_pinf": (Q("n", "gt", ("Infinity",)), "N"), "le_pinf": (Q("n", "le", ("Infinity",)), "PMF"),
    "lt_pinf": (Q("n", "lt", ("Infinity",)), "MF"),
    "eq_minf": (Q("n", "eq", ("-Infinity",)), "M"), "ge_minf": (Q("n", "ge", ("-Infinity",)), "NPMF"),
    "gt_minf": (Q("n", "gt", ("-Infinity",)), "NPF"), "le_minf": (Q("n", "le", ("-Infinity",)), "M"),
    "lt_minf": (Q("n", "lt", ("-Infinity",)), ""),
    "bt_minf_pinf": (Q("n", "between", ("-Infinity", "Infinity")), "PMF"),
    "bt_nan_nan": (Q("n", "between", ("NaN", "NaN")), "N"),
    "bt_pinf_nan": (Q("n", "between", ("Infinity", "NaN")), "NP"),
    "bt_minf_minf": (Q("n", "between", ("-Infinity", "-Infinity")), "M"),
    "bt_1_pinf": (Q("n", "between", (1, "Infinity")), "PF"),
    "bt_nan_pinf": (Q("n", "between", ("NaN", "Infinity")), ""),       # an empty range
    "in_specials": (Q("n", "in", (["NaN", "-Infinity"],)), "NM"),
}
_case("nm/specials", DN, [[
    Tup(_nt(_SP[r]), {n: ("K" if r in keep else "D") for n, (_, keep) in _SPQ.items()})
    for r in "NPMF"]], {n: [q] for n, (q, _) in _SPQ.items()})


# ================================================================== geometry
def geometry_relation(npages: int, page_sz: int, seed: int = 0):
    """A small well-formed relation for the launch-geometry tests: (pages,
    desc, quals, gen 0 predicate).  Rows (id int4, v int8, t text); a few
    tuples per page, some with xmin not hinted committed (removed by a
    snapshot check or by skip_invisible)."""
    desc = T.TupleDesc.of([("id", "int4"), ("v", "int8"), ("t", "text")])
    rng = np.random.default_rng(seed + npages * 7 + page_sz)
    pages = []
    for p in range(npages):
        tl = []
        for r in range(int(rng.integers(1, 6))):
            mask = VIS if rng.random() < 0.8 else P.HEAP_XMIN_INVALID | P.HEAP_XMAX_INVALID
            row = [p * 8 + r, int(rng.integers(-50, 50)), "k%d" % int(rng.integers(0, 4))]
            tl.append(T.heap_tuple(row, desc, infomask=mask))
        pages.append(P.build_page(tl, blkno=p, page_sz=page_sz))
    # an AND list that fits the fixed form, so that gen 1 and gen 2 both run it
    quals = [Q("v", "between", (-20, 30)), Q("t", "prefix", ("k",)), Q("t", "notnull")]
    return b"".join(pages), desc, quals, dict(attr_off=8, attr_width=8, lo=-20, hi=30)


GEOMETRY_NPAGES = (1, 7, 8, 9, 31, 32, 33, 65)
PAGE_SIZES = (1024, 2048, 4096, 16384, 32768)


# =================================================================== mutants
def corpus_pages():
    """(page bytes, page size, case) of every corpus page."""
    return [(pg, c.page_sz, c) for c in CASES for pg in c.pages]


def mutants(seed: int = 20240607, n: int = 400):
    """A fixed list of (page bytes, page size, case name): corpus pages with
    bits flipped and with header, line pointer, t_hoff, natts and varlena
    header fields rewritten.  Most mutations stay away from the page header,
    so that more than half of the pages still pass the header check and the
    damage reaches the tuple code."""
    rng = np.random.default_rng(seed)
    src = [(pg, sz, c.name) for pg, sz, c in corpus_pages() if sz == 8192 and c.desc is not None
           and not c.name.startswith(("hdr/", "ck/"))]
    out = []
    for k in range(n):
        pg, sz, name = src[int(rng.integers(0, len(src)))]
        b = bytearray(pg)
        lower, upper = struct.unpack_from("<HH", b, 12)
        nlp = max(1, (lower - 24) // 4)
        for _ in range(int(rng.integers(1, 4))):
            kind = int(rng.integers(0, 10))
            lp_at = 24 + 4 * int(rng.integers(0, nlp))
            w, = struct.unpack_from("<I", b, lp_at)
            off = w & 0x7FFF
            if kind == 0:                      # a header field
                struct.pack_into("<H", b, int(rng.choice([10, 12, 14, 16, 18])),
                                 int(rng.integers(0, 1 << 16)))
            elif kind == 1:                    # a bit anywhere behind the header
                at = int(rng.integers(24, sz))
                b[at] ^= 1 << int(rng.integers(0, 8))
            elif kind in (2, 3):               # a line pointer field
                f = int(rng.integers(0, 3))
                if f == 0:
                    w = (w & ~0x7FFF) | int(rng.choice([off ^ 4, off ^ 1, sz - 24, sz - 8, 16, 24,
                                                        int(rng.integers(0, 1 << 15))]))
                elif f == 1:
                    w = (w & ~(3 << 15)) | (int(rng.integers(0, 4)) << 15)
                else:
                    ln = w >> 17
                    w = (w & 0x1FFFF) | (int(rng.choice([22, 23, 24, max(0, ln - 1), ln + 1, ln + 9,
                                                         sz - off if off < sz else 0,
                                                         int(rng.integers(0, 1 << 15))])) << 17)
                struct.pack_into("<I", b, lp_at, w & 0xFFFFFFFF)
            elif off + 24 <= sz:
                if kind == 4:                  # t_hoff
                    b[off + 22] = int(rng.choice([0, 22, 23, 24, 25, 32, 255,
                                                  int(rng.integers(0, 256))]))
                elif kind == 5:                # natts / infomask2
                    struct.pack_into("<H", b, off + 18, int(rng.choice([0, 1, 2, 9, 2047, 0xFFFF])))
                elif kind == 6:                # infomask: HASNULL and the rest
                    b[off + 20] ^= int(rng.choice([1, 1, 2, 0x80]))
                else:                          # a byte of the data: varlena headers live here
                    ln = w >> 17
                    at = off + 24 + int(rng.integers(0, max(1, min(ln, 64))))
                    if at < sz:
                        b[at] = int(rng.choice([0, 1, 2, 3, 0x12, 0xFF, 0x10, int(rng.integers(0, 256))]))
        out.append((bytes(b), sz, name))
    return out
