"""Case generator and an independent reference for the LIKE qualifier
(csrc/kernels/collike.hip, ``P.like`` / ``contains`` / ``endswith``), shared
by the CPU and GPU tests.  Tables are qualgen's (one buffer set per record
batch, every batch on a fresh bitmap word).

The reference shares no code with ``colpred.evaluate``: a pattern becomes a
Python ``re`` over bytes (``%`` -> ``(?s:.*)``, ``_`` -> ``(?s:.)`` on a
binary column and ``(?s:.)[\\x80-\\xbf]*(?![\\x80-\\xbf])`` on utf8, anything
else escaped) and every row is put to ``fullmatch``.
"""
from __future__ import annotations

import re
from typing import List, Optional

import numpy as np

from nvme_strom_amd.ops import colpred as CP
from nvme_strom_amd.utils.arrow_ipc import Column
from qualgen import (GEOMETRY, VALIDITY, Batch, DeviceTable, Table, expected_words,  # noqa: F401
                     host_values, make_valid, pack_words, popcount, row_bytes, valid_words,
                     values_bytes)

# 1-, 2-, 3- and 4-byte characters, the three specials, a newline, digits
UNIT = "héllo wörld €uro 😀smile 日本語 a_b%c\\d\nxyz 0123 "
MASTER = (UNIT * 120).encode()
assert len(MASTER) >= 5000
LENGTHS = list(range(10)) + [15, 16, 17, 40, 255, 256, 257, 1000, 5000]
# the 64 two-byte tokens of the segment-limit pattern, and a row holding them
TOKENS = [b"%c%c" % (0x41 + k // 8, 0x30 + k % 8) for k in range(CP.MAX_LIKE_SEGMENTS)]
TOKEN_ROW = b"..".join(TOKENS)


def column(dt: str, utf8: bool, name: str = "c") -> Column:
    return Column(name, "utf8" if utf8 else "binary", nbuffers=3, large=dt == "s8")


def _cut(src: bytes, start: int, n: int, utf8: bool) -> bytes:
    """n bytes of src from start; on utf8 a character the cut would split is
    replaced by as many 'x' (rows stay valid UTF-8 at their exact length)."""
    if not utf8:
        return src[start:start + n]
    while start < len(src) and (src[start] & 0xC0) == 0x80:
        start += 1
    r = src[start:start + n]
    k = len(r)
    while k and (r[k - 1] & 0xC0) == 0x80:
        k -= 1
    if k and r[k - 1] >= 0xC0:                      # a lead byte: is its character whole?
        need = 2 if r[k - 1] < 0xE0 else 3 if r[k - 1] < 0xF0 else 4
        if len(r) - (k - 1) < need:
            r = r[:k - 1] + b"x" * (len(r) - k + 1)
    return r


def like_rows(utf8: bool, rng) -> List[bytes]:
    rows = []
    for L in LENGTHS:
        rows.append(_cut(MASTER, 0, L, utf8))
        rows.append(b"a" * L)
        if L < 1000:
            rows.append(_cut(MASTER, 7, L, utf8))                 # starts at "wörld"
            rows.append(_cut(MASTER, len(UNIT.encode()) - 9, L, utf8))   # "xyz 0123 héllo ..."
            rows.append(b"a" * max(L - 1, 0) + b"b" * min(L, 1))  # aaab
            rows.append((b"aab" * (L // 3 + 1))[:L])
            rows.append((b"ab" * (L // 2 + 1))[:L])
    rows += [b"aba", b"abba", b"ab", b"ba", b"abab", b"aaab", b"aabaab", "日本語".encode(),
             "héllo".encode(), "h\nllo".encode(), b"a_b%c\\d", b"a_b", b"axb", b"%", b"_", b"\\",
             b"\n", TOKEN_ROW, b"xx" + TOKEN_ROW + b"yy", TOKEN_ROW[:-1], b"..".join(TOKENS[:-1]),
             "é".encode(), "€".encode(), "😀".encode(), "a😀b".encode(), "😀😀".encode()]
    if not utf8:
        rows += [bytes([0x80, 0x81]), bytes([0xC3]), bytes([0x61, 0xA9, 0xA9, 0x62]),
                 bytes(rng.integers(0, 256, 33, dtype=np.uint8))]
    return rows


def like_table(dt: str, utf8: bool, rng, malformed: bool = False, geometry=GEOMETRY,
               validity=VALIDITY, rows: Optional[List[bytes]] = None) -> Table:
    """Every row of like_rows() at every start alignment 0-3 of the character
    buffer (a filler row of 0x80-0xBF bytes before it sets the alignment),
    dealt over the batches of ``geometry`` and repeated to fill them; the
    last row of a batch ends exactly at its aux_len.  ``malformed``: three
    offsets of every batch of four rows or more are replaced by a negative
    one, one past the characters and one below its predecessor."""
    rows = like_rows(utf8, rng) if rows is None else rows
    short = [r for r in rows if len(r) <= 40]
    order = [(r, a) for a in range(4) for r in rows]
    order = [order[i] for i in rng.permutation(len(order))]
    at, batches = 0, []
    for n, mode in zip(geometry, validity):
        offs, chars = [0], bytearray()
        while len(offs) - 1 < n:
            if at < len(order):
                r, a = order[at]
            else:                                   # all placed: short rows fill the rest
                r, a = short[int(rng.integers(len(short)))], int(rng.integers(4))
            at += 1
            pad = (a - len(chars)) % 4
            if pad and len(offs) + 1 < n:
                chars += bytes(rng.integers(0x80, 0xC0, pad, dtype=np.uint8))
                offs.append(len(chars))
            chars += r
            offs.append(len(chars))
        offs = np.array(offs, np.int64)
        if malformed and n >= 4:
            offs[n // 4] = -3
            offs[n // 2] = len(chars) + (64 if dt == "s4" else (1 << 33) + 5)
            offs[3 * n // 4] = offs[3 * n // 4 - 1] - 1
        batches.append(Batch(n, (offs, np.frombuffer(bytes(chars), np.uint8)),
                             make_valid(n, mode, rng), mode))
    assert at >= len(order), "geometry too small for the rows"
    return Table(dt, batches)


# ---------------------------------------------------------------- reference
def like_regex(pat: bytes, utf8: bool):
    out, i = [], 0
    while i < len(pat):
        ch = pat[i:i + 1]
        if ch == b"\\":
            out.append(re.escape(pat[i + 1:i + 2]))
            i += 2
            continue
        if ch == b"%":
            out.append(b"(?s:.*)")
        elif ch == b"_":
            out.append(b"(?s:.)[\\x80-\\xbf]*(?![\\x80-\\xbf])" if utf8 else b"(?s:.)")
        else:
            out.append(re.escape(ch))
        i += 1
    return re.compile(b"".join(out))


def _esc(x: bytes) -> bytes:
    return re.sub(rb"([\\%_])", rb"\\\1", x)


def ref_patterns(op: str, value) -> List[bytes]:
    """The LIKE patterns a predicate stands for."""
    enc = lambda x: x.encode() if isinstance(x, str) else bytes(x)
    base = op[4:] if op.startswith("not ") else op
    if base == "like":
        return [enc(value)]
    vs = value if isinstance(value, (list, tuple)) else [value]
    return [b"%" + _esc(enc(x)) + (b"%" if base == "contains" else b"") for x in vs]


def like_ref(t: Table, op: str, value, utf8: bool, neg: bool = False) -> List[np.ndarray]:
    """Per batch bool[nrows]: rows the predicate selects (nulls and rows with
    a malformed offset pair cleared, negated or not)."""
    rxs = [like_regex(p, utf8) for p in ref_patterns(op, value)]
    neg = neg != op.startswith("not ")
    memo, out = {}, []
    for b in t.batches:
        ok = np.ones(b.nrows, bool) if b.valid is None else b.valid.copy()
        hit = np.zeros(b.nrows, bool)
        for i in range(b.nrows):
            x = row_bytes(b, i)
            if x is None:
                continue
            if x not in memo:
                memo[x] = any(rx.fullmatch(x) is not None for rx in rxs)
            hit[i] = memo[x] != neg
        out.append(hit & ok)
    return out


# ------------------------------------------------------------------ patterns
def like_preds(utf8: bool):
    """(name, op, value) of every pattern class; the values are str on a utf8
    column and bytes on a binary one."""
    v = (lambda s: s) if utf8 else (lambda s: s.encode())
    long_lit = MASTER[:300].decode()
    out = [
        # anchoring combinations
        ("x", "like", v("héllo")), ("x%", "like", v("hé%")), ("%x", "like", v("%llo")),
        ("%x%", "like", v("%wör%")), ("x%y", "like", v("hé%x")), ("%x%y%", "like", v("%llo%€u%")),
        ("x%y%z", "like", v("hé%wör%€")), ("x%y%z-2", "like", v("xyz%12%llo")),
        # _ at the start, in the middle, at the end of a segment, over multi-byte characters
        ("_x", "like", v("_éllo%")), ("x_y", "like", v("h_llo%")), ("x_", "like", v("%wör_")),
        ("%_x%", "like", v("%_uro%")), ("%x_y%", "like", v("%w_rld%")), ("%x_%", "like", v("%smile _%")),
        ("%x__y", "like", v("%l__w%")), ("_%_", "like", v("_%_")), ("x%_", "like", v("h%_")),
        ("%x_y_z%", "like", v("% _smile _本_ %")), ("4byte", "like", v("a_b")),
        ("tail_", "like", v("%hé_")), ("tail__x", "like", v("%__o")), ("head__", "like", v("__l%")),
        # only _s, the empty pattern, only %
        ("_", "like", v("_")), ("___", "like", v("___")), ("_"*9, "like", v("_" * 9)),
        ("empty", "like", v("")), ("%", "like", v("%")), ("%%", "like", v("%%")),
        ("%_%", "like", v("%_%")), ("%___%", "like", v("%___%")),
        # escapes
        ("esc", "like", v("%a\\_b\\%c\\\\d%")), ("esc-exact", "like", v("a\\_b\\%c\\\\d")),
        ("esc%", "like", v("\\%")), ("esc_", "like", v("\\_")), ("esc\\", "like", v("\\\\")),
        ("esc-mixed", "like", v("a_b\\%c%")),
        # a segment longer than the row, a tail that would overlap the head
        ("long-seg", "contains", v(long_lit)), ("overlap", "like", v("ab%ba")),
        ("overlap_", "like", v("a_%_a")), ("overlap2", "like", v("aab%aab")),
        # needles that are prefixes of themselves
        ("%aab%", "like", v("%aab%")), ("%aaab", "like", v("%aaab")), ("%abab%", "like", v("%abab%")),
        ("%aa_b%", "like", v("%aa_b%")), ("%aab%aab%", "like", v("%aab%aab%")),
        ("%a%b%a%", "like", v("%a%b%a%")), ("a%a%a", "like", v("a%a%a")),
        ("%aaaaaaab", "like", v("%" + "a" * 40 + "b")),
        # the other spellings: literal constants, lists, the empty constant
        ("contains", "contains", v("wör")), ("contains-sp", "contains", v("a_b%c\\d")),
        ("contains-list", "contains", [v("😀s"), v("日本"), v("zzz")]),
        ("contains-empty", "contains", v("")), ("suffix", "suffix", v("llo")),
        ("suffix-list", "suffix", [v("0123 "), v("b"), v("語")]), ("suffix-empty", "suffix", v("")),
        ("suffix-sp", "suffix", v("%c\\d")), ("not-contains", "not contains", v("wör")),
        ("not-suffix", "not suffix", v("llo")), ("not-like", "not like", v("h_llo%")),
        # the largest operands the compiler accepts
        ("max-bytes", "like", v("%" + "a" * (CP.MAX_LIKE_BYTES - 2) + "%")),
        ("max-segs", "like", v("%" + "%".join(t.decode() for t in TOKENS) + "%")),
        ("max-pats", "contains", [v("%c%c%c" % (0x61 + k % 3, 0x61 + k // 3 % 3, 0x30 + k // 9))
                                  for k in range(CP.MAX_LIKE_PATTERNS - 2)] + [v("wör"), v("aab")]),
    ]
    if not utf8:
        out += [("bin_", "like", b"a_\xa9b"), ("bin-hi", "like", b"%\x80_"),
                ("bin-c3", "like", b"h\xc3_llo%"), ("bin__", "like", b"h__llo%")]
    return out


PRED_NAMES = {True: [p[0] for p in like_preds(True)], False: [p[0] for p in like_preds(False)]}


def compile_like(op: str, value, dt: str, utf8: bool, neg: bool = False) -> CP.Compiled:
    c = CP.compile_pred(CP.Pred("c", op, value), column(dt, utf8))
    if neg:
        c.flags ^= CP.FLAG_NEGATE
    return c


class HostTable:
    """The batches' buffers in host memory (each padded to 8 bytes, as Arrow
    buffers are) and the (n, 7) strom_qual_batch table of their addresses:
    what colpred.like_host takes."""

    def __init__(self, t: Table):
        self.keep, rows = [], []

        def buf(raw: bytes) -> int:
            a = np.frombuffer(raw + b"\0" * (-len(raw) % 8 or (8 if not raw else 0)), np.uint8).copy()
            self.keep.append(a)
            return a.ctypes.data
        for k, b in enumerate(t.batches):
            chars = np.asarray(b.values[1], np.uint8)
            vw = valid_words(b)
            rows.append([buf(values_bytes(t.dt, b)), buf(vw.tobytes()) if vw is not None else 0,
                         b.nrows, t.word_base[k], t.row_base[k], buf(chars.tobytes()), len(chars)])
        self.qtab = np.array(rows, dtype=np.uint64).reshape(-1, 7)
        self.nwords = t.nwords


# ------------------------------------------------------------- whole scans
WORDS = ["", "a", "ab", "abc", "green", "dark green", "greenish", "special requests",
         "special packages and requests", "héllo", "hello", "日本語", "日本", "a_b", "axb", "50%",
         "50% off", "line\nbreak", "back\\slash", "😀 smile", "zz" * 13, "x" * 300 + "green"]


def arrow_table(n: int = 6000, seed: int = 9):
    """Valid UTF-8 in a string, a large_string, a binary and a
    dictionary-encoded column, nulls in three of them, and a number."""
    import pyarrow as pa
    rng = np.random.default_rng(seed)
    pick = lambda: [WORDS[k] for k in rng.integers(0, len(WORDS), n)]
    nulls = lambda: rng.random(n) < 0.07
    s, b = pick(), pick()
    return pa.table({
        "s": pa.array(s, mask=nulls()),
        "ls": pa.array(pick(), pa.large_string()),
        "bin": pa.array([x.encode() for x in b], pa.binary(), mask=nulls()),
        "dict": pa.array(pick(), mask=nulls()).dictionary_encode(),
        "v": pa.array(rng.integers(0, 1000, n)),
    })


def pc_mask(tbl, col: str, op: str, value) -> np.ndarray:
    """The rows pyarrow.compute selects (nulls: not selected, negated or
    not); a dictionary column is decoded first (no match_like kernel for it)."""
    import pyarrow as pa
    import pyarrow.compute as pc
    a = tbl.column(col).combine_chunks()
    if pa.types.is_dictionary(a.type):
        a = a.dictionary_decode()
    neg, base = op.startswith("not "), op[4:] if op.startswith("not ") else op
    enc = (lambda x: x.encode() if isinstance(x, str) else x) if pa.types.is_binary(a.type) \
        else (lambda x: x)
    if base == "like":
        m = pc.match_like(a, enc(value))
    else:
        fn = pc.match_substring if base == "contains" else pc.ends_with
        vs = value if isinstance(value, (list, tuple)) else [value]
        m = fn(a, enc(vs[0]))
        for x in vs[1:]:
            m = pc.or_(m, fn(a, enc(x)))
    if neg:
        m = pc.invert(m)
    return np.asarray(m.fill_null(False))


# (label, op, value): run on every string column of arrow_table()
SCAN_PREDS = [
    ("like-req", "like", "%special%requests%"), ("like-green", "like", "%green"),
    ("like-h_llo", "like", "h_llo"), ("like-3", "like", "___"), ("like-a_b", "like", "a\\_b"),
    ("like-pct", "like", "50\\%%"), ("like-head", "like", "gr%n%"), ("like-nl", "like", "line_break"),
    ("like-all", "like", "%"), ("like-empty", "like", ""), ("like-jp", "like", "日_%"),
    ("like-emoji", "like", "_ smile"), ("contains", "contains", "een"),
    ("contains-list", "contains", ["本", "%", "zzz"]), ("contains-empty", "contains", ""),
    ("endswith", "suffix", "green"), ("endswith-list", "suffix", ["s", "語", "_b"]),
    ("endswith-empty", "suffix", ""), ("not-like", "not like", "%green%"),
    ("not-contains", "not contains", "a"), ("not-suffix", "not suffix", "o"),
]
