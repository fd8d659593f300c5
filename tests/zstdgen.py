"""Zstandard stream builder, plain reference decoder and the hand-built
corpora of the zstd decoder edge tests (test_zstdstreams_cpu.py,
test_gpu_zstdstreams.py).  No project imports: the streams are written from
RFC 8878, so they hold what no encoder in the suite emits (window
descriptors, non-minimal size fields, RLE tables of wide codes, the
"repeat offset 1 minus one" code) and put every construct where the
decoders' own constants say an edge is.

A stream is described once and read twice: ``build_stream`` turns the
description into compressed bytes, ``decode`` into the bytes it must decode
to (plain copy loops).

stream:   [frame | ("skip", nibble, bytes), ...]
frame:    ("frame", [block, ...], {header options})
block:    ("raw", bytes) | ("rle", byte, n) |
          ("comp", literals, [(ll, offset | ("rep", 1..3), ml), ...], tables)
literals: ("raw", bytes[, fmt]) | ("rle", byte, n[, fmt]) |
          ("huf", bytes, {opts}) | ("treeless", bytes, {opts})
tables:   None | {"ll" | "of" | "ml": "predef" | "rle" | "repeat" |
                  ("fse", accuracy_log[, norm])[, "nseq_form": 1 | 2 | 3]
                  [, "marker": 0..7]}
The literals of a block are the literal runs of its sequences back to back
plus the trailing literals; an integer offset is the distance itself.

The valid builders raise ValueError on anything the format forbids (with
``strict=False`` they write the field as asked: the malformed corpus);
``raw_*`` emit unchecked pieces.
"""
import struct

import numpy as np

try:
    import xxhash

    def _xxh64(b):
        return xxhash.xxh64_intdigest(bytes(b), 0)
    HAVE_XXH = True
except Exception:  # without it no frame carries a checksum (the families say so)
    HAVE_XXH = False

# ---------------------------------------------------------------- constants
# The decoders' own constants, csrc/kernels/zstd.hip (line of the definition):
SEQN = 128            # :76/:90   sequences per decode chunk (wave, fp)
OB = 1024             # :88/:91   output bytes per resolve batch
LSYM = 256            # :94       literal symbols per stream per round
LWIN = 384            # :95       literal window: LSYM x <= 11 bits
MAXB = 128 << 10      # :96       Block_Maximum_Size
KPOSMAX = 1 << 30     # :101      kPosMax: outputs and offsets below 1 GiB
NWMAX = 8             # :1483     most waves of a frame-parallel group
KMAXSEQ = MAXB // 3   # :1484     kMaxSeq
LP_LSYM = 128         # :2234     lane-parallel: literal symbols per round
LP_SEQN = 64          # :2236     lane-parallel: sequences per round
LPLB = 4              # :2232/:2466  literal sections per wave (ZS_LPB)
LPSB = 6              # :2469     sequence sections per wave
LPX_OB = 4096         # :2989     lane-parallel execution batch
FPW = 4               # :3203     blocks in flight per frame (fp)

MAGIC = 0xFD2FB528
SKIP_MAGIC = 0x184D2A50

LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048,
                             4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027,
                                2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
NORM_LL = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1,
           1, 1, 1, -1, -1, -1, -1]
NORM_ML = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
NORM_OF = [1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5
PREDEF = {"ll": (NORM_LL, 6), "of": (NORM_OF, 5), "ml": (NORM_ML, 6)}
MAX_SYM = {"ll": 35, "of": 31, "ml": 52}
MAX_AL = {"ll": 9, "of": 8, "ml": 9}
KINDS = ("ll", "of", "ml")


def _rnd(rng, n):
    return rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()


def _need(ok, msg, strict=True):
    if strict and not ok:
        raise ValueError(msg)


# ---------------------------------------------------------------- bit writers
class FwdBits:
    """Forward bit writer: the first value put sits in the lowest bits."""

    def __init__(self):
        self.v = self.k = self.n = 0      # pending bits, their count, bits put in all
        self.out = bytearray()

    def put(self, val, nb):
        if not 0 <= val < (1 << nb):
            raise ValueError("value %d in %d bits" % (val, nb))
        self.v |= val << self.k
        self.k += nb
        self.n += nb
        if self.k >= 64:                  # whole bytes out: the pending value stays small
            self.out += (self.v & ((1 << (self.k & ~7)) - 1)).to_bytes(self.k >> 3, "little")
            self.v >>= self.k & ~7
            self.k &= 7

    def bytes(self):
        return bytes(self.out) + self.v.to_bytes((self.k + 7) // 8, "little")


def backward_stream(items, marker=None, slack_bits=0):
    """A backward bitstream from its fields in the order the decoder reads
    them, (value, bit count) each, closed by the final-bit marker.  The
    marker's bit position in the last byte follows from the bit total;
    ``marker`` = 0..7 insists on one and raises when the fields do not put
    it there.  ``slack_bits`` > 0 (malformed corpus only) puts that many
    zero bits under the fields: a stream with bits left over."""
    w = FwdBits()
    w.put(0, slack_bits)
    for val, nb in reversed(items):
        w.put(val, nb)
    if marker is not None and w.n % 8 != marker:
        raise ValueError("marker falls on bit %d, not %d" % (w.n % 8, marker))
    w.put(1, 1)
    return w.bytes()


def marker_bit(stream):
    return stream[-1].bit_length() - 1


# ------------------------------------------------------------------------ FSE
def fse_header(norm, al, strict=True):
    """The normalised-count header (RFC 8878 4.1.1) of ``norm`` (-1 = "less
    than 1") at accuracy log ``al``; zero runs become repeat flags."""
    _need(5 <= al <= 9, "accuracy log %d" % al, strict)
    _need(sum(abs(x) for x in norm) == 1 << al, "counts do not sum to the table size", strict)
    _need(norm and norm[-1] != 0, "the last count is not zero", strict)
    w = FwdBits()
    w.put(al - 5, 4)
    remaining, threshold, nbits = (1 << al) + 1, 1 << al, al + 1
    sym, prev0 = 0, False
    while sym < len(norm) and (remaining > 1 or not strict):
        if prev0:
            z = 0
            while sym + z < len(norm) and norm[sym + z] == 0:
                z += 1
            sym += z
            while z >= 3:
                w.put(3, 2)
                z -= 3
            w.put(z, 2)
            if sym >= len(norm):
                break
        count = norm[sym]
        mx = 2 * threshold - 1 - remaining
        v = count + 1
        if v < mx:
            w.put(v, nbits - 1)                   # the low form
        else:
            w.put(v + mx if v >= threshold else v, nbits)
        remaining -= abs(count)
        sym += 1
        prev0 = count == 0
        while remaining < threshold and threshold > 1:
            nbits -= 1
            threshold >>= 1
    _need(sym == len(norm) and remaining == 1, "counts end early", strict)
    return w.bytes()


class FseTable:
    """A decoding table (RFC 8878 4.1.1: spread, then state numbering);
    rows[state] = (symbol, bits, baseline)."""

    def __init__(self, norm, al):
        size = 1 << al
        self.al, self.norm = al, list(norm)
        cell = [None] * size
        high = size - 1
        nxt = {}
        for s, c in enumerate(norm):
            if c == -1:
                cell[high] = s
                high -= 1
                nxt[s] = 1
            else:
                nxt[s] = c
        pos, step = 0, (size >> 1) + (size >> 3) + 3
        for s, c in enumerate(norm):
            for _ in range(max(c, 0)):
                cell[pos] = s
                pos = (pos + step) & (size - 1)
                while pos > high:
                    pos = (pos + step) & (size - 1)
        if pos != 0 or None in cell:
            raise ValueError("spread does not close")
        self.rows = []
        for u in range(size):
            s = cell[u]
            nx = nxt[s]
            nxt[s] += 1
            nb = al - (nx.bit_length() - 1)
            self.rows.append((s, nb, (nx << nb) - size))
        self.by_sym = {}
        for u, (s, nb, base) in enumerate(self.rows):
            self.by_sym.setdefault(s, []).append((base, nb, u))

    @classmethod
    def rle(cls, sym):
        t = cls.__new__(cls)
        t.al, t.norm, t.rows, t.by_sym = 0, None, [(sym, 0, 0)], {sym: [(0, 0, 0)]}
        return t

    def states(self, syms, pick=0, last_needs_bits=False):
        """The states that decode ``syms`` in order and the (value, bits)
        each state update reads: (states, updates), len(updates) =
        len(syms) - 1.  The last state is free: ``pick`` chooses among the
        symbol's states."""
        for s in syms:
            if s not in self.by_sym:
                raise ValueError("symbol %d has no probability" % s)
        cands = self.by_sym[syms[-1]]
        if last_needs_bits:
            cands = [c for c in cands if c[1] > 0]
            if not cands:
                raise ValueError("no state of symbol %d reads bits" % syms[-1])
        st = [cands[pick % len(cands)][2]]         # built backwards
        ups = []
        for s in reversed(syms[:-1]):
            for base, nb, u in self.by_sym[s]:
                if base <= st[-1] < base + (1 << nb):
                    ups.append((st[-1] - base, nb))
                    st.append(u)
                    break
            else:
                raise AssertionError("no state of %d reaches %d" % (s, st[-1]))
        return st[::-1], ups[::-1]


def normalize(hist, al):
    """Counts summing to 1 << al, every present symbol >= 1."""
    total, size = sum(hist), 1 << al
    if sum(1 for h in hist if h) > size:
        raise ValueError("more symbols than states")
    norm = [max(1, h * size // total) if h else 0 for h in hist]
    while norm and norm[-1] == 0:
        norm.pop()
    big = max(range(len(norm)), key=lambda i: norm[i])
    norm[big] += size - sum(norm)
    if norm[big] < 1:
        raise ValueError("cannot normalise")
    return norm


# -------------------------------------------------------------------- Huffman
def huf_flat_lengths(symbols):
    """Code lengths of a complete prefix code over ``symbols``, as flat as
    it goes (the later symbols get the longer codes)."""
    n = len(symbols)
    if n < 2:
        raise ValueError("a Huffman alphabet has at least 2 symbols")
    k = (n - 1).bit_length()
    short = (1 << k) - n
    return {s: (k - 1 if i < short else k) for i, s in enumerate(sorted(symbols))}


def huf_weights(lengths, strict=True):
    """Weights of symbols 0..last-1 from {symbol: code length}; the last
    symbol's weight is implied (RFC 8878 4.2.1)."""
    mx = max(lengths.values())
    _need(1 <= mx <= 11, "code length above 11", strict)
    _need(len(lengths) >= 2, "fewer than 2 symbols", strict)
    _need(sum(1 << (mx - l) for l in lengths.values()) == 1 << mx, "code is not complete", strict)
    last = max(lengths)
    return [mx + 1 - lengths[s] if s in lengths else 0 for s in range(last)], mx


def huf_codes(lengths):
    """{symbol: (code, length)}: decode-table order, by weight then symbol."""
    mx = max(lengths.values())
    pos, codes = 0, {}
    for w in range(1, mx + 1):
        for s in sorted(lengths):
            if mx + 1 - lengths[s] == w:
                codes[s] = (pos >> (w - 1), lengths[s])
                pos += 1 << (w - 1)
    return codes


def huf_header(lengths, mode=None, al=6, strict=True):
    """The tree description: ``mode`` "direct" (4-bit weights) or "fse"
    (default: direct when the weights fit its 128)."""
    weights, _ = huf_weights(lengths, strict)
    nw = len(weights)
    if mode is None:
        mode = "direct" if nw <= 128 else "fse"
    if mode == "direct":
        _need(1 <= nw <= 128, "%d weights do not fit the direct form" % nw, strict)
        ws = weights + [0]
        return bytes([127 + nw]) + bytes((ws[i] << 4) | ws[i + 1] for i in range(0, nw, 2))
    _need(nw >= 2, "an FSE weight stream holds at least 2 weights", strict)
    hist = [0] * 13
    for x in weights:
        hist[x] += 1
    norm = normalize(hist, al)
    tab = FseTable(norm, al)
    # two interleaved states: even weights on the first, odd on the second;
    # the update after the last but one weight over-reads, so its state
    # must read bits (RFC 8878 4.2.1.2)
    ev, od = weights[0::2], weights[1::2]
    last_is_even = (nw - 1) % 2 == 0
    se, ue = tab.states(ev, last_needs_bits=not last_is_even)
    so, uo = tab.states(od, last_needs_bits=last_is_even)
    items = [(se[0], al), (so[0], al)]
    for i in range(max(len(ue), len(uo))):
        if i < len(ue):
            items.append(ue[i])
        if i < len(uo):
            items.append(uo[i])
    body = fse_header(norm, al) + backward_stream(items)
    _need(len(body) < 128, "FSE weight description of %d bytes" % len(body), strict)
    return bytes([len(body)]) + body


def huf_stream(codes, data, marker=None):
    return backward_stream([codes[b] for b in data], marker)


def huf_payload(codes, data, streams, markers=None, strict=True):
    """1 stream, or the jump table and 4 streams."""
    markers = markers or [None] * 4
    if streams == 1:
        return huf_stream(codes, data, markers[0])
    _need(len(data) >= 6, "4 streams need at least 6 literals", strict)
    seg = (len(data) + 3) // 4
    parts = [huf_stream(codes, data[i * seg:(i + 1) * seg] if i < 3 else data[3 * seg:], markers[i])
             for i in range(4)]
    _need(all(len(p) < 65536 for p in parts[:3]), "stream above 64 KiB", strict)
    return struct.pack("<HHH", *(len(p) & 0xFFFF for p in parts[:3])) + b"".join(parts)


# ----------------------------------------------------------- literals section
def raw_lit_header(kind, fmt, regen, comp=0):
    """kind 0 raw, 1 RLE: fmt 0 = 1 byte (5 bits; the format is one bit,
    the bit above it is the size's lowest), 1 = 2 bytes (12), 3 = 3 bytes (20).  kind 2 Huffman, 3 treeless: fmt 0 = 1 stream and 1 =
    4 streams (10 + 10 bits), 2 = 14 + 14, 3 = 18 + 18.  Unchecked."""
    if kind <= 1:
        if fmt == 0:
            return bytes([(kind | regen << 3) & 0xFF])
        v = kind | fmt << 2 | regen << 4
        return (v & 0xFFFFFF).to_bytes(2 if fmt == 1 else 3, "little")
    bits = (10, 10, 14, 18)[fmt]
    v = kind | fmt << 2 | (regen & ((1 << bits) - 1)) << 4 | (comp & ((1 << bits) - 1)) << (4 + bits)
    return v.to_bytes((3, 3, 4, 5)[fmt], "little")


def lit_header(kind, regen, comp=0, fmt=None, streams=None, strict=True):
    if kind <= 1:
        room = {0: 32, 1: 4096, 3: 1 << 20}
        if fmt is None:
            fmt = 0 if regen < 32 else 1 if regen < 4096 else 3
        _need(fmt in room, "size format %r" % fmt, True)
        _need(regen < room[fmt], "%d literals in size format %d" % (regen, fmt), strict)
    else:
        room = {0: 1024, 1: 1024, 2: 1 << 14, 3: 1 << 18}
        if fmt is None:
            big = max(regen, comp)
            fmt = (0 if streams == 1 else 1) if big < 1024 else 2 if big < 1 << 14 else 3
        _need((fmt == 0) == (streams == 1), "size format %d with %s streams" % (fmt, streams), strict)
        _need(regen < room[fmt] and comp < room[fmt], "sizes do not fit format %d" % fmt, strict)
    _need(regen <= MAXB, "more literals than a block holds", strict)
    return raw_lit_header(kind, fmt, regen, comp)


class FrameState:
    """What a frame carries from block to block."""

    def __init__(self):
        self.rep = [1, 4, 8]
        self.pos = 0           # frame output so far
        self.tabs = {}         # kind -> FseTable of the last block with sequences
        self.huf = None        # code lengths of the last Huffman literal section


def literals_section(st, spec, strict=True):
    """(section bytes, literal bytes) of a literals spec."""
    kind = spec[0]
    if kind == "raw":
        data = bytes(spec[1])
        return lit_header(0, len(data), fmt=spec[2] if len(spec) > 2 else None, strict=strict) + data, data
    if kind == "rle":
        n = spec[2]
        _need(n >= 1, "an RLE literal section of 0 bytes", strict)
        return lit_header(1, n, fmt=spec[3] if len(spec) > 3 else None, strict=strict) + bytes([spec[1]]), \
            bytes([spec[1]]) * n
    data = bytes(spec[1])
    o = dict(spec[2]) if len(spec) > 2 else {}
    streams = o.get("streams", 1 if len(data) < 6 else 4)
    if kind == "huf":
        lengths = o.get("lengths") or huf_flat_lengths(set(data) if len(set(data)) > 1
                                                       else set(data) | {(data[0] + 1) % 256})
        desc = huf_header(lengths, o.get("weights"), o.get("al", 6), strict)
        st.huf = lengths
    elif kind == "treeless":
        _need(st.huf is not None, "treeless literals without an earlier tree", strict)
        lengths, desc = st.huf or o.get("lengths"), b""
    else:
        raise ValueError(kind)
    _need(all(b in lengths for b in data), "literal outside the alphabet", strict)
    pay = huf_payload(huf_codes(lengths), data, streams, o.get("markers"), strict)
    comp = len(desc) + len(pay)
    return lit_header(2 if kind == "huf" else 3, len(data), comp, o.get("fmt"), streams, strict) + desc + pay, data


# ---------------------------------------------------------- sequences section
def raw_nseq(n, form):
    """Number_of_Sequences in the 1-, 2- or 3-byte form, unchecked."""
    if form == 1:
        return bytes([n & 0xFF])
    if form == 2:
        return bytes([((n >> 8) + 128) & 0xFF, n & 0xFF])
    return b"\xff" + struct.pack("<H", (n - 0x7F00) & 0xFFFF)


def nseq_field(n, form=None, strict=True):
    """The forms do not overlap above 127: 2 bytes reach 0x7EFF, 3 bytes
    begin at 0x7F00 (the bias); only n < 128 has a second spelling."""
    if form is None:
        form = 1 if n < 128 else 2 if n < 0x7F00 else 3
    ok = {1: n < 128, 2: n < 0x7F00, 3: 0x7F00 <= n <= 0x7F00 + 0xFFFF}[form]
    _need(ok, "%d sequences in the %d-byte form" % (n, form), strict)
    return raw_nseq(n, form)


def _code(base, v):
    c = len(base) - 1
    while base[c] > v:
        c -= 1
    return c


def ll_code(v):
    c = _code(LL_BASE, v)
    return c, v - LL_BASE[c], LL_BITS[c]


def ml_code(v):
    c = _code(ML_BASE, v)
    return c, v - ML_BASE[c], ML_BITS[c]


def of_code(ov):
    c = ov.bit_length() - 1
    return c, ov - (1 << c), c


def apply_offset(rep, spec, ll, strict=True):
    """(offset value written, actual distance, repeat offsets after) for an
    offset spec under RFC 8878 3.1.2.5."""
    if isinstance(spec, tuple):
        k = spec[1]
        _need(spec[0] == "rep" and k in (1, 2, 3), "repeat code %r" % (spec,), True)
        idx = k - 1 + (1 if ll == 0 else 0)
        if idx == 0:
            return k, rep[0], list(rep)
        if idx == 1:
            return k, rep[1], [rep[1], rep[0], rep[2]]
        if idx == 2:
            return k, rep[2], [rep[2], rep[0], rep[1]]
        _need(rep[0] - 1 >= 1, "repeat offset 1 minus one is 0", strict)
        return k, rep[0] - 1, [rep[0] - 1, rep[0], rep[1]]
    _need(spec >= 1, "offset %d" % spec, strict)
    return spec + 3, spec, [spec, rep[0], rep[1]]


def sequences_section(st, seqs, tables, nlit, strict=True):
    """The section's bytes; advances st.rep / st.pos past the block."""
    tables = tables or {}
    n = len(seqs)
    if n == 0:
        _need(not any(k in tables for k in KINDS), "tables without sequences", strict)
        st.pos += nlit
        return nseq_field(0, tables.get("nseq_form"), strict)
    codes = {k: [] for k in KINDS}
    extra = []
    used = out = 0
    for ll, off, ml in seqs:
        _need(ml >= 3, "match length %d" % ml, strict)
        ov, dist, st.rep = apply_offset(st.rep, off, ll, strict)
        used += ll
        out += ll
        _need(dist <= st.pos + out, "offset %d with %d bytes produced" % (dist, st.pos + out), strict)
        out += ml
        a, b, c = ll_code(ll), of_code(ov), ml_code(ml)
        codes["ll"].append(a[0])
        codes["of"].append(b[0])
        codes["ml"].append(c[0])
        extra.append((b[1:], c[1:], a[1:]))
    _need(used <= nlit, "sequences use %d of %d literals" % (used, nlit), strict)
    _need(out + nlit - used <= MAXB, "block output above Block_Maximum_Size", strict)
    st.pos += out + nlit - used
    head, tabs, modes = b"", {}, 0
    for i, k in enumerate(KINDS):
        spec = tables.get(k, "predef")
        if spec == "predef":
            m, tabs[k] = 0, FseTable(*PREDEF[k])
        elif spec == "rle":
            _need(len(set(codes[k])) == 1, "RLE table over several %s codes" % k, strict)
            m, tabs[k] = 1, FseTable.rle(codes[k][0])
            head += bytes([codes[k][0]])
        elif spec == "repeat":
            _need(k in st.tabs, "repeat mode without an earlier %s table" % k, strict)
            m, tabs[k] = 3, st.tabs.get(k) or FseTable(*PREDEF[k])
        else:
            al = spec[1]
            _need(5 <= al <= MAX_AL[k], "%s accuracy log %d" % (k, al), strict)
            if len(spec) > 2 and spec[2] is not None:
                norm = list(spec[2])
            else:
                hist = [0] * (MAX_SYM[k] + 1)
                for c in codes[k]:
                    hist[c] += 1
                if sum(1 for h in hist if h) == 1:      # one symbol: a second keeps it an FSE table
                    hist[(codes[k][0] + 1) % 8] += 1
                norm = normalize(hist, al)
            _need(len(norm) <= MAX_SYM[k] + 1, "%s symbol above its maximum" % k, strict)
            m, tabs[k] = 2, FseTable(norm, al)
            head += fse_header(norm, al, strict)
        modes |= m << (6 - 2 * i)
    st.tabs = tabs
    sts, ups = {}, {}
    for k in KINDS:
        sts[k], ups[k] = tabs[k].states(codes[k], tables.get("pick", 0))
    items = [(sts[k][0], tabs[k].al) for k in KINDS]
    for i in range(n):
        items += list(extra[i])
        if i + 1 < n:
            items += [ups["ll"][i], ups["ml"][i], ups["of"][i]]
    return nseq_field(n, tables.get("nseq_form"), strict) + bytes([modes]) + head + \
        backward_stream(items, tables.get("marker"))


# ------------------------------------------------------------ blocks, frames
def raw_block_header(btype, size, last):
    return ((last & 1) | (btype & 3) << 1 | size << 3).to_bytes(3, "little")


def block_bytes(st, blk, last, strict=True):
    kind = blk[0]
    if kind == "raw":
        _need(len(blk[1]) <= MAXB, "raw block above Block_Maximum_Size", strict)
        st.pos += len(blk[1])
        return raw_block_header(0, len(blk[1]), last) + bytes(blk[1])
    if kind == "rle":
        _need(0 <= blk[2] <= MAXB, "RLE block above Block_Maximum_Size", strict)
        st.pos += blk[2]
        return raw_block_header(1, blk[2], last) + bytes([blk[1]])
    if kind == "bytes":            # a ready block, header and all (malformed corpus)
        return blk[1]
    _, lits, seqs, tables = blk
    sec, data = literals_section(st, lits, strict)
    body = sec + sequences_section(st, seqs, tables, len(data), strict)
    _need(len(body) < MAXB, "compressed block of %d bytes" % len(body), strict)
    return raw_block_header(2, len(body), last) + body


def raw_frame_header(desc_byte, window=None, did=b"", fcs=b""):
    return struct.pack("<I", MAGIC) + bytes([desc_byte]) + (b"" if window is None else bytes([window])) + did + fcs


def window_byte(size):
    """The smallest window descriptor covering ``size`` bytes."""
    for e in range(32):
        for m in range(8):
            if (1 << (10 + e)) + ((1 << (10 + e)) >> 3) * m >= size:
                return e << 3 | m
    raise ValueError(size)


def frame_bytes(blocks, single=None, fcs_bytes=None, fcs=None, did_bytes=0, did=0, checksum=False,
                window=None, strict=True):
    """One frame.  single: Single_Segment (None: set when every block fits
    the content size, the window of such a frame); fcs_bytes: 0 / 1 / 2 / 4
    / 8 (None: the smallest, or 0 with a window); fcs: the value written
    (None: the truth); window: the descriptor byte."""
    _need(blocks, "a frame has at least one block", strict)
    st = FrameState()
    body = [block_bytes(st, b, i == len(blocks) - 1, strict) for i, b in enumerate(blocks)]
    content = decode_frame(blocks) if strict else None
    n = len(content) if strict else st.pos
    if single is None:
        single = window is None and all(len(b) - 3 <= n for b in body) and \
            all(b[0] != "rle" or b[2] <= n for b in blocks)
    _need(not single or all(len(b) - 3 <= n for b in body), "a block above the content size, "
          "the window of a single-segment frame", strict)
    if fcs_bytes is None:
        fcs_bytes = (1 if n < 256 else 2 if n < 65792 else 4) if single else 0
    val = n if fcs is None else fcs
    _need(fcs_bytes in ((1, 2, 4, 8) if single else (0, 2, 4, 8)), "FCS of %d bytes" % fcs_bytes, strict)
    _need(did_bytes in (0, 1, 2, 4), "dictionary id of %d bytes" % did_bytes, strict)
    _need(did == 0, "dictionaries are out of scope", strict)
    if fcs_bytes == 2:
        _need(256 <= val < 65792, "%d in the 2-byte FCS" % val, strict)
        f = struct.pack("<H", (val - 256) & 0xFFFF)
    else:
        _need(fcs_bytes == 0 or val < 1 << (8 * fcs_bytes), "%d in %d FCS bytes" % (val, fcs_bytes), strict)
        f = (val & ((1 << (8 * fcs_bytes)) - 1)).to_bytes(fcs_bytes, "little")
    flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes]
    desc = flag << 6 | (0x20 if single else 0) | (4 if checksum else 0) | {0: 0, 1: 1, 2: 2, 4: 3}[did_bytes]
    if not single and window is None:
        window = window_byte(max([n] + [len(b) - 3 for b in body]))
    _need(single or not strict or
          (1 << (10 + (window >> 3))) // 8 * (8 + (window & 7)) >= max(len(b) - 3 for b in body),
          "a block above the window size", strict)
    out = raw_frame_header(desc, None if single else window, did.to_bytes(did_bytes, "little"), f) + b"".join(body)
    if checksum:
        _need(HAVE_XXH, "no xxhash", True)
        out += struct.pack("<I", _xxh64(content if content is not None else b"") & 0xFFFFFFFF)
    return out


def skippable(nibble, data):
    if not 0 <= nibble <= 15:
        raise ValueError("skippable magic")
    return struct.pack("<II", SKIP_MAGIC + nibble, len(data)) + bytes(data)


def build_stream(stream, strict=True):
    out = []
    for it in stream:
        if it[0] == "skip":
            out.append(skippable(it[1], it[2]))
        elif it[0] == "frame":
            out.append(frame_bytes(it[1], strict=strict, **(it[2] if len(it) > 2 else {})))
        else:
            raise ValueError(it[0])
    return b"".join(out)


def arrow_zstd(buffer_len, payload):
    """An Arrow IPC compressed buffer: int64 length prefix + zstd frame(s);
    buffer_len -1 = the stored form (``payload`` is then the raw bytes)."""
    return struct.pack("<q", buffer_len) + payload


# ------------------------------------------------------------------ reference
def decode_frame(blocks):
    """What a frame's blocks decode to: plain copy loops, the repeat-offset
    rules of RFC 8878 3.1.2.5."""
    o = bytearray()
    rep = [1, 4, 8]
    for blk in blocks:
        if blk[0] == "raw":
            o += blk[1]
        elif blk[0] == "rle":
            o += bytes([blk[1]]) * blk[2]
        else:
            lits = blk[1]
            data = bytes([lits[1]]) * lits[2] if lits[0] == "rle" else bytes(lits[1])
            lp = 0
            for ll, off, ml in blk[2]:
                o += data[lp:lp + ll]
                lp += ll
                _, dist, rep = apply_offset(rep, off, ll)
                assert 1 <= dist <= len(o), (dist, len(o))
                if dist >= ml:
                    o += o[len(o) - dist:len(o) - dist + ml]
                else:
                    for _ in range(ml):
                        o.append(o[-dist])
            o += data[lp:]
    return bytes(o)


def decode(stream):
    return b"".join(decode_frame(it[1]) for it in stream if it[0] == "frame")


# --------------------------------------------------------------------- cases
class Case:
    """name; comp: the stream; exp: its output; arrow: behind the Arrow
    prefix (codec ARROW_ZSTD); lp: the lane-parallel path takes it (one data
    frame, nothing after it, not stored: lp_walk, zstd.hip:2399-2457; no
    content checksum, which the serial decoder verifies: zstd.hip:3293-3294)."""

    def __init__(self, name, comp, exp, arrow=False, lp=True, nblk=1, nent=0):
        self.name, self.comp, self.exp, self.arrow, self.lp = name, comp, exp, arrow, lp
        self.cap = len(exp)
        self.nblk, self.nent = nblk, nent      # blocks, and sequences + 1 of each compressed one


def lp_fits(items):
    """Whether one lane-parallel launch lists every block and holds every
    entry of ``items`` (Case / Bad): its block list has room for capacity /
    32 KiB + 4 per stream + 64 blocks, its entry pool for 3 bytes per byte
    of capacity + 4 KiB in the host twin, the smaller of the two (zstd.hip
    :3702-3704 and :3775-3776; an entry is 16 bytes, :1488).  Past either,
    which streams fall back depends on the order of the walks."""
    cap = sum(c.cap for c in items)
    return sum(c.nblk for c in items) <= cap // 32768 + 4 * len(items) + 64 and \
        16 * sum(c.nent for c in items) <= 3 * cap + 4096


def lp_batches(items):
    """``items`` in launches that lp_fits (greedy, in order; all in one when
    that fits)."""
    if lp_fits(items):
        return [list(items)]
    out = [[]]
    for c in items:
        if out[-1] and not lp_fits(out[-1] + [c]):
            out.append([])
        out[-1].append(c)
    return out


def _walkable(stream):
    kinds = [it[0] for it in stream]
    return kinds.count("frame") == 1 and kinds[-1] == "frame" and \
        not (len(stream[-1]) > 2 and stream[-1][2].get("checksum"))


def case(name, stream, arrow=False):
    exp = decode(stream)
    comp = build_stream(stream)
    if arrow:
        comp = arrow_zstd(len(exp), comp)
    blks = [b for it in stream if it[0] == "frame" for b in it[1]]
    return Case(name, comp, exp, arrow, _walkable(stream), len(blks),
                sum(len(b[2]) + 1 for b in blks if b[0] == "comp"))


def one(name, blocks, **opts):
    return case(name, [("frame", blocks, opts)])


def simple_block(rng, nlit=40, seqs=None, tables=None, lits=None):
    """A small compressed block: raw literals and three ordinary matches."""
    seqs = seqs if seqs is not None else [(7, 5, 9), (3, 12, 4), (0, ("rep", 1), 6)]
    return ("comp", lits or ("raw", _rnd(rng, nlit)), seqs, tables)


# --------------------------------------------------------------------- frames
def frames(seed=501):
    """Frame headers: every FCS width at its first and last values, window
    descriptors, zero dictionary-ID fields, checksums, the empty frame,
    skippable frames around data frames, several data frames, and all of it
    behind the Arrow prefix."""
    rng = np.random.default_rng(seed)
    out = []
    for n in (0, 1, 255, 256, 65791, 65792):
        data = _rnd(rng, n)
        for fb in (1, 2, 4, 8):
            if (fb == 1 and n > 255) or (fb == 2 and not 256 <= n < 65792):
                continue
            out.append(one("fcs%d_b%d" % (n, fb), [("raw", data)], fcs_bytes=fb, single=True))
        for fb in (0, 2, 4, 8):
            if fb == 2 and not 256 <= n < 65792:
                continue
            out.append(one("win_fcs%d_b%d" % (n, fb), [("raw", data)], fcs_bytes=fb, single=False))
    blk = lambda: simple_block(rng)
    for db in (1, 2, 4):
        out.append(one("did0_b%d" % db, [blk()], did_bytes=db))
        out.append(one("did0_b%d_win" % db, [blk()], did_bytes=db, single=False))
    if HAVE_XXH:
        for n in (0, 31, 32, 33, 5000):
            out.append(one("cksum%d" % n, [("raw", _rnd(rng, n))], checksum=True))
        out.append(one("cksum_comp", [blk(), ("rle", 7, 100), blk()], checksum=True))
        out.append(one("cksum_win", [blk()], checksum=True, single=False))
    out.append(one("empty", [("raw", b"")]))
    out.append(one("empty_win", [("raw", b"")], single=False))
    f = lambda **o: ("frame", [blk(), ("raw", _rnd(rng, 33))], o)
    sk0, sk9 = ("skip", 0, b""), ("skip", 9, _rnd(rng, 9))
    for nib in range(16):
        out.append(case("skip_magic%x" % nib, [("skip", nib, _rnd(rng, nib)), f()]))
    out.append(case("skip0_before", [sk0, f()]))
    out.append(case("skip_after", [f(), sk9]))
    out.append(case("skip0_after", [f(), sk0]))
    out.append(case("skip_between", [f(), sk9, f()]))
    out.append(case("skip_everywhere", [sk0, sk9, f(), sk0, f(), sk9, sk0]))
    out.append(case("skip_only", [sk9]))
    # later frames begin with fresh repeat offsets: their first sequences use them
    reps = lambda: ("frame", [("comp", ("raw", _rnd(rng, 30)),
                               [(9, ("rep", 1), 5), (5, ("rep", 2), 4), (9, ("rep", 3), 7), (0, 2, 3)], None)], {})
    moved = lambda: ("frame", [simple_block(rng, 60, [(20, 17, 5), (9, 13, 4), (9, 11, 3)])], {})
    out.append(case("frames2_fresh_reps", [moved(), reps()]))
    out.append(case("frames3_fresh_reps", [moved(), reps(), reps()]))
    out.append(case("frames2_win_then_single", [("frame", [blk()], {"single": False}), f()]))
    if HAVE_XXH:
        out.append(case("frames3_cksum", [f(checksum=True), f(), f(checksum=True)]))
    out += [Case("arrow_" + c.name, arrow_zstd(len(c.exp), c.comp), c.exp, True, c.lp, c.nblk, c.nent) for c in list(out)]
    for n in (0, 1, 15, 16, 17, 4097):
        raw = _rnd(rng, n)
        out.append(Case("arrow_stored%d" % n, arrow_zstd(-1, raw), raw, True, False))
    return out


# --------------------------------------------------------------------- blocks
def blocks(seed=502):
    """Raw and RLE blocks of 0, 1 and MAXB bytes; a compressed block of
    exactly MAXB output; each type last; each plain type between two
    compressed blocks that share history, repeat offsets and tables."""
    rng = np.random.default_rng(seed)
    out = []
    for n in (0, 1, MAXB):
        out.append(one("raw%d" % n, [("raw", _rnd(rng, n))]))
        out.append(one("rle%d" % n, [("rle", 0x5A, n)], single=n >= 1))
        out.append(one("raw%d_then_comp" % n, [("raw", _rnd(rng, n)), simple_block(rng)]))
        out.append(one("rle%d_mid" % n, [simple_block(rng), ("rle", 3, n), simple_block(rng)]))
    lits = _rnd(rng, 2000)
    out.append(one("comp_out_maxb", [("comp", ("raw", lits), [(1000, 999, MAXB - 2000)], None)]))
    out.append(one("comp_out_maxb_lits", [("comp", ("rle", 0x42, MAXB - 3), [(MAXB - 3, 1, 3)], None)]))
    out.append(one("last_raw", [simple_block(rng), ("raw", _rnd(rng, 50))]))
    out.append(one("last_rle", [simple_block(rng), ("rle", 9, 50)]))
    out.append(one("last_comp", [("raw", _rnd(rng, 50)), simple_block(rng)]))
    hl = {s: l for s, l in zip(range(40, 48), (1, 2, 3, 4, 5, 6, 7, 7))}
    for mid_name, mid in (("raw", ("raw", _rnd(rng, 77))), ("rle", ("rle", 0xEE, 77)),
                          ("raw0", ("raw", b"")), ("rle0", ("rle", 1, 0))):
        syms = bytes(rng.choice(list(hl), 64).astype(np.uint8))
        first = ("comp", ("huf", syms, {"lengths": hl}), [(20, 19, 5), (20, 7, 5), (9, 3, 5)],
                 {"ll": ("fse", 6, NORM_LL), "of": ("fse", 5, NORM_OF), "ml": "rle"})
        # after the plain block: the tree, the three tables and all three
        # repeat offsets of the first block, and a match into each block
        third = ("comp", ("treeless", syms[::-1]),
                 [(20, ("rep", 3), 5), (20, ("rep", 2), 5), (9, ("rep", 1), 5), (0, 64 + 40, 5)],
                 {"ll": "repeat", "of": "repeat", "ml": "repeat"})
        out.append(one("survive_" + mid_name, [first, mid, third]))
    return out


# ------------------------------------------------------------------- literals
def _syms(rng, lengths, n, only=None):
    pool = sorted(only if only is not None else lengths)
    return bytes(rng.choice(pool, int(n)).astype(np.uint8))


LEN11 = {s: l for s, l in zip(range(100, 112), (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 11))}


def literals(seed=503):
    """Literal sections: every header format, 1 and 4 Huffman streams around
    each decoder's round (LSYM 256 x 1 or 4 streams; LP_LSYM 128 x 4), small
    and 11-bit alphabets, symbol 255, 128 direct weights, every marker
    position, treeless after each kind of block, literals-only blocks."""
    rng = np.random.default_rng(seed)
    out = []
    tail = [(2, 1, 3)]

    def lb(name, spec, seqs=None, pre=None):
        data_len = spec[2] if spec[0] == "rle" else len(spec[1])
        seqs = tail if seqs is None else seqs
        seqs = [s for s in seqs if s[0] <= data_len][:1] if data_len < 2 else seqs
        out.append(one(name, (pre or []) + [("comp", spec, seqs if data_len >= 2 else [], None)]))

    for n, fmts in ((0, (0, 1, 3)), (1, (0, 1, 3)), (30, (0, 1, 3)), (31, (0, 1, 3)), (32, (1, 3)),
                    (4095, (1, 3)), (4096, (3,)), (MAXB - 16, (3,)), (MAXB - 3, (3,))):
        for fmt in fmts:
            if n <= MAXB - 16:        # raw, more would not fit a block next to the sequence
                lb("raw%d_f%d" % (n, fmt), ("raw", _rnd(rng, n), fmt), [] if n == 0 else None)
            if n:
                lb("rle%d_f%d" % (n, fmt), ("rle", 0xC3, n, fmt))
    flat = huf_flat_lengths(range(30, 47))                      # 17 symbols: lengths 4 and 5
    for R in (6, 7, 8, 9, 10, 11, 12, 13):
        lb("huf4_R%d" % R, ("huf", _syms(rng, flat, R), {"lengths": flat, "streams": 4}))
    for R in (2, 5, LP_LSYM - 1, LP_LSYM, LP_LSYM + 1, LSYM - 1, LSYM, LSYM + 1, 2 * LSYM + 1, 1023):
        lb("huf1_R%d" % R, ("huf", _syms(rng, flat, R), {"lengths": flat, "streams": 1}))
    for R in (4 * LP_LSYM - 1, 4 * LP_LSYM, 4 * LP_LSYM + 1, 4 * LSYM - 1, 4 * LSYM, 4 * LSYM + 1,
              8 * LSYM - 1, 8 * LSYM, 8 * LSYM + 1, 4 * LSYM - 3, 4 * LSYM - 4):
        for fmt in (1, 2, 3) if R == 4 * LP_LSYM else (2, 3) if R == 4 * LSYM else (None,):
            lb("huf4_R%d_f%s" % (R, fmt), ("huf", _syms(rng, flat, R), {"lengths": flat, "streams": 4, "fmt": fmt}))
    lb("huf4_R16383_f2", ("huf", _syms(rng, flat, 16383), {"lengths": flat, "streams": 4, "fmt": 2}))
    lb("huf4_R16384_f3", ("huf", _syms(rng, flat, 16384), {"lengths": flat, "streams": 4, "fmt": 3}))
    two = {7: 1, 200: 1}
    for streams, R in ((1, 3), (1, LSYM + 1), (4, 6), (4, 4 * LSYM + 1)):
        lb("huf2sym_s%d_R%d" % (streams, R), ("huf", _syms(rng, two, R), {"lengths": two, "streams": streams}))
    # whole rounds of 11-bit codes: the literal window's bound (LWIN,
    # LP_LWIN); then mixed lengths
    for streams, R in ((1, LSYM), (1, 2 * LSYM + 3), (4, 4 * LSYM), (4, 8 * LSYM + 5), (4, 4 * LP_LSYM)):
        lb("huf11_all11_s%d_R%d" % (streams, R),
           ("huf", _syms(rng, LEN11, R, (110, 111)), {"lengths": LEN11, "streams": streams}))
        lb("huf11_mixed_s%d_R%d" % (streams, R),
           ("huf", _syms(rng, LEN11, R), {"lengths": LEN11, "streams": streams}))
    with255 = {0: 2, 1: 2, 2: 2, 255: 2}
    lb("huf_sym255_fse", ("huf", _syms(rng, with255, 300), {"lengths": with255}))
    with255b = dict(huf_flat_lengths(list(range(0, 250, 5)) + [255]))
    lb("huf_sym255_51syms_fse", ("huf", _syms(rng, with255b, 1500), {"lengths": with255b}))
    for al in (5, 6):
        lb("huf_fse_weights_al%d" % al,
           ("huf", _syms(rng, LEN11, 400), {"lengths": LEN11, "weights": "fse", "al": al}))
    all256 = {s: 8 for s in range(256)}
    all256.update({0: 7, 1: 7, 252: 9, 253: 9, 254: 9, 255: 9})
    lb("huf_256syms_fse", ("huf", bytes(range(256)) * 3, {"lengths": all256}))
    for nw in (127, 128):           # direct weights, odd and even counts, up to the form's 128
        ln = huf_flat_lengths(range(nw + 1))
        lb("huf_direct%d" % nw, ("huf", _syms(rng, ln, 700), {"lengths": ln, "weights": "direct"}))
    lb("huf_direct1", ("huf", _syms(rng, {0: 1, 1: 1}, 50), {"lengths": {0: 1, 1: 1}, "weights": "direct"}))
    # every marker position on every stream: the literals are drawn until
    # the stream's bit total lands there
    for streams in (1, 4):
        for m in range(8):
            data = b""
            for _ in range(streams):
                while True:
                    seg = _syms(rng, flat, 41)
                    if sum(flat[b] for b in seg) % 8 == m:
                        break
                data += seg
            lb("huf%d_marker%d" % (streams, m),
               ("huf", data, {"lengths": flat, "streams": streams, "markers": [m] * 4}))
    # treeless after ...
    h = lambda n=80: ("comp", ("huf", _syms(rng, flat, n), {"lengths": flat}), [(5, 3, 4)], None)
    t = lambda n=80, s=None: ("comp", ("treeless", _syms(rng, flat, n), {"streams": s or 4}), [(5, 2, 4)], None)
    rawlit = ("comp", ("raw", _rnd(rng, 20)), [(5, 2, 4)], None)
    rlelit = ("comp", ("rle", 4, 20), [(5, 2, 4)], None)
    out.append(one("treeless_after_huf", [h(), t()]))
    out.append(one("treeless_after_rawlit", [h(), rawlit, t()]))
    out.append(one("treeless_after_rlelit", [h(), rlelit, t()]))
    out.append(one("treeless_after_rawblock", [h(), ("raw", _rnd(rng, 30)), t()]))
    out.append(one("treeless_after_rleblock", [h(), ("rle", 8, 30), t()]))
    out.append(one("treeless_after_treeless", [h(), t(), t(300), t(5, 1)]))
    out.append(one("treeless_after_new_tree", [h(), ("comp", ("huf", _syms(rng, LEN11, 99), {"lengths": LEN11}),
                                                     [(5, 2, 4)], None),
                                               ("comp", ("treeless", _syms(rng, LEN11, 99)), [(1, 1, 3)], None)]))
    out.append(one("treeless_after_litonly", [("comp", ("huf", _syms(rng, flat, 80), {"lengths": flat}), [], None), t()]))
    # literals-only (nseq == 0) next to the same literals with one sequence
    for R in (LSYM - 1, 4 * LSYM + 1, 5000):
        data = _syms(rng, flat, R)
        for streams in (1, 4) if R < 1000 else (4,):
            spec = ("huf", data, {"lengths": flat, "streams": streams})
            out.append(one("litonly_s%d_R%d" % (streams, R), [("comp", spec, [], None)]))
            out.append(one("litonly_s%d_R%d_1seq" % (streams, R), [("comp", spec, [(R - 1, 4, 3)], None)]))
            out.append(one("litonly_s%d_R%d_mid" % (streams, R),
                           [("raw", _rnd(rng, 9)), ("comp", spec, [], None), simple_block(rng)]))
    out.append(one("litonly_raw", [("comp", ("raw", _rnd(rng, 300)), [], None)]))
    out.append(one("litonly_rle", [("comp", ("rle", 1, 300), [], None)]))
    return out


# ------------------------------------------------------------------ sequences
def _many(rng, n, ml=3):
    """n short sequences over a small literal pool."""
    return [(int(rng.integers(0, 3)), int(rng.integers(1, 9)), ml + int(rng.integers(0, 3))) for _ in range(n)]


def _blk_of(rng, seqs, tables=None, trailing=5, pre=8):
    seqs = [(seqs[0][0] + pre,) + tuple(seqs[0][1:])] + list(seqs[1:])
    nl = sum(s[0] for s in seqs) + trailing
    if nl > MAXB - 64:             # raw, they would not fit a block next to the sequences
        return ("comp", ("rle", 0x3C, nl), seqs, tables)
    return ("comp", ("raw", _rnd(rng, nl)), seqs, tables)


def sequences(seed=504):
    """Sequence counts around each decoder's round (SEQN 128, LP_SEQN 64),
    the count field's forms and the 0x7F00 bias, every LL / ML / OF code at
    its lowest and highest value, a full round of the widest fields (SWIN),
    every table mode and every marker position."""
    rng = np.random.default_rng(seed)
    out = []
    for n in (1, LP_SEQN - 1, LP_SEQN, LP_SEQN + 1, SEQN - 1, SEQN, SEQN + 1, 2 * SEQN - 1, 2 * SEQN,
              2 * SEQN + 1, 8 * LP_SEQN + 1):
        for tr in (0, 5):
            out.append(one("n%d_tr%d" % (n, tr), [_blk_of(rng, _many(rng, n), None, tr)]))
    for n in (1, 127):
        out.append(one("n%d_form2" % n, [_blk_of(rng, _many(rng, n), {"nseq_form": 2})]))
    out.append(one("n128_form2_first", [_blk_of(rng, _many(rng, 128))]))
    out.append(one("n0x7eff_form2_last", [_blk_of(rng, [(0, 1 + i % 4, 3) for i in range(0x7EFF)], None, 0)]))
    # 0x7F00 sequences of 3 bytes and 0x7F01 (the first with a non-zero field): minimal
    # matches, one block
    for n in (0x7F00, 0x7F01):
        out.append(one("n0x%x_form3" % n, [_blk_of(rng, [(0, 1 + i % 4, 3) for i in range(n)], None, 0)]))
    # kMaxSeq: the most sequences a block's output has room for
    out.append(one("n%d_kmaxseq" % KMAXSEQ, [_blk_of(rng, [(1, 1, 3)] + [(0, 1 + i % 4, 3) for i in range(KMAXSEQ - 1)],
                                                      None, 0, pre=0)]))
    # LL and ML codes: baseline and the highest value (the all-ones extra
    # bits; for the codes whose all-ones value cannot fit a block, the
    # highest the block allows)
    for c in range(36):
        for v in sorted({LL_BASE[c], min(LL_BASE[c] + (1 << LL_BITS[c]) - 1, MAXB - 3 - 8)}):
            out.append(one("ll_c%d_v%d" % (c, v), [_blk_of(rng, [(v, 2, 3)], None, 0)]))
    for c in range(53):
        for v in sorted({ML_BASE[c], min(ML_BASE[c] + (1 << ML_BITS[c]) - 1, MAXB - 8 - 5)}):
            out.append(one("ml_c%d_v%d" % (c, v), [_blk_of(rng, [(0, 5, v), (2, 1, 3)], None, 0)]))
    # offset codes: offset value 2^c and 2^(c + 1) - 1 behind enough history
    # (RLE blocks: 4 bytes each); code 18 at its lowest value reaches
    # 2^18 - 3 bytes back, the most here
    for c in range(2, 19):
        for ov in ((1 << c), (2 << c) - 1)[:1 if c == 18 else 2]:
            dist = ov - 3
            hist, pre = [], dist
            while pre > 8:
                k = min(pre - 8, MAXB)
                hist.append(("rle", 0x11 + len(hist), k))
                pre -= k
            out.append(one("of_c%d_ov%d" % (c, ov),
                           hist + [("comp", ("raw", _rnd(rng, pre + 4)), [(pre, dist, 9), (2, 1, 3)], None)]))
    # >= SEQN consecutive sequences each with the widest fields the history
    # allows: LL code 24 (4 bits; more would overflow the block), ML code 42
    # (5 bits), OF code 17 (17 bits) behind 2 x MAXB of RLE history, through
    # RLE tables (predefined OF ends at code 28 but LL 24 has 5-bit states)
    for n in (SEQN, SEQN + 3, 3 * LP_SEQN + 1):
        seqs = [(48 + int(rng.integers(0, 16)), (1 << 17) - 3 + int(rng.integers(0, 1 << 17)) % (1 << 17),
                 99 + int(rng.integers(0, 32))) for _ in range(n)]
        b = ("comp", ("raw", _rnd(rng, sum(s[0] for s in seqs) + 3)), seqs,
             {"ll": "rle", "of": "rle", "ml": "rle"})
        out.append(one("wide_round_n%d" % n, [("rle", 1, MAXB), ("rle", 2, MAXB), b]))
    # wider still, fewer: LL 16 bits is one sequence per block; ML code 46 (10 bits) x 100
    seqs = [(0, (1 << 17) - 3 + int(rng.integers(0, 1 << 17)), 1027 + int(rng.integers(0, 256))) for _ in range(100)]
    out.append(one("wide_ml10_of17_n100", [("rle", 1, MAXB), ("rle", 2, MAXB),
                                          ("comp", ("raw", _rnd(rng, 3)), seqs, {"of": "rle", "ml": "rle"})]))
    # table modes
    base = lambda: [(int(rng.integers(0, 16)), int(rng.integers(1, 5)), 3 + int(rng.integers(0, 30)))
                    for _ in range(150)]
    same = lambda ll, ov, ml, n=70: [(ll, ov, ml)] * n
    T = {"predef": None,
         "rle_zero_bits": (same(4, 1, 7), {"ll": "rle", "of": "rle", "ml": "rle"}),
         "rle_widest": ([(1024 + 7 * i, 4000 + i, 515 + i) for i in range(60)], {"ll": "rle", "of": "rle", "ml": "rle"}),
         "fse_min_al": (None, {"ll": ("fse", 5), "of": ("fse", 5), "ml": ("fse", 5)}),
         "fse_max_al": (None, {"ll": ("fse", 9), "of": ("fse", 8), "ml": ("fse", 9)})}
    for name, v in T.items():
        seqs, tabs = v if v else (None, None)
        seqs = seqs or base()
        pre = [("rle", 5, 8000)] if name == "rle_widest" else []
        out.append(one("mode_" + name, pre + [_blk_of(rng, seqs, tabs, pre=0 if name.startswith("rle") else 8)]))
    # maximum accuracy logs with "less than 1" probabilities and long zero
    # runs (3, 4 and 30+ zeros: the chained repeat flags)
    nll = [300, -1, 0, 0, 0, 100, 0, 0, 0, 0, 50, -1] + [0] * 12 + [60]
    nof = [-1, 200, 40, 0, 0, 0, 5, 0, 0, 0, 0, 0, 10]
    nml = [400, 0, 0, 0, 0, 0, 0, 100, -1, -1] + [0] * 33 + [10]
    assert sum(map(abs, nll)) == 512 and sum(map(abs, nof)) == 256 and sum(map(abs, nml)) == 512
    pick = lambda norm: [i for i, c in enumerate(norm) if c][int(rng.integers(0, sum(1 for c in norm if c)))]
    seqs, rep = [], [1, 4, 8]
    while len(seqs) < 140:
        lc, oc, mc = pick(nll), pick(nof), pick(nml)
        ll = LL_BASE[lc] + int(rng.integers(0, 1 << LL_BITS[lc]))
        ml = ML_BASE[mc] + int(rng.integers(0, 1 << ML_BITS[mc]))
        ov = (1 << oc) + int(rng.integers(0, 1 << oc))
        off = ("rep", ov) if ov <= 3 else ov - 3
        try:
            rep = apply_offset(rep, off, ll)[2]
        except ValueError:                      # "minus one" down to 0: drawn again
            continue
        seqs.append((ll, off, ml))
    out.append(one("mode_fse_max_al_lt1_zero_runs",
                   [("rle", 9, 9000), ("comp", ("raw", _rnd(rng, sum(s[0] for s in seqs) + 9)), seqs,
                                       {"ll": ("fse", 9, nll), "of": ("fse", 8, nof), "ml": ("fse", 9, nml)})]))
    # repeat after each mode, and after a repeat; across raw, RLE and nseq == 0 blocks
    fixed = [(4, 3, 7)] * 40
    for name, tabs in (("predef", None), ("rle", {"ll": "rle", "of": "rle", "ml": "rle"}),
                       ("fse", {"ll": ("fse", 6), "of": ("fse", 5), "ml": ("fse", 7)})):
        rp = {"ll": "repeat", "of": "repeat", "ml": "repeat"}
        mk = lambda t: _blk_of(rng, fixed, t, pre=0)
        out.append(one("repeat_after_%s" % name, [mk(tabs), mk(rp), mk(rp)]))
        for gap_name, gap in (("rawblock", ("raw", _rnd(rng, 40))), ("rleblock", ("rle", 2, 40)),
                              ("nseq0", ("comp", ("raw", _rnd(rng, 40)), [], None))):
            out.append(one("repeat_after_%s_across_%s" % (name, gap_name), [mk(tabs), gap, mk(rp)]))
    out.append(one("repeat_mixed", [mk({"ll": ("fse", 6), "of": "rle", "ml": "predef"}),
                                    mk({"ll": "repeat", "of": ("fse", 5), "ml": "repeat"}),
                                    mk({"ll": "rle", "of": "repeat", "ml": "repeat"})]))
    # the bitstream's marker on each bit of the last byte
    for m in range(8):
        while True:
            try:
                out.append(one("marker%d" % m, [_blk_of(rng, _many(rng, 9) + [(17 + m, 90, 40)], {"marker": m}, pre=90)]))
                break
            except ValueError:
                continue
    return out


# -------------------------------------------------------------------- offsets
def offsets(seed=505):
    """Repeat codes with and without literals, the rotation over long runs,
    offsets 1..65 and the frame position, matches into earlier blocks,
    matches and literals around the OB batch edge, doubling chains."""
    rng = np.random.default_rng(seed)
    out = []
    R = lambda k: ("rep", k)
    setup = [(9, 21, 4), (9, 14, 4), (9, 33, 4)]              # rep = 33, 14, 21
    for k in (1, 2, 3):
        for ll in (0, 6):
            out.append(one("rep%d_ll%d" % (k, ll), [_blk_of(rng, setup + [(ll, R(k), 5), (1, R(1), 3)], pre=40)]))
    out.append(one("rep3_ll0_chain", [_blk_of(rng, setup + [(0, R(3), 4)] * 20 + [(2, R(1), 3)], pre=40)]))
    for n in (3 * SEQN + 7,):
        seqs = list(setup)
        for i in range(n):
            ll = (0, 2, 0, 1)[i % 4] if i % 7 else 0
            k = (2, 3, 1, 3, 2, 2, 3)[i % 7]
            seqs.append((ll, R(k), 3 + i % 3))
        out.append(one("rep_rotation_n%d" % n, [_blk_of(rng, seqs, pre=40)]))
        # drawn codes (a draw the rules forbid, "minus one" down to 0, is drawn again)
        seqs, rep = list(setup), [33, 14, 21]
        while len(seqs) < n:
            ll, k = int(rng.integers(0, 2)) * int(rng.integers(1, 4)), int(rng.integers(1, 4))
            try:
                rep = apply_offset(rep, R(k), ll)[2]
            except ValueError:
                continue
            seqs.append((ll, R(k), 3 + len(seqs) % 2))
        out.append(one("rep_rotation_drawn_n%d" % n, [_blk_of(rng, seqs, pre=40)]))
    out.append(one("new_equals_rep", [_blk_of(rng, setup + [(2, 33, 4), (2, 14, 4), (0, 21, 4), (2, R(3), 5),
                                                             (0, R(1), 4)], pre=40)]))
    for ml in (3, 64, 1025, 5000):
        out.append(one("off1_ml%d" % ml, [_blk_of(rng, [(1, 1, ml), (3, 2, 4)], pre=0)]))
    for off in (2, 3, 4, 7, 63, 64, 65):
        out.append(one("off%d" % off, [_blk_of(rng, [(off, off, 3 * off + 5), (3, off, 3), (0, 1, 70)], pre=0)]))
    for pos in (1, 2, 100, OB, 5000):
        out.append(one("off_eq_pos%d" % pos, [_blk_of(rng, [(pos, pos, 10), (0, pos + 10, 2 * pos + 20)], pre=0)]))
        out.append(one("off_eq_pos%d_block2" % pos,
                       [("raw", _rnd(rng, pos)), _blk_of(rng, [(0, pos, 10), (4, pos + 14, 30)], pre=0)]))
    for prev_name, prev in (("raw", ("raw", _rnd(rng, 300))), ("rle", ("rle", 0x77, 300)),
                            ("comp", _blk_of(rng, _many(rng, 40), trailing=100))):
        n = len(decode_frame([prev]))
        for start in (n, 10, 1):                 # distance to the match's first byte
            out.append(one("cross_%s_o%d" % (prev_name, start),
                           [("raw", _rnd(rng, 50)), prev, _blk_of(rng, [(0, start, start + 40), (3, 2, 9)], pre=0)]))
    # a match / a literal run starting on output OB - 1, OB, OB + 1 of the
    # block (LPX_OB likewise), short and spanning into the next batch
    for ob in (OB, LPX_OB):
        for d in (-1, 0, 1):
            p = ob + d
            out.append(one("match_at%d" % p, [_blk_of(rng, [(600, 9, p - 600), (0, 7, 5), (9, 300, 2 * ob + 9)], pre=0)]))
            out.append(one("lits_at%d" % p, [_blk_of(rng, [(600, 9, p - 600), (ob + 50, 7, 5)], pre=0)]))
            out.append(one("match_spans_%d" % p, [_blk_of(rng, [(p - 20, 9, 40), (2, p - 5, 30)], pre=0)]))
    # one batch of short matches that each copy the match before: the
    # longest in-batch pointer chains
    for ml, off in ((3, 3), (4, 1), (3, 1), (5, 2)):
        seqs = [(3, 2, 3)] + [(0, off, ml)] * ((OB - 6) // ml + 2)
        out.append(one("chain_ml%d_off%d" % (ml, off), [_blk_of(rng, seqs, pre=0)]))
        seqs = [(3, 2, 3)] + [(0, off, ml)] * ((2 * LPX_OB) // ml)
        out.append(one("chain_ml%d_off%d_long" % (ml, off), [_blk_of(rng, seqs, pre=0)]))
    return out


# ------------------------------------------------------------------- fp_carry
def fp_carry(seed=506):
    """Frames of 2..9 small compressed blocks (around FPW 4 and NWMAX 8)
    whose blocks open on the repeat offsets the block before left: each
    code, with and without literals; blocks that make fewer than three new
    offsets, so an incoming offset crosses several blocks; plain and
    literals-only blocks between; repeat tables and treeless literals."""
    rng = np.random.default_rng(seed)
    out = []
    R = lambda k: ("rep", k)
    opens = [[(4, R(1), 4), (4, R(2), 4), (4, R(3), 5)],
             [(0, R(1), 4), (0, R(2), 4), (3, R(1), 3)],
             [(0, R(3), 4), (0, R(3), 3), (2, R(2), 5)],
             [(0, R(2), 3), (5, R(3), 4), (0, R(1), 6)],
             [(2, R(3), 7), (0, R(3), 3)],
             [(1, R(1), 3)]]
    first = lambda: _blk_of(rng, [(30, 29, 4), (9, 17, 4), (9, 23, 5)], pre=0)
    flat = huf_flat_lengths(range(60, 77))

    def mk(i, news, style):
        seqs = list(opens[i % len(opens)]) + [(3, 6 + (5 * i + j) % 20, 4) for j in range(news)]
        nl = sum(s[0] for s in seqs) + 4
        if style == "plain":
            return ("comp", ("raw", _rnd(rng, nl)), seqs, None)
        tabs = {"ll": "repeat", "of": "repeat", "ml": "repeat"}
        return ("comp", ("treeless", _syms(rng, flat, nl), {"streams": 1 if nl < 6 else 4}), seqs, tabs)

    for nb in (2, 3, FPW, FPW + 1, NWMAX, NWMAX + 1, 13, 2 * NWMAX + 1):
        for news in (3, 1, 0):
            out.append(one("carry_b%d_new%d" % (nb, news), [first()] + [mk(i, news, "plain") for i in range(nb - 1)]))
        gaps = [("comp", ("raw", _rnd(rng, 12)), [], None), ("raw", _rnd(rng, 12)), ("rle", 3, 12)]
        blks = [first()]
        for i in range(nb - 1):
            blks.append(mk(i, i % 2, "plain"))
            if i % 2 == 0:
                blks.append(gaps[(i // 2) % 3])
        out.append(one("carry_b%d_gaps" % nb, blks))
        h0 = ("comp", ("huf", _syms(rng, flat, 60), {"lengths": flat}), [(30, 29, 4), (9, 17, 4), (9, 23, 5)],
              {"ll": ("fse", 6, NORM_LL), "of": ("fse", 5, NORM_OF), "ml": ("fse", 6, NORM_ML)})
        out.append(one("carry_b%d_repeat_treeless" % nb, [h0] + [mk(i, (i + 1) % 2, "rt") for i in range(nb - 1)]))
        blks = [h0]
        for i in range(nb - 1):
            blks.append(mk(i, 0, "rt" if i % 3 else "plain"))
            if i % 3 == 1:
                blks.append(gaps[i % 3])
        out.append(one("carry_b%d_all" % nb, blks))
    # the "minus one" symbol carried through blocks that make no new offset
    out.append(one("carry_rep0_minus_k", [first()] + [("comp", ("raw", _rnd(rng, 2)), [(0, R(3), 3)] * 3, None)
                                                      for _ in range(6)]))
    return out


FAMILIES = {"frames": frames, "blocks": blocks, "literals": literals, "sequences": sequences,
            "offsets": offsets, "fp_carry": fp_carry}


def align_streams(seed=507):
    """A small mixed subset (a Huffman block with compressed tables, repeat
    codes, a raw block, an Arrow-prefixed frame): [Case]."""
    rng = np.random.default_rng(seed)
    flat = huf_flat_lengths(range(30, 47))
    b1 = ("comp", ("huf", _syms(rng, flat, 300), {"lengths": flat}),
          [(37, 5, 6), (120, 90, 300), (9, 1, 70), (0, ("rep", 2), 9), (30, 13, 4)],
          {"ll": ("fse", 6, NORM_LL), "of": ("fse", 5), "ml": ("fse", 6)})
    b2 = ("comp", ("treeless", _syms(rng, flat, 50)), [(10, ("rep", 1), 9), (0, ("rep", 3), 9)],
          {"ll": "repeat", "of": "predef", "ml": "rle"})
    return [one("align_huf", [b1]), one("align_3blocks", [b1, ("raw", _rnd(rng, 33)), b2]),
            case("align_arrow", [("frame", [b1, b2], {})], arrow=True),
            one("align_raw", [("raw", _rnd(rng, 101))])]


# ------------------------------------------------------------------ malformed
class Bad:
    """name; comp; cap: the capacity handed over; status: the exact code
    where the contract names one, else None (any negative); arrow."""

    def __init__(self, name, comp, cap, status=None, arrow=False, nblk=4, nent=200):
        self.name, self.comp, self.cap, self.status, self.arrow = name, comp, cap, status, arrow
        self.nblk, self.nent = nblk, nent      # upper bounds, for lp_fits


def _edit(b, pos, val):
    b = bytearray(b)
    b[pos] = val
    return bytes(b)


def malformed(seed=601):
    """Streams wrong in exactly one field, each a one-field edit of a valid
    one (or the same description built with strict=False)."""
    rng = np.random.default_rng(seed)
    out = []
    flat = huf_flat_lengths(range(30, 47))
    good_blocks = [simple_block(rng), ("raw", _rnd(rng, 20))]
    good = frame_bytes(good_blocks)
    n = len(decode_frame(good_blocks))
    add = lambda name, comp, cap=n, status=None, arrow=False: out.append(Bad(name, comp, cap, status, arrow))
    fr = lambda blocks, **o: frame_bytes(blocks, strict=False, **o)

    add("reserved_fhd_bit", _edit(good, 4, good[4] | 0x08))
    for db in (1, 2, 4):
        add("dict_id_b%d" % db, fr(good_blocks, did_bytes=db, did=1 << (8 * db - 1), single=True, fcs=n), n, -4)
    add("bad_magic", _edit(good, 0, 0x29))
    # block headers
    hdr = 4 + 1 + 1           # magic, descriptor, 1-byte FCS
    add("block_type3", _edit(good, hdr, good[hdr] | 0x06))
    big = _rnd(rng, MAXB + 1)
    add("block_size_gt_maxb", fr([("bytes", raw_block_header(0, MAXB + 1, 1) + big)], single=True, fcs_bytes=4,
                                 fcs=MAXB + 1), MAXB + 1)
    add("rle_block_gt_maxb", fr([("rle", 1, MAXB + 1)], single=True, fcs_bytes=4, fcs=MAXB + 1), MAXB + 1)
    add("block_output_gt_maxb", fr([("comp", ("raw", _rnd(rng, 10)), [(5, 2, MAXB)], None)], single=True,
                                   fcs_bytes=4, fcs=MAXB + 10), MAXB + 10)
    add("block_output_gt_maxb_lits", fr([("rle", 1, 100), ("comp", ("rle", 7, MAXB - 1), [(MAXB - 1, 2, 3)], None)],
                                        single=True, fcs_bytes=4, fcs=MAXB + 102), MAXB + 102)
    # content size and capacity
    add("fcs_too_small", fr(good_blocks, fcs=n - 1, fcs_bytes=1, single=True))
    add("fcs_too_large", fr(good_blocks, fcs=n + 1, fcs_bytes=1, single=True), n + 1)
    add("fcs_gt_cap", fr(good_blocks, fcs=n + 1, fcs_bytes=1, single=True), n, -2)
    add("fcs8_huge", fr(good_blocks, fcs=1 << 40, fcs_bytes=8, single=True), n, -2)
    add("cap_one_short", good, n - 1, -2)
    add("cap_one_short_nofcs", fr(good_blocks, single=False), n - 1, -2)
    add("cap_one_short_comp_last", fr([("raw", _rnd(rng, 20)), simple_block(rng)], single=False), n - 1, -2)
    add("cap_one_short_rle", fr([("rle", 4, 50)], single=False), 49, -2)
    add("cap_one_short_litonly", fr([("comp", ("huf", _syms(rng, flat, 80), {"lengths": flat}), [], None)],
                                    single=False), 79, -2)
    if HAVE_XXH:
        ck = frame_bytes(good_blocks, checksum=True)
        add("wrong_checksum", ck[:-1] + bytes([ck[-1] ^ 1]), n, -5)
        add("checksum_cut", ck[:-2], n)
    # distances
    add("off_pos_plus_1", fr([("comp", ("raw", _rnd(rng, 20)), [(10, 11, 5)], None)], fcs=25, single=True), 25, -3)
    add("off_pos_plus_1_block2", fr([("raw", _rnd(rng, 30)), ("comp", ("raw", _rnd(rng, 20)), [(10, 41, 5)], None)],
                                    fcs=55, single=True), 55, -3)
    add("off_pos_plus_1_chunk2", fr([_blk_of(rng, _many(rng, SEQN + 5) + [(0, 100000, 4)])], single=False),
        4000, -3)
    two = frame_bytes(good_blocks) + fr([("comp", ("raw", _rnd(rng, 20)), [(10, 11, 5)], None)], fcs=25, single=True)
    add("frame2_reaches_frame1", two, n + 25, -3)
    two = frame_bytes(good_blocks) + fr([("comp", ("raw", _rnd(rng, 20)), [(0, ("rep", 1), 5)], None)], fcs=25,
                                        single=True)
    add("frame2_rep_reaches_frame1", two, n + 25, -3)
    add("rep0_minus_1_is_0", fr([("comp", ("raw", _rnd(rng, 20)), [(5, 1, 4), (0, ("rep", 3), 4)], None)],
                                fcs=28, single=True), 28)
    add("rep0_minus_1_is_0_fresh", fr([("raw", _rnd(rng, 9)), ("comp", ("raw", _rnd(rng, 20)),
                                                             [(0, ("rep", 3), 4)], None)], fcs=33, single=True), 33)
    # tables and trees a frame does not have (yet)
    tl = ("comp", ("treeless", _syms(rng, flat, 50), {"lengths": flat}), [(5, 2, 4)], None)
    rp = lambda k: ("comp", ("raw", _rnd(rng, 20)), [(5, 2, 4)], {k: "repeat"})
    hf = ("comp", ("huf", _syms(rng, flat, 50), {"lengths": flat}), [(5, 2, 4)],
          {"ll": ("fse", 6), "of": ("fse", 5), "ml": ("fse", 6)})
    add("treeless_first", fr([tl], single=False), 54)
    add("treeless_after_raw_only", fr([("raw", _rnd(rng, 30)), simple_block(rng), tl], single=False), 200)
    for k in KINDS:
        add("repeat_%s_first" % k, fr([rp(k)], single=False), 24)
        add("repeat_%s_frame2" % k, frame_bytes([hf]) + fr([rp(k)], single=False), 54 + 24)
    add("repeat_after_nseq0_only", fr([("comp", ("raw", _rnd(rng, 9)), [], None), rp("of")], single=False), 33)
    add("treeless_frame2", frame_bytes([hf]) + fr([tl], single=False), 54 + 54)
    # table descriptions
    v = frame_bytes([_blk_of(rng, [(4, 1, 7)] * 9, {"ll": "rle", "of": "rle", "ml": "rle"}, pre=0)], single=False)
    p = v.index(bytes([9, 0x54])) + 2          # the sequence count, the modes, then the three symbols
    vn = 9 * 11 + 5
    assert v[p:p + 3] == bytes([4, 2, 4])
    add("rle_ll_sym36", _edit(v, p, 36), vn)
    add("rle_of_sym32", _edit(v, p + 1, 32), vn)
    add("rle_ml_sym53", _edit(v, p + 2, 53), vn)
    add("seq_modes_reserved", _edit(v, p - 1, 0x55), vn)
    add("seq_modes_reserved2", _edit(v, p - 1, 0x56), vn)
    v = frame_bytes([_blk_of(rng, [(4, 3, 7)] * 40, {"ll": ("fse", 9), "of": ("fse", 8), "ml": ("fse", 9)}, pre=0)],
                    single=False)
    vn = 40 * 11 + 5
    p = v.index(bytes([40, 0xA8])) + 2
    assert v[p] & 15 == 4
    add("ll_al_10", _edit(v, p, (v[p] & 0xF0) | 5), vn)
    q = p + len(fse_header(normalize([0] * 4 + [40, 1], 9), 9))
    assert v[q] & 15 == 3
    add("of_al_9", _edit(v, q, (v[q] & 0xF0) | 4), vn)
    add("ll_first_count_edit", _edit(v, p, v[p] | 0xF0), vn)
    # a count can say at most what is left of the table (the value's range
    # ends there), so a description overshoots through its symbols: a 37th
    body = fse_header([1] * 36 + [28], 6, strict=False)
    add("ll_counts_past_max_symbol", fr([("bytes", raw_block_header(2, 5 + len(body) + 2, 1) +
                                        raw_lit_header(0, 0, 3) + b"abc" + bytes([1, 0x80]) + body + b"\x01\x01")],
                                      single=False), 100)
    body = fse_header([10, 10], 5, strict=False)
    add("ll_counts_undershoot", fr([("bytes", raw_block_header(2, 5 + len(body) + 2, 1) +
                                     raw_lit_header(0, 0, 3) + b"abc" + bytes([1, 0x80]) + body + b"\x01\x01")],
                                   single=False), 100)
    # Huffman
    hb = frame_bytes([("comp", ("huf", _syms(rng, flat, 300), {"lengths": flat, "streams": 4}), [(5, 2, 4)], None)],
                     single=False)
    p = hb.index(bytes([127 + 46]))
    add("huf_weights_not_pow2", _edit(hb, p + 16, hb[p + 16] ^ 0x10), 304)
    add("huf_weight_12", _edit(hb, p + 16, 0xC0 | (hb[p + 16] & 15)), 304)
    jt = p + 1 + 23
    add("huf_jump_gt_section", hb[:jt] + struct.pack("<H", 2000) + hb[jt + 2:], 304)
    l1 = struct.unpack_from("<H", hb, jt)[0]
    add("huf_jump_shifted", hb[:jt] + struct.pack("<H", l1 + 1) + hb[jt + 2:], 304)
    add("huf_stream_zero_last_byte", _edit(hb, jt + 6 + l1 - 1, 0), 304)
    h1 = frame_bytes([("comp", ("huf", _syms(rng, flat, 100), {"lengths": flat, "streams": 1}), [(5, 2, 4)], None)],
                     single=False)
    p = h1.index(bytes([127 + 46]))
    R, C = 100, (int.from_bytes(h1[p - 3:p], "little") >> 14)
    add("huf1_stream_zero_last_byte", _edit(h1, p + C - 1, 0), 105)
    add("huf_regen_plus_1", h1[:p - 3] + raw_lit_header(2, 0, R + 1, C) + h1[p:], 105)
    add("huf_regen_minus_1", h1[:p - 3] + raw_lit_header(2, 0, R - 1, C) + h1[p:], 105)
    add("huf_4streams_R5", fr([("comp", ("huf", _syms(rng, flat, 5), {"lengths": flat, "streams": 4, "fmt": 1}),
                                [(5, 2, 4)], None)], single=False), 9)
    add("huf_one_weight_only", fr([("bytes", raw_block_header(2, 3 + 2 + 1 + 1, 1) + raw_lit_header(2, 0, 4, 3) +
                                    bytes([128, 0x10, 0x01, 0]))], single=False), 10)
    # sequence bitstream
    sq = frame_bytes([_blk_of(rng, [(4, 300, 7), (9, 77, 30), (2, 1, 3)], pre=400)], single=False)
    sn = 415 + 5 + 40
    add("seq_zero_last_byte", _edit(sq, len(sq) - 1, 0), sn)
    st = FrameState()
    sec = sequences_section(st, [(404, 300, 7), (9, 77, 30), (2, 1, 3)], None, 420)
    lit = raw_lit_header(0, 1, 420) + _rnd(rng, 420)
    mkb = lambda s: fr([("bytes", raw_block_header(2, len(lit) + len(s), 1) + lit + s)], single=False)
    assert mkb(sec)[:6] == sq[:6]
    add("seq_stream_short", mkb(sec[:-2] + b"\x01"), sn)      # the last 2 bytes gone, a marker put back
    add("seq_stream_long", mkb(sec[:2] + b"\xff" + sec[2:]), sn)
    add("seq_stream_cut_to_marker", mkb(sec[:2] + b"\x01"), sn)
    add("lits_used_gt_present", fr([("comp", ("raw", _rnd(rng, 10)), [(5, 2, 4), (6, 2, 4)], None)], single=False), 30)
    add("lits_used_gt_present_rle", fr([("comp", ("rle", 5, 10), [(11, 2, 4)], None)], single=False), 30)
    add("nseq0_then_bytes", fr([("bytes", raw_block_header(2, 6, 1) + raw_lit_header(0, 0, 3) + b"abc\x00\x00")],
                               single=False), 10)
    add("nseq_missing", fr([("bytes", raw_block_header(2, 4, 1) + raw_lit_header(0, 0, 3) + b"abc")], single=False), 10)
    add("nseq_gt_stream", mkb(bytes([100]) + sec[1:]), 5000)
    add("nseq_form3_no_stream", mkb(b"\xff\x00\x00" + sec[1:]), 200000)
    out[-1].nent = 0x7F00 + 1
    add("nseq_kmaxseq_plus_1", mkb(raw_nseq(KMAXSEQ + 1, 3) + sec[1:]), 200000)
    out[-1].nent = KMAXSEQ + 2
    # offsets of codes 30 and 31: at kPosMax and above, past any output
    for c in (30, 31):
        add("off_code%d" % c, fr([("comp", ("raw", _rnd(rng, 20)), [(5, (1 << c) - 3 + 77, 4)],
                                   {"of": "rle"})], single=False), 40, -3)
    add("match_len_past_maxb", fr([_blk_of(rng, [(4, 2, 65539 + 65535), (2, 1, 3)])], single=False), 140000)
    # truncation at every structural boundary of a three-block frame with a
    # checksum (or without it), and in the middle of each piece
    st = FrameState()
    tb = [("comp", ("huf", _syms(rng, flat, 60), {"lengths": flat}), [(20, 19, 5), (9, 3, 5)],
           {"ll": ("fse", 6), "of": ("fse", 5), "ml": "rle"}), ("rle", 6, 10), ("raw", _rnd(rng, 10))]
    whole = frame_bytes(tb, checksum=HAVE_XXH, single=True)
    tn = len(decode_frame(tb))
    blk0 = block_bytes(st, tb[0], False)
    lsec, _ = literals_section(FrameState(), tb[0][1])
    cuts = {0, 1, 4, 5, 6, 6 + 1, 6 + 3, 6 + 3 + 1, 6 + 3 + 3, 6 + 3 + 3 + 23, 6 + 3 + 3 + 24,
            6 + 3 + len(lsec) - 1, 6 + 3 + len(lsec), 6 + 3 + len(lsec) + 1, 6 + 3 + len(lsec) + 2,
            6 + len(blk0) - 1, 6 + len(blk0), 6 + len(blk0) + 2, 6 + len(blk0) + 3, 6 + len(blk0) + 4,
            6 + len(blk0) + 7, 6 + len(blk0) + 8, len(whole) - 4, len(whole) - 1}
    assert whole[:5] == raw_frame_header(0x20 | (4 if HAVE_XXH else 0))     # a 6-byte header
    for c in sorted(x for x in cuts if 0 <= x < len(whole)):
        if c == 0:
            continue                                  # an empty stream is valid: no frame at all
        add("trunc_at%d" % c, whole[:c], tn)
    sk = skippable(3, b"abcdef")
    add("skip_cut_header", good + sk[:6])
    add("skip_cut_body", good + sk[:-1])
    add("skip_len_huge", good + struct.pack("<II", SKIP_MAGIC, 0xFFFFFFF0))
    add("trailing_garbage", good + b"\x00")
    # the Arrow prefix
    add("arrow_prefix_gt_cap", arrow_zstd(n, good), n - 1, -2, True)
    add("arrow_prefix_gt_cap_frame_fits", arrow_zstd(n + 5, good), n, -2, True)
    add("arrow_prefix_huge", arrow_zstd(1 << 40, good), n, -2, True)
    add("arrow_prefix_lt_frame", arrow_zstd(n - 1, good), n, None, True)
    add("arrow_prefix_gt_frame", arrow_zstd(n + 1, good), n + 1, None, True)
    add("arrow_prefix_minus_2", arrow_zstd(-2, good), n, None, True)
    add("arrow_stored_gt_cap", arrow_zstd(-1, _rnd(rng, 100)), 99, -2, True)
    add("arrow_prefix_cut", arrow_zstd(n, good)[:7], n, None, True)
    return out


# which family's launch a malformed case rides in (test_gpu_zstdstreams.py):
# by the first matching prefix of its name
_BAD_FAMILY = [("treeless_frame2", "fp_carry"), ("repeat_ll_frame2", "fp_carry"), ("repeat_of_frame2", "fp_carry"),
               ("repeat_ml_frame2", "fp_carry"), ("frame2_", "fp_carry"), ("treeless_after_raw_only", "fp_carry"),
               ("block_", "blocks"), ("rle_block", "blocks"), ("nseq0_", "blocks"), ("nseq_missing", "blocks"),
               ("match_len_past_maxb", "blocks"), ("treeless_", "literals"), ("huf", "literals"),
               ("lits_used", "literals"), ("off_", "offsets"), ("rep0_", "offsets"), ("repeat_", "sequences"),
               ("rle_", "sequences"), ("seq_", "sequences"), ("ll_", "sequences"), ("of_", "sequences"),
               ("nseq_", "sequences"), ("", "frames")]


def bad_family(name):
    return next(f for p, f in _BAD_FAMILY if name.startswith(p))


def window_lenient(seed=602):
    """A compressed block of 3 KiB in a frame whose window descriptor says
    1 KiB: above that frame's Block_Maximum_Size (the smaller of the window
    and 128 KiB), so libzstd refuses it; the decoders here do not look at
    the window.  (Bad, output)"""
    rng = np.random.default_rng(seed)
    blks = [("comp", ("raw", _rnd(rng, 3000)), [(2999, 7, 2000)], None)]
    return Bad("window_1k_block_3k", frame_bytes(blks, single=False, window=0, strict=False), 5000), \
        decode_frame(blks)
