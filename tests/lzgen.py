"""Sequence-level LZ4 / snappy stream builders, a plain reference decoder and
the hand-built corpora of the decoder edge tests (test_lzstreams_cpu.py,
test_gpu_lzstreams.py).  No project imports: the streams are written from
the formats' own rules, so they hold what no encoder in the suite emits
(4-byte snappy offsets, padded length bytes, block checksums) and put every
construct where the decoders' own constants say an edge is.

A stream is described twice, by the same list: the builder turns the list
into compressed bytes, ``decode`` turns it into the bytes it must decode to.

LZ4 block:  [(literal_bytes, offset, match_len), ..., (literal_bytes, None, 0)]
snappy:     [("L", bytes, n_len_bytes | None), ("C", offset, length, kind | None), ...]
"""
import struct

import numpy as np

try:
    import xxhash

    def _xxh32(b):
        return xxhash.xxh32_intdigest(bytes(b), 0)
    HAVE_XXH = True
except Exception:  # the decoders skip checksum bytes; only pyarrow reads them
    def _xxh32(b):
        return 0x5A5A5A5A
    HAVE_XXH = False


# ---------------------------------------------------------------- geometry
# The lane decoder's geometries, (STROM_DECOMP_G value, W, kRing, kInW), from
# csrc/kernels/decompress.hip:812-824 (the `using S16 = Stream<GL, RING, INW>`
# lines; W = 4 GL) and the G -> geometry table of strom_decompress_lanes.
LANE_GEOMS = [
    (16, 16, 2048, 448),
    (32, 16, 1024, 256),
    (8, 32, 2048, 512),
    (4, 64, 2048, 512),
    (1, 256, 2048, 1024),
    (2, 128, 16384, 512),
    (6, 64, 8192, 512),
    (3, 256, 16384, 1024),
]
# The block-parallel builds, STROM_DECOMP_PAR value -> PW, SL, PAD, OB, from
# csrc/kernels/lz4par.hip:64-95 (SL = PW / NT) and the defines of
# lz4par_nt512.hip (NT 512) and lz4par_nt512_ob8k.hip (NT 512, OB 8192).
PAR_BUILDS = {
    256: dict(PW=16384, SL=64, PAD=64, OB=4096),
    512: dict(PW=16384, SL=32, PAD=64, OB=4096),
    8192: dict(PW=16384, SL=32, PAD=64, OB=8192),
}
WS = sorted({g[1] for g in LANE_GEOMS})
RINGS = sorted({g[2] for g in LANE_GEOMS})
INWS = sorted({g[3] for g in LANE_GEOMS})
RING_W = sorted({(g[2], g[1]) for g in LANE_GEOMS})
OBS = sorted({b["OB"] for b in PAR_BUILDS.values()})
PW = 16384
PAD = 64


def kslide(inw):
    return inw - 64


def _rnd(rng, n):
    return rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()


# ------------------------------------------------------------- LZ4 builder
def lz4_len_ext(n, n_ext=None):
    """The extension bytes of a length field whose nibble is 15 (n = the
    length minus 15).  LZ4 admits exactly one spelling, n // 255 bytes of 255
    and one of n % 255; ``n_ext`` asks for a count and raises when the
    format does not allow it."""
    out = b"\xff" * (n // 255) + bytes([n % 255])
    if n_ext is not None and n_ext != len(out):
        raise ValueError("LZ4 length %d takes %d extension bytes, not %d" % (n + 15, len(out), n_ext))
    return out


def lz4_seq_bytes(lit, off, mlen, lit_ext=None, ml_ext=None):
    """One sequence, unchecked (the malformed corpus uses it directly)."""
    ll = len(lit)
    if off is None:
        tok = min(ll, 15) << 4
        return bytes([tok]) + (lz4_len_ext(ll - 15, lit_ext) if ll >= 15 else b"") + lit
    m = mlen - 4
    tok = (min(ll, 15) << 4) | min(m, 15)
    return (bytes([tok]) + (lz4_len_ext(ll - 15, lit_ext) if ll >= 15 else b"") + lit +
            struct.pack("<H", off) + (lz4_len_ext(m - 15, ml_ext) if m >= 15 else b""))


def lz4_block(seqs, ext=None, history=0):
    """A valid raw LZ4 block.  ``ext``: {sequence index: (lit_ext, ml_ext)}
    extension byte counts to insist on; ``history``: output bytes before the
    block that its matches may reach (linked frames).  Raises on anything
    the format forbids, the end-of-block rules included."""
    ext = ext or {}
    if not seqs or seqs[-1][1] is not None:
        raise ValueError("the last sequence is literals only")
    if len(seqs) > 1 and len(seqs[-1][0]) < 5:
        raise ValueError("final literals: at least 5 bytes")
    out, produced, last_match_start = [], 0, None
    for i, (lit, off, mlen) in enumerate(seqs):
        le, me = ext.get(i, (None, None))
        if off is None:
            if i != len(seqs) - 1:
                raise ValueError("literal-only sequence before the end")
        else:
            if not 1 <= off <= 65535 or off > history + produced + len(lit):
                raise ValueError("offset %d with %d bytes produced" % (off, produced + len(lit)))
            if mlen < 4:
                raise ValueError("match length < 4")
        out.append(lz4_seq_bytes(lit, off, mlen, le, me))
        produced += len(lit) + (mlen if off is not None else 0)
        if off is not None:
            last_match_start = produced - mlen
    if last_match_start is not None and produced - last_match_start < 12:
        raise ValueError("last match begins less than 12 bytes before the end")
    return b"".join(out)


def lz4_frame(blocks, linked=True, block_checksum=False, content_size=None, block_max=7):
    """An LZ4 frame over raw blocks: ("lz4", seqs) | ("stored", bytes), with
    the end mark.  ``content_size``: the value of the header field, or None."""
    flg = 0x40 | (0 if linked else 0x20) | (0x10 if block_checksum else 0) | \
        (0x08 if content_size is not None else 0)
    desc = bytes([flg, block_max << 4])
    if content_size is not None:
        desc += struct.pack("<Q", content_size)
    out = [struct.pack("<I", 0x184D2204), desc, bytes([(_xxh32(desc) >> 8) & 0xFF])]
    produced = 0
    for kind, body in blocks:
        if kind == "lz4":
            data = lz4_block(body, history=produced if linked else 0)
            out.append(struct.pack("<I", len(data)))
            produced += sum(len(s[0]) + s[2] for s in body)
        elif kind == "stored":
            data = bytes(body)
            out.append(struct.pack("<I", len(data) | 0x80000000))
            produced += len(data)
        else:
            raise ValueError(kind)
        if not data:
            raise ValueError("an empty block is the end mark")
        out.append(data)
        if block_checksum:
            out.append(struct.pack("<I", _xxh32(data)))
    out.append(b"\0\0\0\0")
    return b"".join(out)


def frame_body(frame):
    """(bytes from the first block header on, block-checksum flag): what the
    LZ4_FRAME / LZ4_FRAME_BCS codecs take."""
    assert frame[:4] == struct.pack("<I", 0x184D2204)
    flg = frame[4]
    p = 6 + (8 if flg & 0x08 else 0) + (4 if flg & 0x01 else 0) + 1
    return frame[p:], bool(flg & 0x10)


def arrow_lz4(buffer_len, frame):
    """An Arrow IPC compressed buffer: int64 length prefix + LZ4 frame;
    buffer_len -1 = the stored form (``frame`` is then the raw bytes)."""
    return struct.pack("<q", buffer_len) + frame


# ---------------------------------------------------------- snappy builder
def varint(n, nbytes=None):
    out = []
    while True:
        b = n & 0x7F
        n >>= 7
        if n:
            out.append(b | 0x80)
        else:
            out.append(b)
            break
    if nbytes is not None:
        if nbytes < len(out):
            raise ValueError("varint does not fit %d bytes" % nbytes)
        while len(out) < nbytes:
            out[-1] |= 0x80
            out.append(0)
    return bytes(out)


def snappy_elem_bytes(e):
    if e[0] == "L":
        _, lit, nlb = e
        n = len(lit)
        if n < 1 or n > 1 << 32:
            raise ValueError("literal length")
        if nlb is None:
            nlb = 0 if n <= 60 else (n - 1).bit_length() + 7 >> 3
        if nlb == 0:
            if n > 60:
                raise ValueError("literal > 60 needs length bytes")
            return bytes([(n - 1) << 2]) + lit
        if not 1 <= nlb <= 4 or (n - 1) >> (8 * nlb):
            raise ValueError("literal %d in %d length bytes" % (n, nlb))
        return bytes([(59 + nlb) << 2]) + (n - 1).to_bytes(nlb, "little") + lit
    _, off, length, kind = e
    if kind is None:
        kind = 1 if 4 <= length <= 11 and off < 2048 else 2 if off < 65536 else 3
    if off < 1:
        raise ValueError("offset 0")
    if kind == 1:
        if not 4 <= length <= 11 or off >= 2048:
            raise ValueError("kind 1: length 4..11, offset < 2048")
        return bytes([1 | ((length - 4) << 2) | ((off >> 8) << 5), off & 0xFF])
    if not 1 <= length <= 64:
        raise ValueError("copy length 1..64")
    if kind == 2:
        if off >= 65536:
            raise ValueError("kind 2: offset < 65536")
        return bytes([2 | ((length - 1) << 2)]) + struct.pack("<H", off)
    if kind == 3:
        if off >= 1 << 32:
            raise ValueError("kind 3: offset < 2^32")
        return bytes([3 | ((length - 1) << 2)]) + struct.pack("<I", off)
    raise ValueError("kind")


def snappy_stream(elems, declared_len, preamble_bytes=None):
    produced, out = 0, [varint(declared_len, preamble_bytes)]
    for e in elems:
        if e[0] == "C" and e[1] > produced:
            raise ValueError("offset %d with %d bytes produced" % (e[1], produced))
        out.append(snappy_elem_bytes(e))
        produced += len(e[1]) if e[0] == "L" else e[2]
    return b"".join(out)


# --------------------------------------------------------------- reference
def decode(items, out=None):
    """The plain reference: what a list of LZ4 sequences or snappy elements
    decodes to, a byte at a time; ``out`` = the output so far (linked frame
    blocks share one)."""
    o = bytearray() if out is None else out
    for it in items:
        if it[0] == "L":
            o += it[1]
            continue
        if it[0] == "C":
            off, n = it[1], it[2]
        else:
            o += it[0]
            off, n = it[1], it[2]
            if off is None:
                continue
        assert 1 <= off <= len(o)
        for _ in range(n):
            o.append(o[-off])
    return o


def decode_frame(blocks, linked=True):
    o = bytearray()
    for kind, body in blocks:
        if kind == "stored":
            o += body
        elif linked:
            decode(body, o)
        else:
            o += decode(body)
    return bytes(o)


def _lz4(name, seqs, ext=None):
    return (name, lz4_block(seqs, ext), bytes(decode(seqs)))


def _snap(name, elems, preamble_bytes=None):
    exp = bytes(decode(elems))
    return (name, snappy_stream(elems, len(exp), preamble_bytes), exp)


# ------------------------------------------------------------ LZ4 corpora
LIT_LENS = [0, 1, 14, 15, 16, 269, 270, 271, 524, 525]
MATCH_LENS = sorted({4, 5, 18, 19, 20, 273, 274, 275, 528, 529} |
                    {x for w in WS for x in (w - 1, w, w + 1, 2 * w - 1, 2 * w, 2 * w + 1)})
OFFSETS = sorted({1, 2, 3, 4, 5, 7, 8} | {x for w in WS for x in (w - 1, w, w + 1)})
TAIL = 12     # final literals of every valid block: covers both end-of-block rules


def lz4_lengths(seed=101):
    """Every literal length x match length x offset of the edge sets, each
    behind a 300-byte random prefix; 70000-byte literal and matches."""
    rng = np.random.default_rng(seed)
    out = []
    # literal and match lengths against one another at a few offsets, and
    # every offset against every match length: the full triple product
    # (10 x 31 x 22) would only repeat these pairs
    for ll in LIT_LENS:
        for ml in MATCH_LENS:
            off = OFFSETS[(ll + ml) % len(OFFSETS)]
            out.append(_lz4("len_l%d_m%d_o%d" % (ll, ml, off),
                            [(_rnd(rng, 300), 300, 4), (_rnd(rng, ll), off, ml),
                             (_rnd(rng, TAIL), None, 0)]))
    for off in OFFSETS:
        for ml in MATCH_LENS:
            ll = LIT_LENS[(off + ml) % len(LIT_LENS)]
            out.append(_lz4("off_o%d_m%d_l%d" % (off, ml, ll),
                            [(_rnd(rng, 300), 300, 4), (_rnd(rng, ll), off, ml),
                             (_rnd(rng, TAIL), None, 0)]))
    for off in OFFSETS:
        for ll in LIT_LENS:
            out.append(_lz4("off_o%d_l%d" % (off, ll),
                            [(_rnd(rng, 300), 300, 4), (_rnd(rng, ll), off, 4 + (off + ll) % 15),
                             (_rnd(rng, TAIL), None, 0)]))
    out.append(_lz4("lit70000", [(_rnd(rng, 70000), None, 0)]))
    for off in (1, 3, 65535):
        out.append(_lz4("match70000_o%d" % off,
                        [(_rnd(rng, max(off, 300)), off, 70000), (_rnd(rng, TAIL), None, 0)]))
    return out


def lz4_far(seed=102):
    """Offsets around kRing - W, kRing and 65535, match lengths that overlap
    their own source, at the very start of the output and 3 kRing later;
    each far match is followed at once by a second one of length 4."""
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    for ring, w in RING_W:
        for off in (ring - w - 1, ring - w, ring - w + 1, ring - 1, ring, ring + 1, 65535):
            for ml in (4, w, 2 * w, 2 * w + 1, off - 1, off, off + 1, 2 * off + 3):
                for extra in (0, 3 * ring):
                    if (off, ml, extra) in seen:
                        continue
                    seen.add((off, ml, extra))
                    out.append(_lz4("far_o%d_m%d_at%d" % (off, ml, off + extra),
                                    [(_rnd(rng, off + extra), off, ml), (b"", off, 4),
                                     (_rnd(rng, TAIL), None, 0)]))
    return out


def _token_positions(inw):
    s = kslide(inw)
    base = list(range(s - 8, s + 9)) + list(range(inw - 72, inw + 9))
    return sorted(set(base + [p + s for p in base]))


def _lit_for_token_at(p):
    """(L, match length) so that a first sequence of L literals and that
    match ends at input position p (a match of 19 spends one more byte where
    the literal length field's own size skips a position)."""
    for ml, mb in ((4, 0), (19, 1)):
        for ll in range(p, max(p - 20, 0), -1):
            if 1 + (0 if ll < 15 else len(lz4_len_ext(ll - 15))) + ll + 2 + mb == p:
                return ll, ml
    raise ValueError(p)


def lz4_window(seed=103):
    """A token on every input position around the slide point and the end
    of each geometry's input window (and one window later), once a short
    sequence and once one with literal and match length extensions; literal
    runs of kInW, kInW + 1 and 2 kInW + 3."""
    rng = np.random.default_rng(seed)
    out = []
    short = [(_rnd(rng, 3), 7, 6), (_rnd(rng, 2), 5, 9), (_rnd(rng, 1), 11, 4)]
    for inw in INWS:
        for p in _token_positions(inw):
            ll, ml0 = _lit_for_token_at(p)
            for kind in ("short", "ext"):
                first = (_rnd(rng, 3), 7, 6) if kind == "short" else (_rnd(rng, 15 + p % 3), 9, 19 + p % 5)
                seqs = [(_rnd(rng, ll), 1 + p % 8, ml0), first] + short + \
                       [(_rnd(rng, inw + 40), None, 0)]    # input for the windows after
                out.append(_lz4("win%d_tok%d_%s" % (inw, p, kind), seqs))
        # the same positions reached through the fast step: 5-byte sequences
        # up to the token at p, so the window runs short in front of it
        # (a long literal run slides the window by itself, ahead of its end)
        for p in _token_positions(inw):
            lead = (p - 3) % 5 or 5
            seqs = [(_rnd(rng, lead), 1, 4)] + [(_rnd(rng, 2), 1 + i % 3, 5) for i in range((p - 3 - lead) // 5)]
            seqs += [(_rnd(rng, 15 + p % 3), 9, 19 + p % 5)] + short + [(_rnd(rng, inw + 40), None, 0)]
            assert len(lz4_block(seqs[:-5] + [(b"x" * 12, None, 0)])) - 13 == p
            out.append(_lz4("win%d_creep%d" % (inw, p), seqs))
        for ll in (inw, inw + 1, 2 * inw + 3):
            out.append(_lz4("win%d_lit%d" % (inw, ll),
                            [(_rnd(rng, ll), 3, 5)] + short + [(_rnd(rng, TAIL), None, 0)]))
    return out


def _lz4_of_comp_len(rng, n):
    """A block of exactly n compressed bytes: 8-byte sequences (5 literals,
    match of 7), the final literals sized to fit."""
    for first in range(5, 12):
        seqs = [(_rnd(rng, first), 3, 7)]
        used = 3 + first
        while n - used > 300:
            seqs.append((_rnd(rng, 5), 1 + len(seqs) % 9, 7))
            used += 8
        rest = n - used                      # token + extension + literals
        for ll in range(max(rest - 4, TAIL), rest):
            if 1 + (0 if ll < 15 else len(lz4_len_ext(ll - 15))) + ll == rest:
                return seqs + [(_rnd(rng, ll), None, 0)]
    raise ValueError(n)


def lz4_par_edges(seed=104):
    """The block-parallel decoder's own edges: compressed lengths around the
    parse window (PW, PAD), output lengths around the resolve batch (OB), an
    offset-1 run across a batch boundary, a match longer than a batch, three
    windows of 3-byte sequences and a literal run on the serial walk."""
    rng = np.random.default_rng(seed)
    out = []
    for k in (1, 2):
        for d in (-PAD - 1, -PAD, -PAD + 1, -33, -32, -31, -1, 0, 1, 31, 32, 33,
                  PAD - 1, PAD, PAD + 1):
            n = k * PW + d
            seqs = _lz4_of_comp_len(rng, n)
            out.append(_lz4("clen%d" % n, seqs))
            assert len(out[-1][1]) == n
    for ob in OBS:
        for k in (1, 2):
            for d in (-1, 0, 1):
                n = k * ob + d
                seqs = [(_rnd(rng, 40), 7, 60)]
                while sum(len(s[0]) + s[2] for s in seqs) < n - 600:
                    seqs.append((_rnd(rng, 9), 1 + len(seqs) % 30, 40))
                seqs.append((_rnd(rng, n - sum(len(s[0]) + s[2] for s in seqs)), None, 0))
                name, c, e = _lz4("olen%d_ob%d" % (n, ob), seqs)
                assert len(e) == n
                out.append((name, c, e))
    out.append(_lz4("run1_across_ob", [(_rnd(rng, 4000), 1, 200), (_rnd(rng, 3900), 1, 200),
                                       (_rnd(rng, TAIL), None, 0)]))
    out.append(_lz4("match_gt_ob_o5", [(_rnd(rng, 100), 5, 9000), (_rnd(rng, TAIL), None, 0)]))
    out.append(_lz4("match_gt_ob_o1000", [(_rnd(rng, 1000), 1000, 10000), (_rnd(rng, TAIL), None, 0)]))
    dense = [(_rnd(rng, 8), 8, 4)] + [(b"", 1 + i % 8, 4) for i in range(3 * PW // 3)]
    out.append(_lz4("dense_3byte_seqs", dense + [(_rnd(rng, TAIL), None, 0)]))
    out.append(_lz4("lit40000", [(_rnd(rng, 40000), 9, 4), (_rnd(rng, TAIL), None, 0)]))
    return out


def lz4_random(seed=105):
    """300 streams of 1-400 sequences (log-uniform), every field drawn from
    the edge sets of the families above."""
    rng = np.random.default_rng(seed)
    offs = sorted(set(OFFSETS) | {x for r, w in RING_W for x in (r - w - 1, r - w, r - w + 1, r - 1, r, r + 1)} |
                  {65535})
    out = []
    for i in range(300):
        nseq = int(np.exp(rng.uniform(0, np.log(400.999))))
        seqs, produced = [], 0
        for _ in range(nseq):
            ll = LIT_LENS[int(rng.integers(0, len(LIT_LENS)))]
            if produced + ll == 0:
                ll = 1
            off = min(offs[int(rng.integers(0, len(offs)))], produced + ll, 65535)
            ml = MATCH_LENS[int(rng.integers(0, len(MATCH_LENS)))]
            seqs.append((_rnd(rng, ll), off, ml))
            produced += ll + ml
        seqs.append((_rnd(rng, TAIL + int(rng.integers(0, 20))), None, 0))
        out.append(_lz4("rand%d_n%d" % (i, nseq), seqs))
    return out


def lz4_frames(seed=106):
    """Frames of 0, 1 and 3-5 blocks under every flag combination, stored
    blocks between compressed ones, and in linked frames matches whose
    source starts 1 and 65535 bytes before the block: (name, frame, expected)."""
    rng = np.random.default_rng(seed)

    def blk(prev, first_off=None):
        seqs = []
        if first_off is not None:
            seqs.append((b"", first_off, 8))      # begins before the block
        seqs += [(_rnd(rng, 40), 7, 20), (_rnd(rng, 3), 17, 300), (_rnd(rng, 200), 64, 33)]
        return ("lz4", seqs + [(_rnd(rng, TAIL), None, 0)])

    out = []
    for linked in (True, False):
        for bc in (False, True):
            for cs in (False, True):
                tag = "%s_%s_%s" % ("linked" if linked else "indep", "bcs" if bc else "nobcs",
                                    "csize" if cs else "nocsize")
                shapes = {
                    "0blk": [],
                    "1blk": [blk(0)],
                    "1stored": [("stored", _rnd(rng, 777))],
                    "3blk": [blk(0), ("stored", _rnd(rng, 1001)), blk(1, 1 if linked else None)],
                    "5blk": [("stored", _rnd(rng, 65536)), blk(1, 65535 if linked else None),
                             ("stored", _rnd(rng, 17)), blk(1, 1 if linked else None),
                             blk(1, 65535 if linked else None)],
                    "4blk": [blk(0), blk(1, 1 if linked else None), blk(1, 300 if linked else None),
                             ("stored", _rnd(rng, 5))],
                }
                for sname, blocks in shapes.items():
                    exp = decode_frame(blocks, linked)
                    f = lz4_frame(blocks, linked=linked, block_checksum=bc,
                                  content_size=len(exp) if cs else None)
                    out.append(("frame_%s_%s" % (tag, sname), f, exp))
    return out


def arrow_buffers(seed=107):
    """Arrow IPC buffers: every frame of lz4_frames behind its length prefix
    and the stored (-1) form at the sizes around a 16-byte chunk and a page."""
    rng = np.random.default_rng(seed)
    out = [("arrow_" + n, arrow_lz4(len(e), f), e) for n, f, e in lz4_frames()]
    for n in (0, 1, 15, 16, 17, 4097):
        raw = _rnd(rng, n)
        out.append(("arrow_stored%d" % n, arrow_lz4(-1, raw), raw))
    return out


# --------------------------------------------------------- snappy corpora
SN_LIT_LENS = sorted({1, 59, 60, 61, 62, 255, 256, 257, 65535, 65536, 65537} |
                     {x for w in WS for x in (w - 1, w, w + 1)})
SN_OFFSETS = sorted({1, 2, 3, 4, 7, 8, 2047, 2048, 65535, 65536, 70000} |
                    {x for r, w in RING_W for x in (w - 1, w + 1, r - w - 1, r - w + 1, r - 1, r + 1)})
SN_COPY_LENS = [1, 2, 3, 4, 11, 12, 63, 64]


def snappy_literals(seed=201):
    """Every literal length with every legal count of length bytes."""
    rng = np.random.default_rng(seed)
    out = []
    for n in SN_LIT_LENS:
        for nlb in range(0, 5):
            if (nlb == 0 and n > 60) or (nlb and (n - 1) >> (8 * nlb)):
                continue
            out.append(_snap("lit%d_lb%d" % (n, nlb),
                             [("L", _rnd(rng, 5), None), ("L", _rnd(rng, n), nlb),
                              ("C", 3, 5, None), ("L", _rnd(rng, 7), None)]))
    return out


def snappy_copies(seed=202):
    """Every offset with every copy kind that can carry it (kind 3 with the
    small offsets too), all copy lengths after one another."""
    rng = np.random.default_rng(seed)
    out = []
    for off in SN_OFFSETS:
        for kind in (1, 2, 3):
            if (kind == 1 and off >= 2048) or (kind == 2 and off >= 65536):
                continue
            elems = [("L", _rnd(rng, off), None)]
            for n in SN_COPY_LENS:
                if kind == 1 and not 4 <= n <= 11:
                    continue
                elems += [("C", off, n, kind), ("L", _rnd(rng, 1 + n % 3), None)]
            out.append(_snap("copy_o%d_k%d" % (off, kind), elems))
            # each length on its own, straight after the prefix
            for n in SN_COPY_LENS:
                if (kind == 1 and not 4 <= n <= 11) or off > 2100:
                    continue
                out.append(_snap("copy_o%d_k%d_n%d" % (off, kind, n),
                                 [("L", _rnd(rng, off), None), ("C", off, n, kind)]))
    return out


def snappy_preambles(seed=203):
    """Preambles of 1-5 bytes, minimal and padded.  (name, stream, expected,
    capacity): capacity equal to, or above, the declared length."""
    rng = np.random.default_rng(seed)
    out = []
    for n in (0, 1, 100, 127, 128, 16383, 16384, 70000):
        elems = [("L", _rnd(rng, n), None)] if n else []
        for nb in range(1, 6):
            if nb < len(varint(n)):
                continue
            name, c, e = _snap("pre%d_b%d" % (n, nb), elems, nb)
            out.append((name, c, e, n))
            out.append((name + "_roomy", c, e, n + 1 + (n + nb) % 17))
    return out


def snappy_window(seed=204):
    """The LZ4 window-edge sweep for snappy: a tag on every input position
    around each geometry's slide point and window end."""
    rng = np.random.default_rng(seed)
    out = []
    short = [("C", 7, 6, 1), ("L", _rnd(rng, 3), None), ("C", 5, 9, 2), ("L", _rnd(rng, 2), None)]
    for inw in INWS:
        for p in _token_positions(inw):
            for kind in ("short", "long"):
                # the preamble's size depends on the total, the total on the
                # leading literal: settle by trying the candidates (the last
                # one pads the length bytes, for the positions that the
                # minimal forms skip)
                for ll, nlb in ((p - 3, None), (p - 4, None), (p - 5, None), (p - 6, None), (p - 5, 2)):
                    lead = ("L", _rnd(rng, ll), nlb)
                    nxt = [("C", 9, 4, 1)] if kind == "short" else \
                          [("L", _rnd(rng, 61 + p % 5), 1 + p % 4), ("C", 1 + p % 64, 64, 3)]
                    elems = [lead] + nxt + short + [("L", _rnd(rng, inw + 40), 2)]
                    total = len(decode(elems))
                    if len(varint(total)) + len(snappy_elem_bytes(lead)) == p:
                        out.append(_snap("win%d_tag%d_%s" % (inw, p, kind), elems))
                        break
                else:
                    raise ValueError(p)
        # the same positions reached through the fast step (5 bytes per
        # copy + literal pair behind a 2-byte preamble)
        for p in _token_positions(inw):
            lead = (p - 3) % 5 or 5
            elems = [("L", _rnd(rng, lead), None)]
            for i in range((p - 3 - lead) // 5):
                elems += [("C", 1 + i % 3, 4 + i % 8, 1), ("L", _rnd(rng, 2), None)]
            assert 2 + sum(len(snappy_elem_bytes(e)) for e in elems) == p
            elems += [("L", _rnd(rng, 61 + p % 5), 1 + p % 4), ("C", 1 + p % 64, 64, 3)] + short + \
                     [("L", _rnd(rng, inw + 40), 2)]
            name, c, e = _snap("win%d_creep%d" % (inw, p), elems)
            assert len(varint(len(e))) == 2
            out.append((name, c, e))
        for ll in (inw, inw + 1, 2 * inw + 3):
            out.append(_snap("win%d_lit%d" % (inw, ll), [("L", _rnd(rng, ll), None)] + short))
    return out


def snappy_random(seed=205):
    rng = np.random.default_rng(seed)
    out = []
    lits = [n for n in SN_LIT_LENS if n < 60000]
    for i in range(300):
        nel = int(np.exp(rng.uniform(0, np.log(400.999))))
        elems, produced = [], 0
        for _ in range(nel):
            if produced == 0 or rng.random() < 0.4:
                n = lits[int(rng.integers(0, len(lits)))]
                legal = [b for b in range(5) if not ((b == 0 and n > 60) or (b and (n - 1) >> (8 * b)))]
                elems.append(("L", _rnd(rng, n), legal[int(rng.integers(0, len(legal)))]))
                produced += n
            else:
                off = min(SN_OFFSETS[int(rng.integers(0, len(SN_OFFSETS)))], produced)
                n = SN_COPY_LENS[int(rng.integers(0, len(SN_COPY_LENS)))]
                kinds = [k for k in (1, 2, 3) if not ((k == 1 and (off >= 2048 or not 4 <= n <= 11)) or
                                                     (k == 2 and off >= 65536))]
                elems.append(("C", off, n, kinds[int(rng.integers(0, len(kinds)))]))
                produced += n
        out.append(_snap("rand%d_n%d" % (i, nel), elems, int(rng.integers(len(varint(produced)), 6))))
    return out


# ------------------------------------------------------ COPY and alignment
def copy_streams(seed=301):
    rng = np.random.default_rng(seed)
    return [("copy%d" % n, b, b) for n in (0, 1, 15, 16, 17, 4095, 4096, 4097)
            for b in [_rnd(rng, n)]]


def align_streams(seed=302):
    """One stream of ~600 output bytes per codec (a short match, a match
    with a length extension, an offset-1 run): {codec name: (stream, expected)},
    to be placed at every source x destination misalignment."""
    rng = np.random.default_rng(seed)
    seqs = [(_rnd(rng, 37), 5, 6), (_rnd(rng, 120), 90, 300), (_rnd(rng, 9), 1, 70),
            (_rnd(rng, 30), 13, 4), (_rnd(rng, 24), None, 0)]
    elems = [("L", _rnd(rng, 37), None), ("C", 5, 6, 1), ("L", _rnd(rng, 120), 2),
             ("C", 90, 64, 2), ("C", 90, 64, 3), ("C", 64, 61, 2), ("L", _rnd(rng, 9), None),
             ("C", 1, 64, 2), ("C", 1, 6, 1), ("L", _rnd(rng, 170), 1), ("C", 13, 4, 1)]
    raw = _rnd(rng, 603)
    return {"lz4": _lz4("align", seqs)[1:], "snappy": _snap("align", elems)[1:], "copy": (raw, raw)}


# --------------------------------------------------------------- malformed
def lz4_malformed(seed=401):
    """Raw LZ4 blocks wrong in exactly one place: (name, stream, capacity,
    status) with status -2 where the contract fixes it, else None (< 0)."""
    rng = np.random.default_rng(seed)
    tail = lz4_seq_bytes(_rnd(rng, TAIL), None, 0)
    pre = lz4_seq_bytes(_rnd(rng, 300), 300, 4)
    out = [("off0", pre + lz4_seq_bytes(_rnd(rng, 5), 0, 8) + tail, 304 + 13 + TAIL, None),
           ("off_past_start_first", lz4_seq_bytes(_rnd(rng, 20), 21, 8) + tail, 28 + TAIL, None)]
    for ring in RINGS:
        n = 3 * ring
        out.append(("off_past_start_at%d" % n, lz4_seq_bytes(_rnd(rng, n), n + 1, 8) + tail,
                    n + 8 + TAIL, None))
    out.append(("lit_past_end", pre + bytes([0xE0]) + _rnd(rng, 5), 304 + 14, None))
    out.append(("lit_ext_past_end", pre + bytes([0xF0, 200]) + _rnd(rng, 100), 304 + 215, None))
    out.append(("one_offset_byte", pre + bytes([0x30]) + _rnd(rng, 3) + b"\x02", 304 + 3 + 4, None))
    out.append(("ends_on_255_lit", pre + bytes([0xF0, 255]), 304 + 600, None))
    out.append(("ends_on_255_match", pre + bytes([0x3F]) + _rnd(rng, 3) + b"\x02\x00\xff", 304 + 600, None))
    good = [(_rnd(rng, 300), 300, 4), (_rnd(rng, 9), 40, 100), (_rnd(rng, 30), None, 0)]
    n = len(decode(good))
    out.append(("short_cap_in_literal", lz4_block(good), n - 1, -2))
    # a well-formed block ends in literals, so the capacity ends one byte
    # short of the match's end: the first byte that does not fit is a match byte
    out.append(("short_cap_in_match", lz4_block(good), 304 + 9 + 100 - 1, -2))
    # and a block that ends with its match (an empty last sequence), one short
    ends_in_match = pre + lz4_seq_bytes(_rnd(rng, 9), 40, 100) + b"\x00"
    out.append(("short_cap_block_ends_in_match", ends_in_match, 304 + 109 - 1, None))
    return out


def snappy_malformed(seed=402):
    rng = np.random.default_rng(seed)
    lit = lambda n: snappy_elem_bytes(("L", _rnd(rng, n), None))
    out = []

    def add(name, body, declared, cap=None, status=None, pre=None):
        out.append((name, varint(declared, pre) + body, declared if cap is None else cap, status))

    add("off0", lit(50) + bytes([2 | (9 << 2), 0, 0]) + lit(7), 67)
    add("off0_kind1", lit(50) + bytes([1 | (2 << 2), 0]) + lit(7), 63)
    add("off_gt_produced", lit(50) + snappy_elem_bytes(("C", 51, 10, 2)) + lit(7), 67)
    add("off_gt_produced_kind3", lit(50) + snappy_elem_bytes(("C", 70000, 10, 3)) + lit(7), 67)
    add("lit_past_end", lit(50) + bytes([(40 - 1) << 2]) + _rnd(rng, 39), 90)
    add("lit_lenbytes_past_end", lit(50) + bytes([62 << 2, 0x10]), 50 + 0x2011)
    for kind in (1, 2, 3):
        full = snappy_elem_bytes(("C", 20, 8, kind))
        for cut in range(1, len(full)):
            add("copy_k%d_cut%d" % (kind, cut), lit(50) + full[:cut], 58)
    add("preamble_gt_cap", lit(50), 50, cap=49, status=-2)
    add("preamble_gt_cap_padded", lit(50), 50, cap=49, status=-2, pre=5)
    add("body_one_short", lit(50) + snappy_elem_bytes(("C", 5, 9, 1)), 60)
    add("body_one_long", lit(50) + snappy_elem_bytes(("C", 5, 9, 1)), 58)
    add("body_one_long_literal", lit(50) + lit(9), 58)
    out.append(("varint6", b"\x80\x80\x80\x80\x80\x00" + lit(50), 50, None))
    # a 5-byte preamble of 2^32 (and 2^32 + 50): above any capacity, not 0 (or 50)
    out.append(("preamble_2p32_empty", b"\x80\x80\x80\x80\x10", 0, -2))
    out.append(("preamble_2p32_plus50", b"\xb2\x80\x80\x80\x10" + lit(50), 50, -2))
    add("lit_ffffffff", lit(50) + bytes([63 << 2]) + b"\xff\xff\xff\xff" + _rnd(rng, 64), 114)
    return out


def arrow_malformed(seed=403):
    rng = np.random.default_rng(seed)
    blocks = [("lz4", [(_rnd(rng, 40), 7, 60), (_rnd(rng, TAIL), None, 0)])]
    f = lz4_frame(blocks)
    n = len(decode_frame(blocks))
    return [("arrow_prefix_gt_cap", arrow_lz4(n, f), n - 1, -2),
            ("arrow_prefix_gt_cap_frame_fits", arrow_lz4(n + 5, f), n, -2),
            ("arrow_prefix_huge", arrow_lz4(1 << 40, f), n, -2),
            ("arrow_stored_gt_cap", arrow_lz4(-1, _rnd(rng, 100)), 99, -2)]


LZ4_FAMILIES = {"lengths": lz4_lengths, "far": lz4_far, "window": lz4_window,
                "par_edges": lz4_par_edges, "random": lz4_random}
SNAPPY_FAMILIES = {"literals": snappy_literals, "copies": snappy_copies, "window": snappy_window,
                   "random": snappy_random}
