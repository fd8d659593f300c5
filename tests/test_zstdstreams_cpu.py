"""The hand-built Zstandard corpora of tests/zstdgen.py against every zstd
decoder that runs without a GPU: the plain reference (zstdgen.decode, which
produced the expected bytes from the same descriptions), libzstd (pyarrow's
codec) and the host twins of the three GPU decoders in csrc/kernels/zstd.hip:
one wave per stream, frame-parallel (4 blocks in flight) and lane-parallel,
alone and over a family at a time.  No stream is skipped or filtered: a
corpus function may only produce streams that all of them accept.
test_gpu_zstdstreams.py feeds the same corpora to the kernels."""
import numpy as np
import pytest

import zstdgen as G
from nvme_strom_amd import _native as N
from nvme_strom_amd.ops import decompress as D

pa = pytest.importorskip("pyarrow")

GUARD = 64
FILL = 0xA5
TWINS = ["wave", "fp4", "lp"]


@pytest.fixture(scope="module")
def corpora():
    return {k: f() for k, f in G.FAMILIES.items()}


def libzstd(comp, n):
    """libzstd's decoder; an empty output through its streaming reader (the
    one-shot call wants a size)."""
    if n == 0:
        return pa.CompressedInputStream(pa.BufferReader(comp), "zstd").read()
    return pa.Codec("zstd").decompress(comp, decompressed_size=n, asbytes=True)


def _codec(c):
    return D.ARROW_ZSTD if c.arrow else D.ZSTD


def twin(which, codec, comp, cap):
    """One host twin on a destination of cap + GUARD bytes pre-filled with
    FILL: (status, the cap bytes, guard untouched)."""
    src = np.frombuffer(comp + b"\0", dtype=np.uint8)
    out = np.full(cap + GUARD, FILL, dtype=np.uint8)
    if which == "wave":
        st = N.lib().strom_zstd_host(codec, src.ctypes.data, len(comp), out.ctypes.data, cap)
    elif which == "fp4":
        st = N.lib().strom_zstd_host_fp(codec, src.ctypes.data, len(comp), out.ctypes.data, cap, G.FPW)
    else:
        st, _, _ = lp_batch(codec, [comp], [cap], out)
        st = st[0]
    return st, out[:cap].tobytes(), bool((out[cap:] == FILL).all())


def lp_batch(codec, comps, caps, out=None, factor=0.0):
    """strom_zstd_host_lp over several streams, outputs GUARD bytes apart:
    (statuses, destination, LP-taken count).  factor: entry bytes per
    decoded byte of the twin's pool (0: its default, 3)."""
    n = len(comps)
    src = np.frombuffer(b"".join(comps) + b"\0", dtype=np.uint8)
    so = np.cumsum([0] + [len(b) for b in comps])[:-1]
    do = np.cumsum([0] + [c + GUARD for c in caps])[:-1]
    d = D.make_descs_arrays(so, [len(b) for b in comps], do, caps)
    if out is None:
        out = np.full(int(sum(caps)) + GUARD * n, FILL, dtype=np.uint8)
    st = np.zeros(n, dtype=np.int32)
    taken = N.lib().strom_zstd_host_lp(codec, src.ctypes.data, d.ctypes.data, n, out.ctypes.data,
                                       st.ctypes.data, factor)
    return st.tolist(), out, taken


def test_builders_refuse_illegal_forms():
    rnd = bytes(range(40))
    blk = lambda seqs, lits=("raw", rnd), tabs=None: [("comp", lits, seqs, tabs)]
    bad = [lambda: G.frame_bytes([]),
           lambda: G.frame_bytes([("raw", b"x")], fcs_bytes=2),                   # 1 < 256
           lambda: G.frame_bytes([("raw", bytes(300))], fcs_bytes=1, single=True),
           lambda: G.frame_bytes([("raw", bytes(65792))], fcs_bytes=2),
           lambda: G.frame_bytes([("raw", b"x")], fcs_bytes=0, single=True),
           lambda: G.frame_bytes([("raw", b"x")], fcs_bytes=1, single=False),
           lambda: G.frame_bytes([("raw", b"x")], did_bytes=3),
           lambda: G.frame_bytes([("raw", b"x")], did_bytes=1, did=5),
           lambda: G.frame_bytes([("raw", bytes(G.MAXB + 1))]),
           lambda: G.frame_bytes([("rle", 1, G.MAXB + 1)]),
           lambda: G.frame_bytes(blk([(5, 2, 4)]), single=True),                  # block above the content size
           lambda: G.frame_bytes(blk([(5, 6, 4)])),                               # offset past the start
           lambda: G.frame_bytes(blk([(5, 2, 2)])),                               # match length < 3
           lambda: G.frame_bytes(blk([(41, 2, 4)])),                              # more literals than present
           lambda: G.frame_bytes(blk([(5, 1, 4), (0, ("rep", 3), 4)])),           # rep[0] - 1 == 0
           lambda: G.frame_bytes(blk([(5, ("rep", 4), 4)])),
           lambda: G.frame_bytes(blk([(5, 2, G.MAXB)])),                          # block output > MAXB
           lambda: G.frame_bytes(blk([(5, 2, 4)], tabs={"ll": "repeat"})),
           lambda: G.frame_bytes(blk([(5, 2, 4)], ("treeless", b"abcabc"))),
           lambda: G.frame_bytes(blk([(5, 2, 4), (6, 2, 4)], tabs={"ll": "rle"})),
           lambda: G.frame_bytes(blk([(5, 2, 4)], tabs={"ll": ("fse", 10)})),
           lambda: G.frame_bytes(blk([(5, 2, 4)], tabs={"of": ("fse", 9)})),
           lambda: G.frame_bytes(blk([(5, 2, 4)], tabs={"ll": ("fse", 5, [16, 15])})),    # sum 31
           lambda: G.frame_bytes(blk([(5, 2, 4)], tabs={"ll": ("fse", 5, [16, 16])})),    # code 5: no probability
           lambda: G.frame_bytes(blk([(5, 2, 4)], tabs={"nseq_form": 3})),        # 3 bytes begin at 0x7F00
           lambda: G.frame_bytes(blk([(5, 2, 4)], tabs={"marker": 0}) + blk([(5, 2, 4)], tabs={"marker": 1})),
           lambda: G.nseq_field(128, 1), lambda: G.nseq_field(0x7F00, 2), lambda: G.nseq_field(0x7EFF, 3),
           lambda: G.lit_header(0, 32, fmt=0), lambda: G.lit_header(0, 4096, fmt=1),
           lambda: G.lit_header(0, 5, fmt=2),                                     # no such raw format
           lambda: G.lit_header(2, 1024, 10, fmt=1, streams=4), lambda: G.lit_header(2, 10, 10, fmt=0, streams=4),
           lambda: G.huf_weights({1: 1, 2: 2}), lambda: G.huf_weights({1: 1}),
           lambda: G.huf_weights(dict(zip(range(13), (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 12)))),
           lambda: G.huf_header(G.huf_flat_lengths(range(130)), "direct"),
           lambda: G.huf_header({0: 8, **{s: 8 for s in range(1, 256)}}, "fse"),   # one weight value: nothing to over-read
           lambda: G.huf_payload(G.huf_codes({1: 1, 2: 1}), b"\x01\x02\x01\x02\x01", 4),
           lambda: G.fse_header([16, 16], 4), lambda: G.fse_header([16, 16, 0], 5),
           lambda: G.backward_stream([(1, 1)], marker=0),
           lambda: G.skippable(16, b""), lambda: G.FwdBits().put(4, 2)]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail("case %d accepted" % i)
    # the forced forms are spelled as asked
    assert G.nseq_field(5) == b"\x05" and G.nseq_field(5, 2) == b"\x80\x05"
    assert G.nseq_field(0x7F00) == b"\xff\x00\x00" and G.nseq_field(0x7EFF) == b"\xfe\xff"
    assert G.lit_header(0, 5) == b"\x28" and G.lit_header(0, 5, fmt=1) == b"\x54\x00"
    assert G.lit_header(1, 5, fmt=3) == b"\x5d\x00\x00"
    assert G.backward_stream([(1, 1), (0, 2)]) == bytes([0b1100]) and G.marker_bit(b"\x0c") == 3
    assert G.frame_bytes([("raw", b"")]) == bytes.fromhex("28b52ffd2000010000")
    assert G.frame_bytes([("raw", bytes(256))], fcs_bytes=2)[4:7] == b"\x60\x00\x00"
    assert G.window_byte(1024) == 0 and G.window_byte(1025) == 1 and G.window_byte(3 << 20) == 0x5C


def test_family_sizes(corpora):
    """The corpora are deterministic; their sizes are part of the record."""
    sizes = {k: len(v) for k, v in corpora.items()}
    assert sizes == {"frames": 162 if G.HAVE_XXH else 146, "blocks": 21, "literals": 128,
                     "sequences": 223, "offsets": 66, "fp_carry": 49}
    for v in corpora.values():
        assert len({c.name for c in v}) == len(v)
        assert max(len(c.exp) for c in v) <= 400 << 10


@pytest.mark.parametrize("family", list(G.FAMILIES))
def test_reference_equals_libzstd(corpora, family):
    """zstdgen.decode(description) == libzstd(zstdgen.build_stream(description))."""
    for c in corpora[family]:
        if c.arrow and c.comp[:8] == b"\xff" * 8:
            assert c.comp[8:] == c.exp, c.name          # the stored form
            continue
        assert libzstd(c.comp[8:] if c.arrow else c.comp, len(c.exp)) == c.exp, c.name


@pytest.mark.parametrize("which", TWINS)
@pytest.mark.parametrize("family", list(G.FAMILIES))
def test_valid_families(corpora, family, which):
    """Every host twin, capacity exactly the decoded size: (length, bytes)
    exact, nothing written behind the capacity."""
    for c in corpora[family]:
        st, out, clean = twin(which, _codec(c), c.comp, len(c.exp))
        assert st == len(c.exp), (c.name, which, st)
        assert out == c.exp, (c.name, which)
        assert clean, (c.name, which)


@pytest.mark.parametrize("family", list(G.FAMILIES))
def test_valid_families_ops_wrapper(corpora, family):
    """The same through ops.decompress.zstd_host (every 5th case, a roomy capacity)."""
    for c in corpora[family][::5]:
        for kw in (dict(fp=0), dict(fp=G.FPW), dict(lp=True)):
            assert D.zstd_host(_codec(c), c.comp, len(c.exp) + 9, **kw) == (len(c.exp), c.exp), (c.name, kw)
    for arrow in (False, True):
        for cs in G.lp_batches([c for c in corpora[family][::5] if c.arrow == arrow]):
            if cs:
                st, outs, taken = D.zstd_host_lp(_codec(cs[0]), [c.comp for c in cs], [len(c.exp) for c in cs])
                assert (st, outs, taken) == ([len(c.exp) for c in cs], [c.exp for c in cs], sum(c.lp for c in cs))


@pytest.mark.parametrize("arrow", [False, True], ids=["zstd", "arrow"])
@pytest.mark.parametrize("family", list(G.FAMILIES))
def test_lp_batches_and_taken(corpora, family, arrow):
    """The lane-parallel twin over a family in one call: statuses, bytes,
    guards, and the LP-taken count: every stream of one data frame with
    nothing behind it is taken, multi-frame and stored streams fall back."""
    cs = [c for c in corpora[family] if c.arrow == arrow]
    if not cs:
        assert family != "frames"
        return
    total = 0
    for cs in G.lp_batches(cs):
        assert G.lp_fits(cs), cs[0].name
        caps = [len(c.exp) for c in cs]
        st, out, taken = lp_batch(_codec(cs[0]), [c.comp for c in cs], caps)
        assert st == caps, [(c.name, s) for c, s in zip(cs, st) if s != len(c.exp)][:5]
        p = 0
        for c in cs:
            assert out[p:p + len(c.exp)].tobytes() == c.exp, c.name
            assert (out[p + len(c.exp):p + len(c.exp) + GUARD] == FILL).all(), c.name
            p += len(c.exp) + GUARD
        assert taken == sum(c.lp for c in cs), cs[0].name
        total += taken - len(cs)
    assert (total < 0) == (family == "frames")      # only there: several frames, checksums, stored


def test_align_streams_decode():
    for c in G.align_streams():
        assert libzstd(c.comp[8:] if c.arrow else c.comp, len(c.exp)) == c.exp, c.name
        for which in TWINS:
            assert twin(which, _codec(c), c.comp, len(c.exp)) == (len(c.exp), c.exp, True), (c.name, which)


def test_capacity_at_kposmax():
    """Positions are 30-bit (kPosMax): a capacity of 1 GiB is refused as an
    overflow before anything is read."""
    c = G.one("x", [("raw", b"abc")])
    for which in ("wave", "fp4"):
        src = np.frombuffer(c.comp + b"\0", dtype=np.uint8)
        out = np.zeros(16, dtype=np.uint8)
        fn = N.lib().strom_zstd_host if which == "wave" else N.lib().strom_zstd_host_fp
        args = (D.ZSTD, src.ctypes.data, len(c.comp), out.ctypes.data, G.KPOSMAX) + ((G.FPW,) if which == "fp4" else ())
        assert fn(*args) == -2 and not out.any(), which


# Streams that libzstd refuses and the decoders here accept, each for a
# reason the code states:
LENIENT = {
    # the window size is not enforced: next_block() steps over the descriptor
    # byte (zstd.hip:690) and bounds a block by the format's 128 KiB alone
    # (zstd.hip:734), where the format says the smaller of that and the window
    "window_1k_block_3k",
}


# The other way round: streams the format forbids (and the decoders here
# refuse) that libzstd's one-shot call decodes without an error.
LIBZSTD_LENIENT = {
    # RFC 8878 3.1.1.2.3: Block_Size and a block's output are bounded by
    # Block_Maximum_Size (128 KiB at most); libzstd copies / decodes them
    "block_size_gt_maxb", "rle_block_gt_maxb", "block_output_gt_maxb", "block_output_gt_maxb_lits",
    # RFC 8878 4.2.2: each of the 4 Huffman streams ends on its marker,
    # consumed exactly; libzstd's 4-stream loop returns (other) bytes
    "huf_jump_shifted", "huf_stream_zero_last_byte",
}


def _libzstd_rejects(b):
    try:
        libzstd(b.comp[8:] if b.arrow else b.comp, max(b.cap, 1))
    except Exception:
        return True
    return False


def test_malformed():
    """Every malformed stream: libzstd refuses it (so it is malformed); every
    twin returns a negative status, the named one where the contract names
    it; nothing is written behind the capacity."""
    cases = G.malformed()
    assert len({b.name for b in cases}) == len(cases) and len(cases) >= 100
    assert {G.bad_family(b.name) for b in cases} == set(G.FAMILIES)     # each rides in a GPU launch
    for b in cases:
        prefix_only = b.arrow and b.status == -2 or b.name.startswith("arrow_prefix")
        cap_only = b.name.startswith("cap_one_short") or b.name == "fcs_gt_cap"
        if not prefix_only and not cap_only:     # those frames are fine; the buffer around them is not
            assert _libzstd_rejects(b) != (b.name in LIBZSTD_LENIENT), b.name
        for which in TWINS:
            st, _, clean = twin(which, D.ARROW_ZSTD if b.arrow else D.ZSTD, b.comp, b.cap)
            assert st < 0, (b.name, which, st)
            if b.status is not None:
                assert st == b.status, (b.name, which, st)
            assert clean, (b.name, which)
    # and in one lane-parallel call: none taken is not required (the walk
    # follows what is well-formed on its level), the statuses are
    for arrow in (False, True):
        bs = [b for b in cases if b.arrow == arrow]
        st, out, _ = lp_batch(D.ARROW_ZSTD if arrow else D.ZSTD, [b.comp for b in bs], [b.cap for b in bs])
        p = 0
        for b, s in zip(bs, st):
            assert s < 0 and (b.status is None or s == b.status), (b.name, s)
            assert (out[p + b.cap:p + b.cap + GUARD] == FILL).all(), b.name
            p += b.cap + GUARD


def test_lenient():
    """What libzstd refuses and the decoders take: the LENIENT table, capped
    at the cases whose reason the code states; the bounds hold all the same."""
    b, exp = G.window_lenient()
    assert {b.name} == LENIENT
    assert _libzstd_rejects(b)
    for which in TWINS:
        assert twin(which, D.ZSTD, b.comp, b.cap) == (len(exp), exp, True), which
        st, _, clean = twin(which, D.ZSTD, b.comp, b.cap - 1)
        assert st == -2 and clean, which
