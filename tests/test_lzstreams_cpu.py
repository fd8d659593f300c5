"""The hand-built LZ4 / snappy corpora of tests/lzgen.py against every
decoder that runs without a GPU: the plain reference (lzgen.decode, which
produced the expected bytes from the same sequence lists), pyarrow's
decoders, the host codecs and the block-parallel decoder's host twin in its
three geometries.  No stream is skipped or filtered: a corpus function may
only produce streams that all of them accept.  test_gpu_lzstreams.py feeds
the same corpora to the GPU decoders."""
import pytest

import lzgen as G
from nvme_strom_amd.ops import decompress as D

pa = pytest.importorskip("pyarrow")

THREADS = [256, 512, "512b"]


@pytest.fixture(scope="module")
def corpora():
    c = {("lz4", k): f() for k, f in G.LZ4_FAMILIES.items()}
    c.update({("snappy", k): f() for k, f in G.SNAPPY_FAMILIES.items()})
    return c


def _par_all(codec, comp, exp, name, cap=None):
    for th in THREADS:
        st, out, _ = D.lz4par_host(codec, comp, len(exp) if cap is None else cap, th)
        assert st == len(exp), (name, th, st)
        assert out == exp, (name, th)


def test_builders_refuse_illegal_forms():
    bad = [lambda: G.snappy_elem_bytes(("C", 5, 12, 1)), lambda: G.snappy_elem_bytes(("C", 5, 3, 1)),
           lambda: G.snappy_elem_bytes(("C", 2048, 5, 1)), lambda: G.snappy_elem_bytes(("C", 65536, 5, 2)),
           lambda: G.snappy_elem_bytes(("C", 5, 65, 3)), lambda: G.snappy_elem_bytes(("C", 0, 5, 2)),
           lambda: G.snappy_elem_bytes(("L", b"x" * 61, 0)), lambda: G.snappy_elem_bytes(("L", b"x" * 257, 1)),
           lambda: G.snappy_stream([("L", b"abc", None), ("C", 4, 4, 1)], 7),
           lambda: G.varint(128, 1),
           lambda: G.lz4_block([(b"abc", 4, 4), (b"x" * 12, None, 0)]),
           lambda: G.lz4_block([(b"abc", 0, 4), (b"x" * 12, None, 0)]),
           lambda: G.lz4_block([(b"abc", 1, 3), (b"x" * 12, None, 0)]),
           lambda: G.lz4_block([(b"abc", 1, 4), (b"x" * 4, None, 0)]),
           lambda: G.lz4_block([(b"abc", 1, 4), (b"x" * 7, None, 0)]),
           lambda: G.lz4_block([(b"abc", 1, 4)]),
           lambda: G.lz4_block([(b"x" * 15, 1, 4), (b"x" * 12, None, 0)], {0: (2, None)}),
           lambda: G.lz4_frame([("stored", b"")])]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail("case %d accepted" % i)
    # the padded forms are spelled as asked
    assert G.varint(0, 5) == b"\x80\x80\x80\x80\x00" and G.varint(300) == b"\xac\x02"
    assert G.snappy_elem_bytes(("L", b"ab", 4)) == bytes([63 << 2, 1, 0, 0, 0]) + b"ab"
    assert G.lz4_seq_bytes(b"", 7, 4 + 15 + 255) == bytes([0x0F, 7, 0, 255, 0])
    assert G.lz4_block([(b"x" * 15, 1, 4), (b"x" * 12, None, 0)], {0: (1, None)})


def test_family_sizes(corpora):
    """The corpora are deterministic; their sizes are part of the record."""
    sizes = {"%s/%s" % k: len(v) for k, v in corpora.items()}
    assert sizes == {"lz4/lengths": 1120, "lz4/far": 687, "lz4/window": 1956, "lz4/par_edges": 47,
                     "lz4/random": 300, "snappy/literals": 96, "snappy/copies": 669,
                     "snappy/window": 1956, "snappy/random": 300}
    for v in corpora.values():
        assert len({c[0] for c in v}) == len(v)


@pytest.mark.parametrize("family", list(G.LZ4_FAMILIES))
def test_lz4_raw_families(corpora, family):
    for name, comp, exp in corpora["lz4", family]:
        got = pa.decompress(comp, decompressed_size=len(exp), codec="lz4_raw", asbytes=True)
        assert got == exp, name
        assert D.lz4_decompress(comp, len(exp)) == exp, name
        _par_all(D.LZ4, comp, exp, name)


@pytest.mark.parametrize("family", list(G.SNAPPY_FAMILIES))
def test_snappy_families(corpora, family):
    for name, comp, exp in corpora["snappy", family]:
        got = pa.decompress(comp, decompressed_size=len(exp), codec="snappy", asbytes=True)
        assert got == exp, name
        assert D.snappy_decompress(comp, len(exp)) == exp, name
        _par_all(D.SNAPPY, comp, exp, name)


def test_snappy_preambles():
    for name, comp, exp, cap in G.snappy_preambles():
        assert pa.decompress(comp, decompressed_size=len(exp), codec="snappy", asbytes=True) == exp, name
        assert D.snappy_decompress(comp, cap) == exp, name
        _par_all(D.SNAPPY, comp, exp, name, cap)


def test_lz4_frames_and_arrow_buffers():
    for name, frame, exp in G.lz4_frames():
        if G.HAVE_XXH:      # pyarrow verifies the header checksum
            assert pa.decompress(frame, decompressed_size=len(exp), codec="lz4", asbytes=True) == exp, name
        body, bcs = G.frame_body(frame)
        info = D.parse_lz4_frame_header(frame)
        assert frame[info.data_offset:] == body and info.block_checksum == bcs, name
        _par_all(D.LZ4_FRAME_BCS if bcs else D.LZ4_FRAME, body, exp, name)
    for name, buf, exp in G.arrow_buffers():
        _par_all(D.ARROW_LZ4, buf, exp, name)
        _par_all(D.ARROW_LZ4, buf, exp, name, len(exp) + 9)


def test_align_streams_decode():
    a = G.align_streams()
    c, e = a["lz4"]
    assert 550 <= len(e) <= 650
    assert pa.decompress(c, decompressed_size=len(e), codec="lz4_raw", asbytes=True) == e
    _par_all(D.LZ4, c, e, "align")
    c, e = a["snappy"]
    assert 550 <= len(e) <= 650
    assert pa.decompress(c, decompressed_size=len(e), codec="snappy", asbytes=True) == e
    _par_all(D.SNAPPY, c, e, "align")


# liblz4 does not look at a zero offset (the match then "copies" from the
# write position: whatever bytes it returns, no valid stream says so); every
# other malformed stream pyarrow must refuse outright
PYARROW_LENIENT = {("lz4", "off0")}


def _pyarrow_rejects(codec, comp, cap):
    try:
        pa.decompress(comp, decompressed_size=cap, codec=codec, asbytes=True)
    except Exception:
        return True
    return False


@pytest.mark.parametrize("which", ["lz4", "snappy", "arrow"])
def test_malformed(which):
    """Every malformed stream is refused by pyarrow, by the host codecs and
    by the host twin: < 0, and -2 exactly where the capacity is what is wrong."""
    cases, codec, pac = {"lz4": (G.lz4_malformed, D.LZ4, "lz4_raw"),
                         "snappy": (G.snappy_malformed, D.SNAPPY, "snappy"),
                         "arrow": (G.arrow_malformed, D.ARROW_LZ4, None)}[which]
    for name, comp, cap, want in cases():
        if pac and (which, name) not in PYARROW_LENIENT:
            assert _pyarrow_rejects(pac, comp, cap), name
        for th in THREADS:
            st = D.lz4par_host(codec, comp, cap, th)[0]
            assert st < 0, (name, th, st)
            if want is not None:
                assert st == want, (name, th, st)
        host = D.lz4_decompress if which == "lz4" else D.snappy_decompress if which == "snappy" else None
        if host:
            with pytest.raises(ValueError):
                host(comp, cap)
