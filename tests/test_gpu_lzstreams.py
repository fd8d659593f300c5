"""The hand-built LZ4 / snappy / COPY corpora of tests/lzgen.py on every GPU
decoder: the lane-group decoder's 8 geometries (decompress.hip) and the
block-parallel decoder's 3 builds (lz4par*.hip).  The lane decoder has no
host twin, so this is its check at its own edges (test_lzstreams_cpu.py
pins the same corpora against pyarrow, the host codecs and the
block-parallel host twin).

Every test is one launch per pass over one layout: the destination is
pre-filled with 0xA5, the outputs lie (i % 37) + 1 guard bytes apart, the
capacities are the exact decoded sizes and, in a second pass, 1..17 bytes
more.  Asserted, exactly: every status, every decoded byte, and that no byte
outside the streams' own [dst_off, dst_off + dst_len) ranges changed."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import lzgen as G
from nvme_strom_amd.ops import decompress as D

pytestmark = pytest.mark.gpu

FILL = 0xA5
LANES = [1, 2, 3, 4, 6, 8, 16, 32]
DECODERS = LANES + ["par256", "par512", "par8192"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def corp():
    """Every corpus once: {key: [(name, compressed, expected, capacity)]} for
    the valid streams (capacity None = the decoded size)."""
    c = {}
    for k, f in G.LZ4_FAMILIES.items():
        c["lz4", k] = [(n, s, e, None) for n, s, e in f()]
    for k, f in G.SNAPPY_FAMILIES.items():
        c["snappy", k] = [(n, s, e, None) for n, s, e in f()]
    c["snappy", "preambles"] = G.snappy_preambles()
    frames = [(n,) + G.frame_body(f) + (e,) for n, f, e in G.lz4_frames()]
    c["frame", "nobcs"] = [(n, b, e, None) for n, b, bcs, e in frames if not bcs]
    c["frame", "bcs"] = [(n, b, e, None) for n, b, bcs, e in frames if bcs]
    c["frame", "arrow"] = [(n, s, e, None) for n, s, e in G.arrow_buffers()]
    c["copy", "sizes"] = [(n, s, e, None) for n, s, e in G.copy_streams()]
    c["layouts"] = {}
    return c


def _set_decoder(monkeypatch, g):
    if str(g).startswith("par"):
        monkeypatch.setenv("STROM_DECOMP_PAR", g[3:])
    else:
        monkeypatch.setenv("STROM_DECOMP_PAR", "0")
        monkeypatch.setenv("STROM_DECOMP_G", str(g))


class Layout:
    """One launch.  items: (name, compressed, expected | None, capacity |
    None); expected None = a malformed stream (its capacity range is not
    compared).  slack: capacities 1..17 bytes above the decoded size.
    src_mis / dst_mis: per-stream misalignment to 16 bytes (default: sources
    16-aligned, so a stream's input positions are the decoder's own;
    destinations wherever the guards put them)."""

    def __init__(self, items, slack=False, src_mis=None, dst_mis=None):
        n = len(items)
        self.names = [it[0] for it in items]
        self.good = np.array([it[2] is not None for it in items])
        self.lens = np.array([len(it[2]) if it[2] is not None else -1 for it in items], np.int64)
        soff, doff, caps = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
        sp = dp = 0
        for i, (_, comp, exp, cap) in enumerate(items):
            sp = (sp + 15) & ~15
            if src_mis is not None:
                sp += src_mis[i]
            soff[i] = sp
            sp += len(comp)
            dp += (i % 37) + 1
            if dst_mis is not None:
                dp += (dst_mis[i] - dp) % 16
            doff[i] = dp
            caps[i] = (len(exp) if cap is None else cap) + ((1 + i % 17) if slack else 0)
            dp += caps[i]
        self.src = np.zeros(sp + 256, np.uint8)
        self.want = np.full(dp + 64, FILL, np.uint8)
        self.care = np.ones(dp + 64, bool)
        for i, (_, comp, exp, _) in enumerate(items):
            self.src[soff[i]:soff[i] + len(comp)] = np.frombuffer(comp, np.uint8)
            if exp is None:
                self.care[doff[i]:doff[i] + caps[i]] = False
            else:
                self.want[doff[i]:doff[i] + len(exp)] = np.frombuffer(exp, np.uint8)
                self.care[doff[i] + len(exp):doff[i] + caps[i]] = False
        self.doff, self.caps = doff, caps
        self.descs = D.make_descs_arrays(soff, [len(it[1]) for it in items], doff, caps)

    def run(self, codec, dev):
        dst = torch.full((len(self.want),), FILL, dtype=torch.uint8, device=dev)
        st = D.decompress(codec, torch.from_numpy(self.src).to(dev), dst, self.descs)
        return st.astype(np.int64), dst.cpu().numpy()

    def check(self, st, out):
        """Statuses and bytes of the good streams, and the guards."""
        bad = np.nonzero(self.good & (st != self.lens))[0]
        assert len(bad) == 0, ("status", len(bad), [(self.names[i], int(st[i]), int(self.lens[i]))
                                                    for i in bad[:5]])
        diff = np.nonzero((out != self.want) & self.care)[0]
        if len(diff):
            where = []
            for j in diff[:5]:
                i = int(np.searchsorted(self.doff, j, "right")) - 1
                inside = i >= 0 and j < self.doff[i] + self.caps[i]
                where.append((self.names[max(i, 0)], "output byte" if inside else "guard byte after",
                              int(j - self.doff[max(i, 0)]), int(out[j]), int(self.want[j])))
            pytest.fail("%d bytes differ: %r" % (len(diff), where))


def _both_passes(corp, key, codec, dev):
    for slack in (False, True):
        lay = corp["layouts"].get((key, slack))
        if lay is None:
            lay = corp["layouts"][key, slack] = Layout(corp[key], slack)
        st, out = lay.run(codec, dev)
        lay.check(st, out)


@pytest.mark.parametrize("g", DECODERS)
@pytest.mark.parametrize("family", list(G.LZ4_FAMILIES))
def test_lz4_raw(dev, corp, monkeypatch, family, g):
    _set_decoder(monkeypatch, g)
    _both_passes(corp, ("lz4", family), D.LZ4, dev)


@pytest.mark.parametrize("g", DECODERS)
@pytest.mark.parametrize("family", list(G.SNAPPY_FAMILIES) + ["preambles"])
def test_snappy(dev, corp, monkeypatch, family, g):
    """"preambles" carries its own capacities (the declared length, and
    above it); its second pass adds the slack on top."""
    _set_decoder(monkeypatch, g)
    _both_passes(corp, ("snappy", family), D.SNAPPY, dev)


@pytest.mark.parametrize("g", DECODERS)
@pytest.mark.parametrize("kind", ["nobcs", "bcs", "arrow"])
def test_lz4_frames(dev, corp, monkeypatch, kind, g):
    _set_decoder(monkeypatch, g)
    codec = {"nobcs": D.LZ4_FRAME, "bcs": D.LZ4_FRAME_BCS, "arrow": D.ARROW_LZ4}[kind]
    _both_passes(corp, ("frame", kind), codec, dev)


@pytest.mark.parametrize("g", LANES)
def test_copy(dev, corp, monkeypatch, g):
    _set_decoder(monkeypatch, g)
    _both_passes(corp, ("copy", "sizes"), D.COPY, dev)


def _alignment(dev, corp, codec):
    comp, exp = G.align_streams()[codec]
    items = [("align_s%d_d%d" % (s, d), comp, exp, None) for s in range(16) for d in range(16)]
    mis_s = [s for s in range(16) for _ in range(16)]
    mis_d = [d for _ in range(16) for d in range(16)]
    for slack in (False, True):
        lay = corp["layouts"].get(("align", codec, slack))
        if lay is None:
            lay = corp["layouts"]["align", codec, slack] = Layout(items, slack, mis_s, mis_d)
        assert ((lay.descs["src_off"] % 16).tolist(), (lay.descs["dst_off"] % 16).tolist()) == (mis_s, mis_d)
        st, out = lay.run({"lz4": D.LZ4, "snappy": D.SNAPPY, "copy": D.COPY}[codec], dev)
        lay.check(st, out)


@pytest.mark.parametrize("g", DECODERS)
@pytest.mark.parametrize("codec", ["lz4", "snappy"])
def test_alignment(dev, corp, monkeypatch, codec, g):
    """One stream at every source misalignment x every destination
    misalignment (16 x 16) in one launch."""
    _set_decoder(monkeypatch, g)
    _alignment(dev, corp, codec)


@pytest.mark.parametrize("g", LANES)
def test_alignment_copy(dev, corp, monkeypatch, g):
    _set_decoder(monkeypatch, g)
    _alignment(dev, corp, "copy")


@pytest.mark.parametrize("g", DECODERS)
@pytest.mark.parametrize("which", ["lz4", "snappy", "arrow"])
def test_malformed(dev, corp, monkeypatch, which, g):
    """Streams wrong in exactly one place, after 20 good ones in the same
    launch: the good ones decode exactly, each malformed one reports an
    error (-2 exactly where the capacity is what is wrong: the documented
    contract of decompress()), and nothing outside a stream's capacity is
    written."""
    _set_decoder(monkeypatch, g)
    cases, codec, good = {"lz4": (G.lz4_malformed, D.LZ4, corp["lz4", "random"]),
                          "snappy": (G.snappy_malformed, D.SNAPPY, corp["snappy", "random"]),
                          "arrow": (G.arrow_malformed, D.ARROW_LZ4, corp["frame", "arrow"])}[which]
    bad = cases()
    lay = corp["layouts"].get(("malformed", which))
    if lay is None:
        lay = corp["layouts"]["malformed", which] = Layout(
            list(good[:20]) + [(n, s, None, cap) for n, s, cap, _ in bad])
    st, out = lay.run(codec, dev)
    print("\n%s %s:" % (which, g), [(n, int(x)) for (n, _, _, _), x in zip(bad, st[20:])])
    lay.check(st, out)
    for (name, _, _, want), x in zip(bad, st[20:].tolist()):
        assert x < 0, (name, x)
        if want is not None:
            assert x == want, (name, x, want)


@pytest.mark.parametrize("g", [1, 3])
@pytest.mark.parametrize("codec", ["lz4", "snappy"])
def test_grid_stride_trip(dev, monkeypatch, codec, g):
    """16385 streams on the one-stream-per-wave geometries: one more than
    the launch's cap of 16384 waves, so one wave takes a second stream."""
    _set_decoder(monkeypatch, g)
    rng = np.random.default_rng(9)
    if codec == "lz4":
        seqs = [(G._rnd(rng, 10), 3, 14), (G._rnd(rng, 16), None, 0)]
        comp, exp = G.lz4_block(seqs), bytes(G.decode(seqs))
    else:
        elems = [("L", G._rnd(rng, 10), None), ("C", 3, 14, 2), ("L", G._rnd(rng, 16), 1)]
        exp = bytes(G.decode(elems))
        comp = G.snappy_stream(elems, len(exp))
    assert len(exp) == 40
    lay = Layout([("copy%d" % i, comp, exp, None) for i in range(16385)])
    st, out = lay.run(D.LZ4 if codec == "lz4" else D.SNAPPY, dev)
    lay.check(st, out)
