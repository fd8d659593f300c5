"""The hand-built Zstandard corpora of tests/zstdgen.py on the three GPU
decoders of csrc/kernels/zstd.hip: one wave per stream, frame-parallel and
lane-parallel (test_zstdstreams_cpu.py pins the same corpora against
libzstd and the decoders' host twins).

One launch decodes a family's valid streams and then its malformed ones,
outputs back to back, capacities the exact decoded sizes, a guard region
behind the last.  Asserted, exactly: every status and byte of the valid
streams; each malformed stream's status against the same decoder's host
twin; the guard; and on the lane-parallel decoder the count of streams it
took against its twin's (test_gpu_kernels._run_lp).  Every stream here is
bounded and every malformed one ends in a clean status on the host twins."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import zstdgen as G
from nvme_strom_amd import _native as N
from nvme_strom_amd.ops import decompress as D
from nvme_strom_amd.ops._util import stream_handle
from test_gpu_kernels import _run, zmode  # noqa: F401  (zmode: the three-decoder fixture)

pytestmark = pytest.mark.gpu

GUARD = 256


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def corp():
    """Every corpus once: {family: [Case]}, {family: [Bad]}, and the host
    twins' statuses of the malformed streams, {(name, mode): status}."""
    good = {k: f() for k, f in G.FAMILIES.items()}
    bad = {k: [] for k in G.FAMILIES}
    for b in G.malformed():
        bad[G.bad_family(b.name)].append(b)
    assert all(bad.values())
    return good, bad, {}


def _twin_status(cache, b, mode):
    if (b.name, mode) not in cache:
        codec = D.ARROW_ZSTD if b.arrow else D.ZSTD
        cache[b.name, mode] = D.zstd_host(codec, b.comp, b.cap, fp=G.FPW if mode == 1 else 0, lp=mode == 2)[0]
    return cache[b.name, mode]


def _guard(arrow):
    """The launch's last stream: no frame at all (0 bytes decode to 0 bytes;
    behind the Arrow prefix, a length of 0) with the guard region as its
    capacity."""
    g = G.Case("guard", G.arrow_zstd(0, b"") if arrow else b"", b"", arrow, False, 0, 0)
    g.cap = GUARD
    return g


def _family(dev, corp, mode, family, arrow):
    good, bad, cache = corp
    cs = [c for c in good[family] if c.arrow == arrow]
    bs = [b for b in bad[family] if b.arrow == arrow]
    n_launch = 0
    for part in G.lp_batches(cs + bs):
        # the launch fits the lane-parallel pool (with the guard stream), so
        # the streams it takes do not depend on the order of the walks
        assert G.lp_fits(part + [_guard(arrow)])
        vs = [c for c in part if isinstance(c, G.Case)]
        ms = [b for b in part if isinstance(b, G.Bad)]
        items = vs + ms + [_guard(arrow)]
        st, outs = _run(D.ARROW_ZSTD if arrow else D.ZSTD, [c.comp for c in items], [c.cap for c in items], dev)
        st = [int(x) for x in st]
        wrong = [(c.name, s, len(c.exp)) for c, s in zip(vs, st) if s != len(c.exp)]
        assert not wrong, wrong[:5]
        for c, o in zip(vs, outs):
            assert o == c.exp, c.name
        got = [(b.name, s) for b, s in zip(ms, st[len(vs):])]
        print("\n%s mode %d:" % (family, mode), got)
        for b, s in zip(ms, st[len(vs):]):
            assert s < 0 and s == _twin_status(cache, b, mode), (b.name, s, _twin_status(cache, b, mode))
            assert b.status is None or s == b.status, (b.name, s)
        assert st[-1] == 0 and outs[-1] == bytes(GUARD), "guard"
        n_launch += 1
    return n_launch


@pytest.mark.parametrize("family", list(G.FAMILIES))
def test_families(dev, corp, zmode, family):
    _family(dev, corp, zmode, family, False)


def test_frames_arrow(dev, corp, zmode):
    """The frames family behind the Arrow length prefix, the stored form,
    and the malformed prefixes."""
    _family(dev, corp, zmode, "frames", True)


def test_alignment(dev, zmode):
    """A small mixed subset at every source misalignment 0..7 x destination
    misalignment 0..3 (the kernels load their windows by dwords): one launch
    per codec, explicit descriptors."""
    for arrow in (False, True):
        cs = [c for c in G.align_streams() if c.arrow == arrow]
        items = [(c, s, d) for c in cs for s in range(8) for d in range(4)]
        soff, doff, sp, dp = [], [], 0, 0
        for c, s, d in items:
            sp = ((sp + 7) & ~7) + s
            dp = ((dp + 3) & ~3) + 4 + d            # >= 1 guard byte between the outputs
            soff.append(sp)
            doff.append(dp)
            sp += len(c.comp)
            dp += len(c.exp)
        assert {(a % 8, b % 4) for a, b in zip(soff, doff)} == {(s, d) for s in range(8) for d in range(4)}
        src = np.zeros(sp + 64, np.uint8)
        for (c, _, _), o in zip(items, soff):
            src[o:o + len(c.comp)] = np.frombuffer(c.comp, np.uint8)
        want = np.full(dp + GUARD, 0xA5, np.uint8)
        for (c, _, _), o in zip(items, doff):
            want[o:o + len(c.exp)] = np.frombuffer(c.exp, np.uint8)
        descs = D.make_descs_arrays(soff, [len(c.comp) for c, _, _ in items], doff,
                                    [len(c.exp) for c, _, _ in items])
        codec = D.ARROW_ZSTD if arrow else D.ZSTD
        d_src = torch.from_numpy(src).to(dev)
        dst = torch.full((len(want),), 0xA5, dtype=torch.uint8, device=dev)
        if zmode == 2:
            d_desc = torch.from_numpy(descs.view(np.uint8).copy()).to(dev)
            status = torch.empty(len(items), dtype=torch.int32, device=dev)
            s = torch.cuda.Stream(device=dev)
            torch.cuda.synchronize()
            D.decompress_async(codec, d_src, dst, d_desc, status, stream=s, zstd_mode=D.ZSTD_LP)
            cnt = np.zeros(4, np.uint64)
            assert N.lib().strom_zstd_lp_last(stream_handle(s), cnt.ctypes.data) == 0
            st = status.cpu().numpy()
            assert int(cnt[1]) == len(items)            # every one a single plain frame
        else:
            st = D.decompress(codec, d_src, dst, descs)
        assert st.tolist() == [len(c.exp) for c, _, _ in items]
        out = dst.cpu().numpy()
        diff = np.nonzero(out != want)[0]
        assert len(diff) == 0, (len(diff), diff[:5].tolist())
