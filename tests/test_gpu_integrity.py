"""GPU tests (MI355X) of the integrity kernels, csrc/kernels/crc32c.hip and
csrc/kernels/copyops.hip, at every schedule and edge of their own launch
arithmetic (the case lists of tests/integritygen.py; test_integrity_cpu.py
proves that the lists reach each path).

Every comparison is exact equality: CRCs against the host CRC (and the
bit-at-a-time reference for small inputs), copies against numpy indexing,
verify results against a numpy count of differing words.  Outputs are
pre-filled with a sentinel, so a value the kernel never wrote shows."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import integritygen as G

pytestmark = pytest.mark.gpu

SENT32 = 0x5A5A5A5A


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nvme_strom_amd as S
    S.configure(gpu_emulation=0, backend="uring", max_request=1 << 20, workers=4,
                pgcache_probe=1, direct_io=1)
    return S


@pytest.fixture(scope="module")
def V(S):
    from nvme_strom_amd.ops import verify
    return verify


def _dev(a, device="cuda"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8)


def _host_chunks(S, data, chunk, n=None):
    n = len(data) if n is None else n
    return np.array([S.crc32c_host(data[i:min(i + chunk, n)]) for i in range(0, n, chunk)],
                    dtype=np.uint32)


def _chunks(V, dev, chunk, nbytes=None, stream=None):
    """crc32c_chunks into a sentinel-filled ``out``."""
    n = dev.numel() if nbytes is None else nbytes
    out = torch.full(((n + chunk - 1) // chunk,), SENT32, dtype=torch.int32, device=dev.device)
    if stream is not None:
        torch.cuda.synchronize()             # the fill ran on the current stream
    assert V.crc32c_chunks(dev, chunk, nbytes, out=out, stream=stream) is out
    if stream is not None:
        stream.synchronize()
    return V.u32(out)


def _same(got, ref, what=""):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, (what, "first difference at", int(bad[0]), "of", int(bad.size),
                           hex(int(got[bad[0]])), hex(int(ref[bad[0]])))


# ---------------------------------------------------------------- crc32c_chunks
@pytest.mark.parametrize("cid,n,chunk,kind", G.CRC_CASES, ids=[c[0] for c in G.CRC_CASES])
def test_crc32c_case(S, V, cid, n, chunk, kind):
    data = G.make_data(kind, n, seed=n + chunk)
    dev = _dev(data)
    ref = _host_chunks(S, data, chunk)
    _same(_chunks(V, dev, chunk), ref, cid)
    whole = S.crc32c_host(data)
    assert V.crc32c(dev, chunk=chunk) == whole
    if n <= 4096:
        assert whole == G.crc32c_bitwise(data)
    if kind == "ones" or kind.startswith("onebit"):
        zeros = np.zeros(n, dtype=np.uint8)
        assert whole != S.crc32c_host(zeros)
        zref = _host_chunks(S, zeros, chunk)
        touched = np.arange(len(ref)) if kind == "ones" else [int(kind.split(":")[1]) // chunk]
        assert np.all(ref[touched] != zref[touched])


def test_crc32c_wave_length_sweep(S, V):
    """One 4 KiB buffer, nbytes = L: every remainder shape of one wave."""
    data = _rand(G.SWEEP_BUF, 11)
    dev = _dev(data)
    for L in G.SWEEP_LENGTHS:
        ref = _host_chunks(S, data, G.SWEEP_CHUNK, L)
        bit = [G.crc32c_bitwise(data[i:min(i + G.SWEEP_CHUNK, L)])
               for i in range(0, L, G.SWEEP_CHUNK)]
        assert ref.tolist() == bit, L
        _same(_chunks(V, dev, G.SWEEP_CHUNK, nbytes=L), ref, L)
        whole = V.crc32c(dev, nbytes=L, chunk=G.SWEEP_CHUNK)
        assert whole == S.crc32c_host(data[:L]) == G.crc32c_bitwise(data[:L]), L


# ---------------------------------------------------------------- combine
@pytest.fixture(scope="module")
def combo(S):
    """Per chunk size, once: (random data for the largest case, the host CRC
    of each of its whole chunks, the data on the device)."""
    made = {}

    def get(chunk):
        if chunk not in made:
            k = max(k for c, k in G.COMBINE_CASES if c == chunk)
            data = _rand(chunk * k, chunk)
            made[chunk] = (data, _host_chunks(S, data, chunk), _dev(data))
        return made[chunk]
    return get


@pytest.mark.parametrize("chunk,nchunks", G.COMBINE_CASES)
def test_crc32c_combine(S, V, combo, chunk, nchunks):
    """strom_crc32c_combine alone on host-computed per-chunk CRCs; from 7169
    chunks (8 and more per thread) also chunks + combine end to end."""
    from nvme_strom_amd.ops._util import lib, ptr, stream_handle
    data, full, dev = combo(chunk)
    for n in G.combine_lengths(chunk, nchunks):
        crcs = full[:nchunks].copy()
        crcs[-1] = S.crc32c_host(data[(nchunks - 1) * chunk:n])
        d_crcs = _dev(crcs.view(np.int32))
        out = torch.full((1,), SENT32, dtype=torch.int32, device="cuda")
        rc = lib().strom_crc32c_combine(ptr(d_crcs), nchunks, chunk, n, ptr(out), stream_handle())
        assert rc == 0
        want = S.crc32c_host(data[:n])
        assert int(V.u32(out)[0]) == want, (n, n % chunk)
        if nchunks >= 7169:
            assert V.crc32c(dev, nbytes=n, chunk=chunk) == want, (n, n % chunk)


# ---------------------------------------------------------------- wrapper surface
def test_crc32c_nbytes_ignores_trailing_bytes(S, V):
    data = _rand(10000, 21)
    dev = _dev(data)
    n, chunk = 5000, 1024
    ref = _host_chunks(S, data, chunk, n)
    _same(_chunks(V, dev, chunk, nbytes=n), ref)
    assert V.crc32c(dev, nbytes=n, chunk=chunk) == S.crc32c_host(data[:n])
    dev[n:] = 0x77
    _same(_chunks(V, dev, chunk, nbytes=n), ref)
    assert V.crc32c(dev, nbytes=n, chunk=chunk) == S.crc32c_host(data[:n])
    assert V.crc32c_chunks(dev, chunk, nbytes=n).numel() == 5


@pytest.mark.parametrize("off", [16, 1040])
def test_crc32c_interior_slice(S, V, off):
    data = _rand(1040 + 40000, 22)
    dev = _dev(data)
    for chunk in (1024, 16384):
        _same(_chunks(V, dev[off:], chunk), _host_chunks(S, data[off:], chunk), chunk)
        assert V.crc32c(dev[off:], chunk=chunk) == S.crc32c_host(data[off:])


def test_crc32c_out_reuse(S, V):
    a, b = _rand(9 * 4096 + 7, 23), _rand(9 * 4096 + 7, 24)
    out = torch.full((10,), SENT32, dtype=torch.int32, device="cuda")
    assert V.crc32c_chunks(_dev(a), 4096, out=out) is out
    _same(V.u32(out), _host_chunks(S, a, 4096))
    assert V.crc32c_chunks(_dev(b), 4096, out=out) is out
    _same(V.u32(out), _host_chunks(S, b, 4096))


def test_crc32c_on_side_stream(S, V):
    data = _rand(300 * 4096 + 33, 25)
    dev = _dev(data)
    big = _dev(data[:5 * 32768 + 3])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    _same(_chunks(V, dev, 4096, stream=s), _host_chunks(S, data, 4096))
    _same(_chunks(V, big, 32768, stream=s), _host_chunks(S, data[:big.numel()], 32768))
    # the whole-buffer forms allocate and read back on the current stream
    out = torch.full((1,), SENT32, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        crc = V.crc32c(dev, chunk=4096)
        V.crc32c_into(dev, out, chunk=4096, stream=s)
    s.synchronize()
    assert crc == S.crc32c_host(data)
    assert int(V.u32(out)[0]) == S.crc32c_host(data)


def test_crc32c_into_and_empty(S, V):
    data = _rand(70000, 26)
    dev = _dev(data)
    for chunk in (16, 4096, 1 << 16):
        out = torch.full((1,), SENT32, dtype=torch.int32, device="cuda")
        V.crc32c_into(dev, out, chunk=chunk)
        assert int(V.u32(out)[0]) == V.crc32c(dev, chunk=chunk) == S.crc32c_host(data)
    empty = torch.empty(0, dtype=torch.uint8, device="cuda")
    out = torch.full((1,), SENT32, dtype=torch.int32, device="cuda")
    V.crc32c_into(empty, out)
    assert int(V.u32(out)[0]) == 0
    assert V.crc32c(empty) == 0 == S.crc32c_host(b"")
    assert V.crc32c(dev, nbytes=0) == 0
    # no chunks of no bytes: an empty list, nothing written
    out = torch.full((4,), SENT32, dtype=torch.int32, device="cuda")
    assert V.crc32c_chunks(dev, 4096, nbytes=0, out=out) is out
    assert V.crc32c_chunks(dev, 4096, nbytes=0).numel() == 0
    assert V.crc32c_chunks(empty, 4096).numel() == 0
    assert V.u32(out).tolist() == [SENT32] * 4


def test_crc32c_refusals(S, V):
    from nvme_strom_amd.ops._util import lib, ptr, stream_handle
    data = _rand(4096 + 16, 27)
    dev = _dev(data)
    out = torch.full((300,), SENT32, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match=r"rc=-22"):
        V.crc32c_chunks(dev[1:], 16, out=out)
    with pytest.raises(RuntimeError, match=r"rc=-22"):
        V.crc32c_chunks(dev, 24, out=out)
    with pytest.raises(RuntimeError, match=r"rc=-22"):
        V.crc32c_chunks(dev, 8, out=out)
    with pytest.raises(RuntimeError, match=r"rc=-22"):
        V.crc32c(dev[1:], chunk=16)
    with pytest.raises(RuntimeError, match=r"rc=-22"):
        V.crc32c(dev, chunk=24)
    # combine: nchunks must be ceil(nbytes / chunk)
    crcs = torch.zeros(8, dtype=torch.int32, device="cuda")
    one = torch.full((1,), SENT32, dtype=torch.int32, device="cuda")
    for nchunks, chunk, nbytes in [(4, 16, 48), (4, 16, 65), (4, 16, 100), (0, 16, 0), (1, 16, 0),
                                   (4, 0, 64), (2, 16, 16)]:
        rc = lib().strom_crc32c_combine(ptr(crcs), nchunks, chunk, nbytes, ptr(one),
                                        stream_handle())
        assert rc == -22, (nchunks, chunk, nbytes)
    torch.cuda.synchronize()
    assert V.u32(out).tolist() == [SENT32] * 300
    assert V.u32(one).tolist() == [SENT32]


def test_crc32c_second_device(S, V):
    """The chunk kernel asks for 128 KiB of dynamic LDS; the request is made
    once per process, and both devices must still launch (a refused launch
    is rc=-5, a RuntimeError here)."""
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU")
    data = _rand(5 * 32768 + 1027, 28)
    for chunk in (4096, 32768):
        ref = _host_chunks(S, data, chunk)
        _same(_chunks(V, _dev(data, "cuda:0"), chunk), ref, ("cuda:0", chunk))
        with torch.cuda.device(1):
            d1 = _dev(data, "cuda:1")
            _same(_chunks(V, d1, chunk), ref, ("cuda:1", chunk))
            assert V.crc32c(d1, chunk=chunk) == S.crc32c_host(data)


# ---------------------------------------------------------------- scatter / gather
def _guarded(nslots, chunk):
    """A sentinel-filled buffer of nslots chunks with one guard chunk on each
    side -> (whole buffer, the interior view)."""
    buf = torch.full(((nslots + 2) * chunk,), G.SENTINEL, dtype=torch.uint8, device="cuda")
    return buf, buf[chunk:(nslots + 1) * chunk]


def _check_guarded(buf, ref2d, chunk, what):
    h = buf.cpu().numpy().reshape(-1, chunk)
    assert np.all(h[0] == G.SENTINEL) and np.all(h[-1] == G.SENTINEL), (what, "guard")
    bad = np.flatnonzero((h[1:-1] != ref2d).any(axis=1))
    assert bad.size == 0, (what, "chunks", bad[:8].tolist())


@pytest.mark.parametrize("cid,chunk,n", G.COPY_CASES, ids=[c[0] for c in G.COPY_CASES])
def test_scatter_gather_case(S, cid, chunk, n):
    from nvme_strom_amd.ops.reorder import chunk_gather, chunk_scatter
    src_h = _rand(n * chunk, chunk + n).reshape(n, chunk)
    src = _dev(src_h.reshape(-1))
    for kind in G.COPY_PERMS:
        perm = G.make_perm(kind, n, seed=n)
        buf, dst = _guarded(n, chunk)
        chunk_scatter(src, dst, perm, chunk)
        ref = np.empty_like(src_h)
        ref[perm] = src_h
        _check_guarded(buf, ref, chunk, (kind, "scatter"))
        buf, dst = _guarded(n, chunk)
        chunk_gather(src, dst, perm, chunk)
        _check_guarded(buf, src_h[perm], chunk, (kind, "gather"))


@pytest.mark.parametrize("chunk", [16, 4112, 12288])
def test_scatter_partial_keeps_unnamed_slots(S, chunk):
    from nvme_strom_amd.ops.reorder import chunk_scatter
    n, slots = 97, 300
    src_h = _rand((n + 3) * chunk, chunk).reshape(n + 3, chunk)
    pos = np.sort(np.random.default_rng(chunk).choice(slots, n, replace=False))
    pos = pos[np.random.default_rng(1).permutation(n)].astype(np.uint32)
    buf, dst = _guarded(slots, chunk)
    chunk_scatter(_dev(src_h.reshape(-1)), dst, pos, chunk)      # src longer than n chunks
    ref = np.full((slots, chunk), G.SENTINEL, dtype=np.uint8)
    ref[pos] = src_h[:n]
    _check_guarded(buf, ref, chunk, "partial")
    # as a device tensor of int32, the other form the wrapper takes
    buf, dst = _guarded(slots, chunk)
    chunk_scatter(_dev(src_h.reshape(-1)), dst, _dev(pos.view(np.int32)), chunk)
    _check_guarded(buf, ref, chunk, "partial, device pos")


@pytest.mark.parametrize("chunk", [16, 4112, 12288])
def test_gather_repeated_indices(S, chunk):
    from nvme_strom_amd.ops.reorder import chunk_gather
    nsrc, n = 13, 97
    src_h = _rand(nsrc * chunk, chunk + 1).reshape(nsrc, chunk)
    idx = np.random.default_rng(chunk).integers(0, nsrc, n).astype(np.uint32)
    idx[:3] = 12
    assert len(set(idx.tolist())) < n
    buf, dst = _guarded(n + 5, chunk)                           # dst longer than n chunks
    chunk_gather(_dev(src_h.reshape(-1)), dst, idx, chunk)
    ref = np.full((n + 5, chunk), G.SENTINEL, dtype=np.uint8)
    ref[:n] = src_h[idx]
    _check_guarded(buf, ref, chunk, "repeated")


def test_scatter_gather_refusals(S):
    from nvme_strom_amd.ops.reorder import chunk_gather, chunk_scatter
    chunk, n = 4096, 8
    src = _dev(_rand(n * chunk, 31))
    buf, dst = _guarded(n, chunk)
    pos = np.arange(n, dtype=np.uint32)
    far = pos.copy()
    far[3] = n
    with pytest.raises(ValueError):
        chunk_scatter(src, dst, far, chunk)
    with pytest.raises(ValueError):
        chunk_gather(src, dst, far, chunk)
    with pytest.raises(ValueError):
        chunk_scatter(src[:-chunk], dst, pos, chunk)             # more chunks than src holds
    with pytest.raises(ValueError):
        chunk_gather(src, dst[:-chunk], pos, chunk)              # more chunks than dst holds
    s24 = _dev(_rand(24 * 4, 32))
    d24 = torch.full((24 * 4,), G.SENTINEL, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match=r"rc=-22"):
        chunk_scatter(s24, d24, np.arange(4, dtype=np.uint32), 24)
    with pytest.raises(RuntimeError, match=r"rc=-22"):
        chunk_gather(s24, d24, np.arange(4, dtype=np.uint32), 24)
    with pytest.raises(RuntimeError, match=r"rc=-22"):
        chunk_scatter(src[4:4 + chunk], dst, pos[:1], chunk)     # source not 16-aligned
    torch.cuda.synchronize()
    assert bool((buf == G.SENTINEL).all()) and bool((d24 == G.SENTINEL).all())


# ---------------------------------------------------------------- fill / verify
@pytest.mark.parametrize("off", [16, 1040])
@pytest.mark.parametrize("cid,nbytes", G.VERIFY_CASES, ids=[c[0] for c in G.VERIFY_CASES])
def test_fill_stays_inside(S, V, cid, nbytes, off):
    buf = torch.full((off + nbytes + 4096,), G.SENTINEL, dtype=torch.uint8, device="cuda")
    inner = buf[off:off + nbytes]
    V.fill_pattern(inner, G.FILL_PATTERN)
    assert V.verify_pattern(inner, G.FILL_PATTERN) == (0, -1)
    h = buf.cpu().numpy()
    assert np.all(h[:off] == G.SENTINEL) and np.all(h[off + nbytes:] == G.SENTINEL)
    assert np.all(h[off:off + nbytes].view("<u4") == G.FILL_PATTERN)
    assert G.mismatch_reference(h[off:off + nbytes], G.FILL_PATTERN) == (0, -1)


def _run_plantings(host, verify):
    """Every planting of integritygen.plantings on the writable byte array
    ``host`` (put back afterwards); ``verify(host)`` -> (device result twice,
    numpy reference)."""
    words = host.view("<u4")
    for label, idx in G.plantings(len(words)):
        saved = words[idx].copy()
        words[idx] ^= np.uint32(1) << ((idx * 7) % 32).astype(np.uint32)
        first, second, want = verify(host, repeat=not label.startswith("edge-"))
        words[idx] = saved
        assert want[0] == len(idx) and want[1] == int(idx[0]) * 4, label
        assert first == want, label
        assert second == want, (label, "second run")


@pytest.mark.parametrize("cid,nbytes", G.VERIFY_CASES, ids=[c[0] for c in G.VERIFY_CASES])
def test_verify_pattern_case(S, V, cid, nbytes):
    pat = 0x41424344
    host = np.full(nbytes // 4, pat, dtype="<u4").view(np.uint8)
    assert V.verify_pattern(_dev(host), pat) == (0, -1)

    def verify(h, repeat):
        d = _dev(h)
        r = V.verify_pattern(d, pat)
        return r, (V.verify_pattern(d, pat) if repeat else r), G.mismatch_reference(h, pat)
    _run_plantings(host, verify)
    # another pattern: every word differs
    assert V.verify_pattern(_dev(host), pat ^ 0x01000000) == (nbytes // 4, 0 if nbytes else -1)


@pytest.mark.parametrize("cid,nbytes", G.VERIFY_CASES, ids=[c[0] for c in G.VERIFY_CASES])
def test_verify_equal_case(S, V, cid, nbytes):
    clean = _rand(nbytes, nbytes + 5)
    host = clean.copy()
    b = _dev(clean)
    assert V.verify_equal(_dev(host), b) == (0, -1)

    def verify(h, repeat):
        a = _dev(h)
        r = V.verify_equal(a, b)
        return r, (V.verify_equal(b, a) if repeat else r), G.mismatch_reference(h, clean)
    _run_plantings(host, verify)
    assert np.array_equal(host, clean)


def test_verify_refusals(S, V):
    t = torch.full((4096 + 16,), G.SENTINEL, dtype=torch.uint8, device="cuda")
    for bad in (t[:6], t[:4097], t[4:20]):                       # not whole words; not 16-aligned
        with pytest.raises(RuntimeError, match=r"rc=-22"):
            V.verify_pattern(bad, 0)
        with pytest.raises(RuntimeError, match=r"rc=-22"):
            V.fill_pattern(bad, 0)
        with pytest.raises(RuntimeError, match=r"rc=-22"):
            V.verify_equal(bad, bad.clone() if bad.data_ptr() % 16 == 0 else bad)
    with pytest.raises(ValueError):
        V.verify_equal(t[:16], t[:32])
    torch.cuda.synchronize()
    assert bool((t == G.SENTINEL).all())
