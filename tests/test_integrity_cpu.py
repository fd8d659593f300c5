"""The references and case lists of tests/integritygen.py, without a GPU:
the bit-at-a-time CRC32C against the host CRC, and proof (from the kernels'
launch arithmetic, mirrored in integritygen.schedule / combine_per) that the
case lists of test_gpu_integrity.py reach every schedule of crc32c.hip and
every copy / verify path of copyops.hip.  The coverage tests are conditions
on the lists, not measurements."""
import numpy as np
import pytest

import integritygen as G
import nvme_strom_amd as S


# ---------------------------------------------------------------- reference
@pytest.mark.parametrize("data,crc", [(b"", 0), (b"123456789", 0xE3069283),
                                      (bytes(32), 0x8A9136AA)])
def test_bitwise_known_vectors(data, crc):
    assert G.crc32c_bitwise(data) == crc
    assert S.crc32c_host(data) == crc


def test_bitwise_equals_host_on_random_lengths():
    rng = np.random.default_rng(7)
    lens = [0, 1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 4095, 4096] + rng.integers(0, 4097, 24).tolist()
    for n in lens:
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert G.crc32c_bitwise(d) == S.crc32c_host(d), n


def test_bitwise_running_crc():
    rng = np.random.default_rng(8)
    d = rng.integers(0, 256, 3000, dtype=np.uint8).tobytes()
    whole = G.crc32c_bitwise(d)
    for cut in (0, 1, 7, 8, 1024, 2999, 3000):
        assert G.crc32c_bitwise(d[cut:], G.crc32c_bitwise(d[:cut])) == whole, cut
        assert S.crc32c_host(d[cut:], S.crc32c_host(d[:cut])) == whole, cut
        assert G.crc32c_bitwise(d[cut:], S.crc32c_host(d[:cut])) == whole, cut


def test_make_data_kinds():
    assert G.make_data("zeros", 5).tolist() == [0] * 5
    assert G.make_data("ones", 3).tolist() == [255] * 3
    a = G.make_data("onebit:4", 9)
    assert np.flatnonzero(a).tolist() == [4] and bin(int(a[4])).count("1") == 1
    assert np.array_equal(G.make_data("random", 100, 3), G.make_data("random", 100, 3))
    with pytest.raises(ValueError):
        G.make_data("noise", 4)


# ---------------------------------------------------------------- CRC coverage
def _sched():
    return {cid: G.schedule(n, chunk) for cid, n, chunk, _ in G.CRC_CASES}


def test_crc_case_ids_unique_and_valid():
    ids = [c[0] for c in G.CRC_CASES]
    assert len(ids) == len(set(ids))
    for cid, n, chunk, kind in G.CRC_CASES:
        assert n > 0 and chunk % 16 == 0, cid
        assert n <= 40 << 20, cid
        assert G.make_data(kind, min(n, 70000)).dtype == np.uint8
        if kind.startswith("onebit:"):
            assert int(kind.split(":")[1]) < n, cid


def test_schedule_mirror_examples():
    # worked by hand from the launch arithmetic
    assert G.schedule(1 << 30, 1 << 16) == (False, 16, 256, 16384, True)
    assert G.schedule(1 << 30, 1 << 20) == (True, 16, 256, 1024, True)
    assert G.schedule(25 * 4096, 4096) == (False, 1, 25, 25, False)
    assert G.schedule(257 * 16, 16) == (False, 2, 129, 257, False)
    assert G.schedule(4096 * 16, 16) == (False, 16, 256, 4096, False)
    assert G.schedule(4097 * 16, 16) == (False, 16, 256, 4097, True)
    assert G.schedule(16384, 16384) == (True, 16, 1, 1, False)
    assert [G.combine_per(k) for k in (1, 1024, 1025, 7168, 7169, 8192, 8193, 16384)] == \
        [1, 1, 2, 7, 8, 8, 9, 16]


def test_crc_cases_reach_every_wave_schedule():
    wave = {cid: s for cid, s in _sched().items() if not s[0]}
    wpbs = {s[1] for s in wave.values()}
    assert 1 in wpbs and 16 in wpbs and any(2 <= w <= 15 for w in wpbs), wpbs
    # several waves per workgroup without and with a second chunk per wave
    assert any(s[1] > 1 and not s[4] for s in wave.values())
    assert sum(s[4] for s in wave.values()) >= 2
    # in the strided cases the second pass of some wave ends on a short chunk
    for cid, n, chunk, _ in G.CRC_CASES:
        if cid.startswith("wave-stride"):
            _, wpb, grid, nch, strides = G.schedule(n, chunk)
            assert strides and nch - 1 >= grid * wpb and n % chunk, cid


def test_crc_cases_reach_every_split_schedule():
    sched = _sched()
    split = {cid: s for cid, s in sched.items() if s[0]}
    assert any(s[2] < s[3] for s in split.values())            # grid < nchunks
    assert any(s[3] == 1 for s in split.values())
    # both sides of the boundary at chunk 16384, and chunk 16368 in wave mode
    by_shape = {(n, chunk): G.schedule(n, chunk) for _, n, chunk, _ in G.CRC_CASES}
    assert by_shape[16384 * 2047, 16384][0] is True and by_shape[16384 * 2047, 16384][3] == 2047
    assert by_shape[16384 * 2048, 16384][0] is False and by_shape[16384 * 2048, 16384][3] == 2048
    assert any(chunk == 16368 and not G.schedule(n, chunk)[0] and G.schedule(n, chunk)[3] == 300
               for _, n, chunk, _ in G.CRC_CASES)
    # a chunk whose parts leave waves empty, and non-first parts of 1..3 and
    # 4..15 bytes (part length: the chunk over 16 waves, rounded up to 1 KiB)
    shapes = set()
    for cid, n, chunk, _ in G.CRC_CASES:
        if sched[cid][0] and sched[cid][3] == 1:
            plen = ((n + 15) // 16 + 1023) // 1024 * 1024
            parts = [min(plen, n - lo) for lo in range(0, n, plen)]
            if len(parts) < 16:
                shapes.add("empty-waves")
            if len(parts) > 1 and 1 <= parts[-1] <= 3:
                shapes.add("last-1-3")
            if len(parts) > 1 and 4 <= parts[-1] <= 15:
                shapes.add("last-4-15")
            if len(parts) == 16 and parts[-1] == plen:
                shapes.add("full")
    assert shapes == {"empty-waves", "last-1-3", "last-4-15", "full"}


def test_structured_cases_run_in_both_schedules():
    sched = _sched()
    for kind in ("zeros", "ones", "onebit"):
        got = {sched[cid][0] for cid, _, _, k in G.CRC_CASES if k.startswith(kind)}
        assert got == {False, True}, kind
    for name in ("wave", "split"):
        for kind in ("zeros", "ones"):
            assert len([1 for cid, *_ in G.CRC_CASES if cid.startswith(f"{kind}-{name}-")]) == 3
        offs = {int(k.split(":")[1]) for cid, n, _, k in G.CRC_CASES
                if cid.startswith(f"onebit-{name}-")}
        n = G.ONEBIT_LEN[name]
        assert offs == {0, 3, 4, 15, 16, 1023, 1024, G.ONEBIT_SECOND_PART, n - 1}
    # the second split part starts where the first one ends
    n = G.ONEBIT_LEN["split"]
    assert ((n + 15) // 16 + 1023) // 1024 * 1024 == G.ONEBIT_SECOND_PART


def test_crc_cases_reach_every_combine_class():
    pers = {}
    for cid, n, chunk, _ in G.CRC_CASES:
        per = G.combine_per(G.schedule(n, chunk)[3])
        pers.setdefault(per, set()).add(bool(n % chunk))
    assert 1 in pers and 8 in pers
    assert any(2 <= p <= 7 for p in pers) and any(p > 8 for p in pers)
    for per, tails in pers.items():
        if per > 1:
            assert tails == {False, True}, per


def test_combine_cases():
    assert {k for _, k in G.COMBINE_CASES} == set(G.COMBINE_NCHUNKS)
    assert {c for c, _ in G.COMBINE_CASES} == {16, 4096}
    pers = {G.combine_per(k) for _, k in G.COMBINE_CASES}
    assert {1, 2, 3, 7, 8, 9, 17} <= pers
    for chunk, k in G.COMBINE_CASES:
        lens = G.combine_lengths(chunk, k)
        assert max(lens) == chunk * k <= 40 << 20
        assert all((n + chunk - 1) // chunk == k for n in lens)
        if k > 1:
            assert sorted(n % chunk for n in lens) == [0, 1, 3, chunk - 1]
    # the thread that holds the partial tail chunk sees it inside a group of
    # eight (per 8), after one (per 9) and behind idle threads (1025: per 2)
    assert G.combine_per(8192) == 8 and 8192 % 8 == 0
    assert G.combine_per(1025) * 1024 > 1025 + G.combine_per(1025)


def test_sweep_lengths():
    assert max(G.SWEEP_LENGTHS) < G.SWEEP_BUF and G.SWEEP_BUF % G.SWEEP_CHUNK == 0
    for L in G.SWEEP_LENGTHS:
        split, wpb, _, _, strides = G.schedule(L, G.SWEEP_CHUNK)
        assert (split, wpb, strides) == (False, 1, False)


# ---------------------------------------------------------------- copyops coverage
def test_copy_cases():
    ids = [c[0] for c in G.COPY_CASES]
    assert len(ids) == len(set(ids))
    nvecs = {chunk // 16 for _, chunk, _ in G.COPY_CASES}
    assert all(chunk % 16 == 0 for _, chunk, _ in G.COPY_CASES)
    assert any(v < 256 for v in nvecs) and 768 in nvecs and 256 in nvecs
    assert any(v > 1024 and v % 256 for v in nvecs)
    assert {n for _, _, n in G.COPY_CASES} == {1, 97, 4097}
    assert {chunk for _, chunk, n in G.COPY_CASES if n > 4096} == {16, 4112}
    assert max(chunk * n for _, chunk, n in G.COPY_CASES) <= 40 << 20
    for kind in G.COPY_PERMS:
        assert sorted(G.make_perm(kind, 97).tolist()) == list(range(97))
    assert G.make_perm("reverse", 3).tolist() == [2, 1, 0]


def test_verify_cases():
    sizes = [n for _, n in G.VERIFY_CASES]
    assert all(n % 4 == 0 for n in sizes) and {0, 4, 12} <= set(sizes)
    assert any(n // 4 % 4 for n in sizes) and any(n // 4 % 4 == 0 and n for n in sizes)
    # more 16-byte vectors than 1024 blocks of 1024 take at the natural grid
    assert sum(n // 16 + 1 > 1024 * 1024 for n in sizes) >= 2
    assert max(sizes) <= 40 << 20
    for n in (4, 12, 20, 4100, (1 << 20) + 12):
        nw = n // 4
        seen = {}
        for label, words in G.plantings(nw):
            assert label not in seen, label
            seen[label] = words
            assert len(words) and words.min() >= 0 and words.max() < nw, (n, label)
            assert np.array_equal(np.unique(words), words), (n, label)
        assert len(seen["all"]) == nw and seen["last"].tolist() == [nw - 1]
        if nw % 4:
            assert seen["tail"].tolist() == list(range(nw // 4 * 4, nw))
        if nw >= 8:
            assert all(w.min() >= nw // 2 for k, w in seen.items() if k.startswith("upper"))
    big = dict(G.plantings(((1 << 20) + 12) // 4))
    assert "random-100000-s1" in big and "edge-4096" in big and "edge-4092" in big
    assert f"edge-{1 << 20}" in big and f"edge-{(1 << 20) - 4}" in big
    assert list(G.plantings(0)) == []


def test_mismatch_reference():
    a = np.zeros(20, dtype=np.uint8)
    assert G.mismatch_reference(a, 0) == (0, -1)
    assert G.mismatch_reference(a, 1) == (5, 0)
    b = a.copy()
    b[7] = 1
    b[16] = 2
    assert G.mismatch_reference(a, b) == (2, 4)
    assert G.mismatch_reference(b, 0) == (2, 4)
    c = np.frombuffer(bytes([4, 3, 2, 1] * 2), dtype=np.uint8)
    assert G.mismatch_reference(c, 0x01020304) == (0, -1)
    assert G.mismatch_reference(np.zeros(0, dtype=np.uint8), 5) == (0, -1)
