"""Shared inputs of the integrity-kernel tests (test_integrity_cpu.py,
test_gpu_integrity.py): a table-less CRC32C reference, the launch arithmetic
of the CRC kernels as plain Python, and the named case lists for
csrc/kernels/crc32c.hip and csrc/kernels/copyops.hip.

The launch arithmetic is here only so the CPU test can prove that the case
lists reach every schedule of the kernels.  No GPU expectation is computed
from it: every expected value comes from ``crc32c_bitwise``, the host CRC or
numpy.
"""
from __future__ import annotations

import numpy as np

# ---------------------------------------------------------------- reference
POLY = 0x82F63B78


def crc32c_bitwise(data, crc: int = 0) -> int:
    """CRC32C (Castagnoli, reflected), one bit at a time: init and final xor
    of ~0, ``crc`` continues a running CRC.  Shares nothing with the host
    tables or the kernel; for inputs of a few KiB."""
    c = (crc ^ 0xFFFFFFFF) & 0xFFFFFFFF
    for byte in bytes(data):
        c ^= byte
        for _ in range(8):
            c = (c >> 1) ^ POLY if c & 1 else c >> 1
    return c ^ 0xFFFFFFFF


# ---------------------------------------------------------------- schedules
# Mirrors of the launch arithmetic of strom_crc32c_chunks
# (csrc/kernels/crc32c.hip:325-336, from `const bool split` to the grid clamp) and of `per` in crc32c_combine_kernel
# (csrc/kernels/crc32c.hip:265).  Coverage bookkeeping only.
K_WAVES = 16
MAX_GRID = 256
COMBINE_THREADS = 1024


def schedule(n: int, chunk: int):
    """-> (split, wpb, grid, nchunks, strides): the schedule a buffer of
    ``n`` bytes takes at ``chunk``; ``strides`` says whether any wave (wave
    mode) or workgroup (split) takes a second chunk."""
    nch = (n + chunk - 1) // chunk
    split = nch < MAX_GRID * 8 and chunk >= 16384
    if split:
        wpb = K_WAVES
        grid = min(nch, MAX_GRID)
        strides = grid < nch
    else:
        wpb = min(K_WAVES, max(1, (nch + MAX_GRID - 1) // MAX_GRID))
        grid = min(MAX_GRID, (nch + wpb - 1) // wpb)
        strides = grid * wpb < nch
    return split, wpb, grid, nch, strides


def combine_per(nchunks: int) -> int:
    """Chunks folded by one thread of the combine kernel."""
    return (nchunks + COMBINE_THREADS - 1) // COMBINE_THREADS


# ---------------------------------------------------------------- data
SENTINEL = 0xA5


def make_data(kind: str, n: int, seed: int = 0) -> np.ndarray:
    """``n`` bytes of ``random``, ``zeros``, ``ones`` (0xFF) or
    ``onebit:<byte offset>`` (a single set bit in a zero buffer)."""
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8)
    if kind == "zeros":
        return np.zeros(n, dtype=np.uint8)
    if kind == "ones":
        return np.full(n, 0xFF, dtype=np.uint8)
    if kind.startswith("onebit:"):
        a = np.zeros(n, dtype=np.uint8)
        a[int(kind.split(":")[1])] = 0x10
        return a
    raise ValueError(kind)


# ---------------------------------------------------------------- CRC cases
# (id, n, chunk, data_kind)
_SPLIT_16K = [16384, 1025, 1027, 1028, 1039, 1040]
_SPLIT_1M = [1, 3, 4, 1023, 1024, 1025, 16383, 16385, 16 * 1024 + 1027, (1 << 20) - 1]

# structured data: one wave-mode shape and one split shape; the split shape's
# parts are 3072 bytes long at L = 40000 (ceil(40000 / 16) rounded up to 1 KiB)
STRUCT_WAVE = (8192, [3, 5000, 2 * 8192 + 1039])       # chunk, lengths
STRUCT_SPLIT = (65536, [3, 40000, 65536 + 1027])
ONEBIT_LEN = {"wave": 5000, "split": 40000}
ONEBIT_SECOND_PART = 3072
ONEBIT_OFFSETS = [0, 3, 4, 15, 16, 1023, 1024, ONEBIT_SECOND_PART]


def _struct_cases():
    out = []
    for name, (chunk, lens) in (("wave", STRUCT_WAVE), ("split", STRUCT_SPLIT)):
        for kind in ("zeros", "ones"):
            out += [(f"{kind}-{name}-{n}", n, chunk, kind) for n in lens]
        n = ONEBIT_LEN[name]
        out += [(f"onebit-{name}-{o}", n, chunk, f"onebit:{o}") for o in ONEBIT_OFFSETS + [n - 1]]
    return out


CRC_CASES = [
    # wave per chunk, several waves per workgroup
    ("wave-wpb4-c16", 16 * 1000 + 5, 16, "random"),
    # 8 KiB + 1 KiB + 48: the 8-row loop, the single-row loop and q = 3
    ("wave-wpb2-c9264", 9264 * 300 + 9263, 9264, "random"),
    # wave per chunk, grid-stride (the strided iteration lands on a 3-byte chunk)
    ("wave-stride-c16", 16 * 4097 + 3, 16, "random"),
    ("wave-stride-c1040", 1040 * 5000 + 1029, 1040, "random"),
    # workgroup per chunk, grid-stride
    ("split-stride-c16384", 16384 * 300 + 3, 16384, "random"),
    # both sides of the split/wave boundary
    ("split-2047", 16384 * 2047, 16384, "random"),
    ("wave-2048", 16384 * 2048, 16384, "random"),
    ("wave-c16368", 16368 * 300, 16368, "random"),
    # split parts: empty waves (plen 2048, a ninth wave of 16 bytes)
    ("split-part-c16400", 16400, 16400, "random"),
] + [(f"split-part-16k-{L}", L, 16384, "random") for L in _SPLIT_16K] \
  + [(f"split-part-1m-{L}", L, 1 << 20, "random") for L in _SPLIT_1M] + [
    # the fold kernel with 8 and more chunks per thread, end to end
    ("fold-per2-tail", 16 * 1500 + 7, 16, "random"),
    ("fold-per5-exact", 16 * 4098, 16, "random"),
    ("fold-per8-exact", 16 * 8192, 16, "random"),
    ("fold-per8-tail", 16 * 8191 + 3, 16, "random"),
    ("fold-per9-exact", 16 * 9000, 16, "random"),
    ("fold-per9-tail", 16 * 8999 + 15, 16, "random"),
    ("fold-per17-exact", 16 * 16385, 16, "random"),
    ("fold-per17-tail", 16 * 16384 + 1, 16, "random"),
] + _struct_cases()

# wave-mode length sweep: one 4 KiB buffer, nbytes=L, chunk 2048
SWEEP_CHUNK = 2048
SWEEP_BUF = 4096
SWEEP_LENGTHS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 1008, 1023, 1024, 1025, 1027, 1028, 1039,
                 1040, 2047, 2048, 2049, 4095]

# strom_crc32c_combine in isolation: (chunk, nchunks); the last chunk is
# whole or holds COMBINE_TAILS(chunk) bytes
COMBINE_NCHUNKS = [1, 2, 1023, 1024, 1025, 2049, 7168, 7169, 8192, 9000, 16385]
COMBINE_MAX_4K = 9000                       # 4 KiB chunks stay under 40 MiB
COMBINE_CASES = [(16, k) for k in COMBINE_NCHUNKS] + \
                [(4096, k) for k in COMBINE_NCHUNKS if k <= COMBINE_MAX_4K]


def combine_lengths(chunk: int, nchunks: int):
    """Buffer lengths of one combine case: the exact multiple, and for more
    than one chunk a last chunk of 1, 3 and chunk - 1 bytes."""
    full = chunk * nchunks
    if nchunks == 1:
        return [full]
    return [full] + [full - chunk + t for t in (1, 3, chunk - 1)]


# ---------------------------------------------------------------- copy cases
# (id, chunk, n): chunk / 16 = 1, 255, 256, 257, 768 (the unrolled loop is
# skipped), 1024, 1025 and 4097 vectors; n = 4097 is past the 4096-block grid
COPY_CHUNKS = [16, 4080, 4096, 4112, 12288, 16384, 16400, 65552]
COPY_CASES = [(f"c{c}-n{n}", c, n) for c in COPY_CHUNKS for n in (1, 97)] + \
             [(f"c{c}-n4097", c, 4097) for c in (16, 4112)]
COPY_PERMS = ["identity", "reverse", "random"]


def make_perm(kind: str, n: int, seed: int = 0) -> np.ndarray:
    if kind == "identity":
        return np.arange(n, dtype=np.uint32)
    if kind == "reverse":
        return np.arange(n, dtype=np.uint32)[::-1].copy()
    if kind == "random":
        return np.random.default_rng(seed).permutation(n).astype(np.uint32)
    raise ValueError(kind)


# ---------------------------------------------------------------- verify cases
# nbytes; the last two are past 1024 blocks of 1024 16-byte vectors
VERIFY_SIZES = [0, 4, 12, 16, 20, 4092, 4096, 4100, (1 << 20) + 12, (16 << 20) + 4,
                (17 << 20) + 8]
VERIFY_CASES = [(f"n{n}", n) for n in VERIFY_SIZES]
VERIFY_RANDOM_COUNTS = [1, 2, 1000, 100000]
VERIFY_SEEDS = [1, 2, 3]
FILL_PATTERN = 0x01020304


def plantings(nwords: int):
    """(label, word indices) of every mismatch planting for a buffer of
    ``nwords`` 4-byte words; indices are unique and ascending."""
    if nwords == 0:
        return
    nvec4 = nwords // 4 * 4
    yield "all", np.arange(nwords, dtype=np.int64)
    yield "word0", np.array([0], dtype=np.int64)
    yield "last", np.array([nwords - 1], dtype=np.int64)
    if nvec4 < nwords:
        yield "tail", np.arange(nvec4, nwords, dtype=np.int64)
        yield "tail-first", np.array([nvec4], dtype=np.int64)
    # byte offsets k * 4096 and k * 4096 - 4 over the whole buffer: each one
    # alone up to 1 MiB, a spread of them above, and all of them at once
    k = np.arange(1, nwords // 1024 + 2, dtype=np.int64)
    edges = np.unique(np.concatenate([[0], k * 1024, k * 1024 - 1]))
    edges = edges[edges < nwords]
    if len(edges) > 1:
        yield "edges-all", edges
        singles = edges if len(edges) <= 600 else edges[:: len(edges) // 40]
        for w in singles.tolist():
            yield f"edge-{w * 4}", np.array([w], dtype=np.int64)
    for seed in VERIFY_SEEDS:
        rng = np.random.default_rng(seed)
        for cnt in VERIFY_RANDOM_COUNTS:
            if cnt <= nwords:
                yield f"random-{cnt}-s{seed}", np.sort(rng.choice(nwords, cnt, replace=False))
        # `first` from a late block: the upper half of the buffer only
        half = nwords // 2
        for cnt in (1, 2, 1000):
            if nwords >= 8 and cnt <= nwords - half:
                yield (f"upper-{cnt}-s{seed}",
                       half + np.sort(rng.choice(nwords - half, cnt, replace=False)))


def mismatch_reference(a: np.ndarray, b) -> tuple:
    """(differing little-endian u32 words, byte offset of the first or -1) of
    two byte arrays, or of one against a 32-bit pattern."""
    wa = np.ascontiguousarray(a).view("<u4")
    wb = np.ascontiguousarray(b).view("<u4") if isinstance(b, np.ndarray) else np.uint32(b)
    bad = np.flatnonzero(wa != wb)
    return (int(bad.size), int(bad[0]) * 4 if bad.size else -1)
